// HIP_OK: a failed HIP call becomes a keto::Error (KETO_E_HIP) that names the call.
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>

#include "snapshot.hpp"

#define HIP_OK(x)                                                                                   \
    do {                                                                                            \
        hipError_t err__ = (x);                                                                     \
        if (err__ != hipSuccess)                                                                    \
            throw Error{KETO_E_HIP, std::string(#x) + ": " + hipGetErrorString(err__)};             \
    } while (0)
