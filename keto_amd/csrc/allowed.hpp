// keto_allowed_subjects_batch (allowed.hip): the SubjectIDs a check allows on an object.  What the
// C-ABI layer needs of it.  The workspace and its stream live with the snapshot's handle
// (capi_internal.hpp), next to the flatten's, and are freed with the handle, before the snapshot's
// device state.
#pragma once

#include <memory>
#include <mutex>
#include <vector>

#include "snapshot.hpp"

namespace keto {

struct AllowedState;     // allowed.hip
struct AllowedStateDeleter {
    void operator()(AllowedState* s) const;
};
struct AllowedCache {
    std::unique_ptr<AllowedState, AllowedStateDeleter> state;
    std::mutex mu;       // the workspace: held for the whole of a call (one at a time per snapshot)
};

struct AllowedResult {
    std::vector<uint8_t> status;                        // n x KETO_ALLOWED_*
    std::vector<uint64_t> offsets, next_page, totals;   // n + 1, n, n
    std::vector<uint64_t> candidates, undecided;        // n, n
    uint32_t* ids = nullptr;                            // a block of the pinned pool (pinned_take), or NULL
    float bfs_ms = 0, dedupe_ms = 0, check_ms = 0, emit_ms = 0;
    // the BFS of the call: (query, row) keys visited, slots of the visited table at the end, levels run,
    // times the table was enlarged ahead of a level, times a level's emit ran again, forwarded rows the
    // count passes met (a level counted again after its predecessor ran again counts twice)
    uint64_t visited = 0, slots = 0, forwards = 0;
    uint32_t levels = 0, regrows = 0, reruns = 0;
};

// The caller holds the snapshot's lock shared, from before the call until it returns: the candidates,
// their checks and the page belong to one version.  Lock order: rw shared -> c.mu -> the device lock
// (device_check_rows, per chunk).  out.ids goes to the caller, who gives it back with pinned_give.
void allowed_subjects(Snapshot& s, AllowedCache& c, const keto_allowed_req* reqs, uint32_t n, int32_t global_max_depth,
                      AllowedResult& out);

}  // namespace keto
