"""keto_expand_encode_batch[_ids] without a GPU: ABI 8, the seven symbols, and the calls' failures on a
host-only snapshot."""
import ctypes as C
import os
import re

import numpy as np

import keto_amd
from keto_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["keto_expand_encode_batch", "keto_expand_encode_batch_ids", "keto_encoded_free", "keto_encoded_count",
           "keto_encoded_bytes", "keto_encoded_offsets", "keto_encoded_status"]
KETO_E_INVALID = -1


def _header():
    return open(os.path.join(ROOT, "include", "keto_mi355x.h")).read()


def test_abi_8_everywhere_and_the_seven_symbols_load():
    hdr = _header()
    assert int(re.search(r"#define KETO_ABI_VERSION (\d+)", hdr).group(1)) == 8
    lib = keto_amd.load()
    assert lib.keto_abi_version() == 8 == capi.KETO_ABI_VERSION
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert re.search(r"#define KETO_ENC_PROTO 0\b", hdr) and re.search(r"#define KETO_ENC_JSON +1\b", hdr)
    assert re.search(r"#define KETO_E_INVALID +\(?-1\)?", hdr)          # the code the tests below name
    assert (capi.ENC_PROTO, capi.ENC_JSON) == (0, 1)


def _host_only():
    return keto_amd.Snapshot.build([(1, "n")], [(1, "a", "r", "u")], device=-1)


def _named(s, reqs, encoding):
    keep = capi._Keep()
    arr = s._expand_reqs(keep, reqs)
    e = C.c_void_p()
    rc = s.lib.keto_expand_encode_batch(s.h, arr, C.c_uint32(len(reqs)), C.c_int32(5), C.c_uint32(encoding), C.byref(e))
    return rc, e


def _ids(s, roots, encoding):
    roots = np.asarray(roots, dtype=np.uint32)
    depths = np.zeros(len(roots), dtype=np.int32)
    e = C.c_void_p()
    rc = s.lib.keto_expand_encode_batch_ids(s.h, roots.ctypes.data_as(C.c_void_p), depths.ctypes.data_as(C.c_void_p),
                                            C.c_uint32(len(roots)), C.c_int32(5), C.c_uint32(encoding), C.byref(e))
    return rc, e


def test_host_only_snapshot_fails_like_expand_batch():
    """device = -1: the code keto_expand_batch[_ids] gives for the same requests, read from those
    calls, a message, and no handle."""
    s = _host_only()
    reqs = [(("set", "n", "a", "r"), 3)]
    keep = capi._Keep()
    a = C.c_void_p()
    want = s.lib.keto_expand_batch(s.h, s._expand_reqs(keep, reqs), C.c_uint32(1), C.c_int32(5), C.byref(a))
    assert want < 0 and not a.value
    roots = np.array([0x80000000], dtype=np.uint32)
    depths = np.zeros(1, dtype=np.int32)
    want_ids = s.lib.keto_expand_batch_ids(s.h, roots.ctypes.data_as(C.c_void_p), depths.ctypes.data_as(C.c_void_p),
                                           C.c_uint32(1), C.c_int32(5), C.byref(a))
    assert want_ids < 0 and not a.value
    for enc in (capi.ENC_PROTO, capi.ENC_JSON):
        rc, e = _named(s, reqs, enc)
        assert rc == want and not e.value
        assert s.lib.keto_last_error()
        rc, e = _ids(s, roots, enc)
        assert rc == want_ids and not e.value
        assert s.lib.keto_last_error()
    for fn in (s.expand_batch_encoded, ):
        try:
            fn(reqs, 5, "json")
        except capi.KetoError as err:
            assert err.code == want
        else:
            raise AssertionError("no error")


def test_unknown_encoding_is_invalid():
    s = _host_only()
    rc, e = _named(s, [(("set", "n", "a", "r"), 3)], 7)
    assert rc == KETO_E_INVALID and not e.value
    assert b"encoding" in s.lib.keto_last_error()
    rc, e = _ids(s, [0x80000000], 7)
    assert rc == KETO_E_INVALID and not e.value
    assert b"encoding" in s.lib.keto_last_error()


def test_free_and_accessors_take_null():
    lib = keto_amd.load()
    lib.keto_encoded_free(None)
    lib.keto_encoded_free(C.c_void_p())
    assert lib.keto_encoded_count(None) == 0
    total = C.c_uint64(99)
    assert not lib.keto_encoded_bytes(None, C.byref(total)) and total.value == 0
    assert not lib.keto_encoded_offsets(None) and not lib.keto_encoded_status(None)
