"""keto_tree_json_all_device without a GPU: the symbol, and its failure on a host-only snapshot."""
import ctypes as C
import os
import re

import numpy as np

import keto_amd
from keto_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_symbol():
    hdr = open(os.path.join(ROOT, "include", "keto_mi355x.h")).read()
    assert re.search(r"^int64_t keto_tree_json_all_device\(keto_snapshot\* s, const keto_tree_arena\* a, char\* buf, "
                     r"uint64_t cap,\s*uint64_t\* offsets\);", hdr, re.M)
    lib = keto_amd.load()
    assert hasattr(lib, "keto_tree_json_all_device")
    assert "keto_tree_json_all_device" in capi.EXPORTS
    assert lib.keto_tree_json_all_device.restype is C.c_int64


def test_bytes_names_are_stored_as_they_are():
    """Names may be bytes (any byte sequence, invalid UTF-8 included) as well as str."""
    s = keto_amd.Snapshot.build([(1, b"n\xff")], [(1, b"\xe2\x82", "r", b"ok\xe2"), (1, "a", "r", "u")], device=-1)
    assert s.stats()["n_tuples"] == 2
    blob, packed = capi.pack_requests([(b"n\xff", "a", "r", ("id", b"\xc0\x80"), 3)])
    assert blob == b"n\xffar\xc0\x80" and packed[0]["len"].tolist() == [2, 1, 1, 2, 0, 0]


def test_null_runs_stand_alone_under_sanitizers(tmp_path):
    """The host side of the per-tree offsets (json_runs.hpp: the "null" bytes of node-less trees in
    front of each tree) in a stand-alone program built with the address and undefined-behaviour
    sanitizers: random batches against the definition."""
    import subprocess
    exe = str(tmp_path / "json_runs_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",        # the runtimes inside the program
                           "-I", os.path.join(ROOT, "keto_amd", "csrc"),
                           os.path.join(ROOT, "tools", "dev", "json_runs_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 0, out.stderr.decode()
    assert b"batches ok" in out.stdout


def test_host_only_snapshot_fails_like_the_proto_encoder():
    """A host-only snapshot (device = -1): the negative code keto_tree_proto_all_device gives for the
    same arguments, read from that call, and a message.  Without a device no arena can be made
    (keto_expand_batch fails), so the arena is NULL here; tests/test_gpu_json_device.py repeats this
    with a real arena."""
    s = keto_amd.Snapshot.build([(1, "n")], [(1, "a", "r", "u")], device=-1)
    lib = s.lib
    offs = np.zeros(2, dtype=np.uint64)
    a = C.c_void_p()
    assert lib.keto_expand_batch(s.h, None, C.c_uint32(0), C.c_int32(5), C.byref(a)) < 0 and not a.value
    want = lib.keto_tree_proto_all_device(s.h, a, None, C.c_uint64(0), offs.ctypes.data_as(C.c_void_p))
    assert want < 0
    got = lib.keto_tree_json_all_device(s.h, a, None, C.c_uint64(0), offs.ctypes.data_as(C.c_void_p))
    assert got == want
    assert lib.keto_last_error()
