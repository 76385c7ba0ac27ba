"""keto_allowed_subjects_batch without a GPU: the entry points exist next to an unchanged ABI version, the
ctypes struct has the header's layout, the call refuses a snapshot without a device, and the expectation
the GPU tests compare with (tests/allowed_util.py) agrees with an example worked out by hand."""
import ctypes as C
import os
import re
import subprocess

import pytest

import keto_amd
from keto_amd import capi
from oracle.oracle_sql import RelationTuple, SQLStore, SubjectID, SubjectSet
from tests import allowed_util
from tests.allowed_util import ALLOWED_OK, ALLOWED_UNKNOWN_NAMESPACE, ALLOWED_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["keto_allowed_subjects_batch", "keto_allowed_free", "keto_allowed_count", "keto_allowed_ids",
                "keto_allowed_offsets", "keto_allowed_status", "keto_allowed_next_page", "keto_allowed_totals",
                "keto_allowed_candidates", "keto_allowed_undecided", "keto_allowed_timing", "keto_allowed_bfs"]


def test_header_declares_and_library_exports_the_allowed_calls():
    hdr = open(os.path.join(ROOT, "include", "keto_mi355x.h")).read()
    lib = keto_amd.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    # every keto_allowed_* function the header declares is one of them
    assert set(re.findall(r"\b(keto_allowed_[a-z_]+)\(", hdr)) == set(ENTRY_POINTS)
    for macro, val in (("KETO_ALLOWED_OK", 0), ("KETO_ALLOWED_UNKNOWN_NAMESPACE", 1), ("KETO_ALLOWED_UNDECIDED", 2),
                       ("KETO_ALLOWED_UNSUPPORTED", 3)):
        assert re.search(r"#define %s\s+%d\b" % (macro, val), hdr), macro
    assert (capi.ALLOWED_OK, capi.ALLOWED_UNKNOWN_NAMESPACE, capi.ALLOWED_UNDECIDED, capi.ALLOWED_UNSUPPORTED) == (0, 1, 2, 3)
    for typ in ("keto_allowed_req", "keto_allowed"):
        assert re.search(r"\b%s;" % typ, hdr), typ
    # additive: the ABI version does not move
    assert int(re.search(r"#define KETO_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert lib.keto_abi_version() == 8 == capi.KETO_ABI_VERSION


def test_ctypes_struct_has_the_header_layout(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "keto_mi355x.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(keto_allowed_req), sizeof(keto_str),\n'
                   "           offsetof(keto_allowed_req, object), offsetof(keto_allowed_req, relation),\n"
                   "           offsetof(keto_allowed_req, max_depth), offsetof(keto_allowed_req, page_size),\n"
                   "           offsetof(keto_allowed_req, page));\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]
    R = capi.KAllowedReq
    assert got == [C.sizeof(R), C.sizeof(capi.KStr), R.object.offset, R.relation.offset, R.max_depth.offset,
                   R.page_size.offset, R.page.offset]


def test_allowed_needs_a_device():
    snap = keto_amd.Snapshot.build([(1, "n")], [(1, "a", "r", "u")], device=-1)
    with pytest.raises(keto_amd.KetoError) as e:
        snap.allowed_subjects([("n", "a", "r", 0, 0, 0)])
    assert e.value.code == -2                                             # KETO_E_HIP
    # n = 0 too: a host-only snapshot is KETO_E_HIP whatever n is, as for lookups
    with pytest.raises(keto_amd.KetoError) as e:
        snap.allowed_subjects_raw([])
    assert e.value.code == -2
    # and NULL arguments are refused before anything else
    lib = keto_amd.load()
    h = C.c_void_p()
    assert lib.keto_allowed_subjects_batch(snap.h, None, C.c_uint32(1), C.c_int32(5), None) == -1
    assert lib.keto_allowed_subjects_batch(snap.h, None, C.c_uint32(1), C.c_int32(5), C.byref(h)) == -1
    assert lib.keto_allowed_subjects_batch(None, None, C.c_uint32(0), C.c_int32(5), C.byref(h)) == -1


def test_null_safe_accessors():
    lib = keto_amd.load()
    total = C.c_uint64(7)
    assert lib.keto_allowed_count(None) == 0
    assert lib.keto_allowed_ids(None, C.byref(total)) is None and total.value == 0
    assert lib.keto_allowed_ids(None, None) is None
    for f in (lib.keto_allowed_offsets, lib.keto_allowed_status, lib.keto_allowed_next_page, lib.keto_allowed_totals,
              lib.keto_allowed_candidates, lib.keto_allowed_undecided):
        assert f(None) is None
    ms = [C.c_float() for _ in range(4)]
    assert lib.keto_allowed_timing(None, *[C.byref(x) for x in ms]) == -1
    assert lib.keto_allowed_bfs(None, None, None, None, None, None, None) == -1
    lib.keto_allowed_free(None)


def test_allowed_util_on_a_hand_written_example():
    """The docs / grp example of tests/test_lookup_cpu.py, asked from the object's side, with two tuples added
    so that one object has three subjects:
         docs:a#view@alice                    direct
         docs:b#view@(grp:eng#member)         indirect: eng's members
         grp:eng#member@alice
         grp:eng#member@carol                 (added)
         docs:c#view@(grp:ops#member)         indirect through two groups: ops -> eng -> alice, carol
         docs:c#view@bob                      (added) direct
         grp:ops#member@(grp:eng#member)
         docs:d#view@bob
    docs:c#view: bob at depth 1; at depth 2 the walk reads ops's row, which holds no id; alice and carol are
    two hops away and need depth 3.  docs:b#view: nobody at depth 1, alice and carol at depth 2.  "nobody" is
    no subject of the store and is never allowed."""
    ns = [(1, "docs"), (2, "grp")]
    T = RelationTuple
    eng, ops = SubjectSet("grp", "eng", "member"), SubjectSet("grp", "ops", "member")
    tuples = [T("docs", "a", "view", SubjectID("alice")), T("docs", "b", "view", eng), T("grp", "eng", "member", SubjectID("alice")),
              T("grp", "eng", "member", SubjectID("carol")), T("docs", "c", "view", ops), T("docs", "c", "view", SubjectID("bob")),
              T("grp", "ops", "member", eng), T("docs", "d", "view", SubjectID("bob"))]
    store = SQLStore(ns, tuples, page_size=2)
    assert allowed_util.subject_ids(store) == ["alice", "bob", "carol"]
    exp = lambda q, g=5: allowed_util.expected(store, q, g)
    assert exp(("docs", "c", "view", 0, 100, 0)) == (ALLOWED_OK, ["alice", "bob", "carol"], "", 3)
    assert exp(("docs", "c", "view", 3, 100, 0)) == (ALLOWED_OK, ["alice", "bob", "carol"], "", 3)
    assert exp(("docs", "c", "view", 2, 100, 0)) == (ALLOWED_OK, ["bob"], "", 1)              # one hop short
    assert exp(("docs", "c", "view", 1, 100, 0)) == (ALLOWED_OK, ["bob"], "", 1)
    assert exp(("docs", "c", "view", 0, 100, 0), g=2) == (ALLOWED_OK, ["bob"], "", 1)         # the global depth clamps
    assert exp(("docs", "c", "view", 7, 100, 0), g=2) == (ALLOWED_OK, ["bob"], "", 1)         # > global -> global
    assert exp(("docs", "c", "view", 7, 100, 0), g=3) == (ALLOWED_OK, ["alice", "bob", "carol"], "", 3)
    assert exp(("docs", "b", "view", 1, 100, 0)) == (ALLOWED_OK, [], "", 0)
    assert exp(("docs", "b", "view", 2, 100, 0)) == (ALLOWED_OK, ["alice", "carol"], "", 2)
    assert exp(("docs", "a", "view", 1, 100, 0)) == (ALLOWED_OK, ["alice"], "", 1)
    assert exp(("docs", "d", "view", 0, 100, 0)) == (ALLOWED_OK, ["bob"], "", 1)
    assert exp(("grp", "ops", "member", 0, 100, 0)) == (ALLOWED_OK, ["alice", "carol"], "", 2)
    assert exp(("docs", "zz", "view", 0, 100, 0)) == (ALLOWED_OK, [], "", 0)                   # no such object
    assert exp(("docs", "c", "edit", 0, 100, 0)) == (ALLOWED_OK, [], "", 0)
    assert exp(("nope", "c", "view", 0, 100, 0)) == (ALLOWED_UNKNOWN_NAMESPACE, [], "", 0)
    assert exp(("docs", "", "view", 0, 100, 0)) == (ALLOWED_UNSUPPORTED, [], "", 0)
    # pages: size 0 is the store's page size (2); the token is "" on the last page and past the end
    assert exp(("docs", "c", "view", 0, 0, 0)) == (ALLOWED_OK, ["alice", "bob"], "2", 3)
    assert exp(("docs", "c", "view", 0, 0, 2)) == (ALLOWED_OK, ["carol"], "", 3)
    assert exp(("docs", "c", "view", 0, 0, 3)) == (ALLOWED_OK, [], "", 3)
    assert exp(("docs", "c", "view", 0, 1, 2)) == (ALLOWED_OK, ["bob"], "3", 3)
