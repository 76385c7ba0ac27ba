"""keto_lookup_objects_batch without a GPU: the entry points exist next to an unchanged ABI version, the
ctypes structs have the header's sizes, the call refuses a snapshot without a device, and the expectation
the GPU tests compare with (tests/lookup_util.py) agrees with an example worked out by hand."""
import ctypes as C
import os
import re
import subprocess

import pytest

import keto_amd
from keto_amd import capi
from oracle.oracle_sql import RelationTuple, SQLStore, SubjectID, SubjectSet
from tests import lookup_util
from tests.lookup_util import LOOKUP_OK, LOOKUP_UNKNOWN_NAMESPACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["keto_lookup_objects_batch", "keto_looked_free", "keto_looked_count", "keto_looked_rows",
                "keto_looked_offsets", "keto_looked_status", "keto_looked_next_page", "keto_looked_totals",
                "keto_looked_candidates", "keto_looked_undecided", "keto_looked_timing"]


def test_header_declares_and_library_exports_the_lookup_calls():
    hdr = open(os.path.join(ROOT, "include", "keto_mi355x.h")).read()
    lib = keto_amd.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    # every keto_lookup* / keto_looked* function the header declares is one of them
    assert set(re.findall(r"\b(keto_look(?:up|ed)_[a-z_]+)\(", hdr)) == set(ENTRY_POINTS)
    for macro, val in (("KETO_LOOKUP_OK", 0), ("KETO_LOOKUP_UNKNOWN_NAMESPACE", 1), ("KETO_LOOKUP_UNDECIDED", 2),
                       ("KETO_LOOKUP_UNSUPPORTED", 3)):
        assert re.search(r"#define %s\s+%d\b" % (macro, val), hdr), macro
    assert (capi.LOOKUP_OK, capi.LOOKUP_UNKNOWN_NAMESPACE, capi.LOOKUP_UNDECIDED, capi.LOOKUP_UNSUPPORTED) == (0, 1, 2, 3)
    for typ in ("keto_lookup_req", "keto_looked"):
        assert re.search(r"\b%s;" % typ, hdr), typ
    # additive: the ABI version does not move
    assert int(re.search(r"#define KETO_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert lib.keto_abi_version() == 8 == capi.KETO_ABI_VERSION


def test_ctypes_structs_have_the_header_sizes(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "keto_mi355x.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(keto_lookup_req), sizeof(keto_subject), sizeof(keto_str),\n'
                   "           offsetof(keto_lookup_req, relation), offsetof(keto_lookup_req, subject),\n"
                   "           offsetof(keto_lookup_req, max_depth), offsetof(keto_lookup_req, page));\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]
    R = capi.KLookupReq
    assert got == [C.sizeof(R), C.sizeof(capi.KSubject), C.sizeof(capi.KStr), R.relation.offset, R.subject.offset,
                   R.max_depth.offset, R.page.offset]


def test_lookup_needs_a_device():
    snap = keto_amd.Snapshot.build([(1, "n")], [(1, "a", "r", "u")], device=-1)
    with pytest.raises(keto_amd.KetoError) as e:
        snap.lookup_objects([("n", "r", ("id", "u"), 0, 0, 0)])
    assert e.value.code == -2                                             # KETO_E_HIP
    # n = 0 too: a host-only snapshot is KETO_E_HIP whatever n is, as for lists
    with pytest.raises(keto_amd.KetoError) as e:
        snap.lookup_objects_raw([])
    assert e.value.code == -2
    with pytest.raises(keto_amd.KetoError) as e:
        snap.list_batch_raw([])
    assert e.value.code == -2
    # and NULL arguments are refused before anything else
    lib = keto_amd.load()
    assert lib.keto_lookup_objects_batch(snap.h, None, C.c_uint32(1), C.c_int32(5), None) == -1
    assert lib.keto_looked_count(None) == 0 and lib.keto_looked_rows(None, None) is None
    lib.keto_looked_free(None)


def test_lookup_util_on_a_hand_written_example():
    """Six tuples; who has `view` on which doc?
         docs:a#view@alice                    direct
         docs:b#view@(grp:eng#member)         indirect: alice is a member of eng
         grp:eng#member@alice
         docs:c#view@(grp:ops#member)         indirect through two groups: ops -> eng -> alice
         grp:ops#member@(grp:eng#member)
         docs:d#view@bob                      not alice's
    alice: a (depth 1), b (needs depth 2), c (needs depth 3).  At request depth 2 the walk for c stops one
    hop short: denied by depth.  bob: d only.  The subject set grp:eng#member itself: b directly, c at depth 2."""
    ns = [(1, "docs"), (2, "grp")]
    T = RelationTuple
    eng, ops = SubjectSet("grp", "eng", "member"), SubjectSet("grp", "ops", "member")
    tuples = [T("docs", "a", "view", SubjectID("alice")), T("docs", "b", "view", eng), T("grp", "eng", "member", SubjectID("alice")),
              T("docs", "c", "view", ops), T("grp", "ops", "member", eng), T("docs", "d", "view", SubjectID("bob"))]
    store = SQLStore(ns, tuples, page_size=2)
    alice, bob = SubjectID("alice"), SubjectID("bob")
    exp = lambda q, g=5: lookup_util.expected(store, q, g)
    assert exp(("docs", "view", alice, 0, 100, 0)) == (LOOKUP_OK, ["a", "b", "c"], "", 3, 4, 0)
    assert exp(("docs", "view", alice, 2, 100, 0)) == (LOOKUP_OK, ["a", "b"], "", 2, 4, 0)       # c denied by depth
    assert exp(("docs", "view", alice, 1, 100, 0)) == (LOOKUP_OK, ["a"], "", 1, 4, 0)
    assert exp(("docs", "view", alice, 0, 100, 0), g=2) == (LOOKUP_OK, ["a", "b"], "", 2, 4, 0)  # the global depth clamps
    assert exp(("docs", "view", alice, 7, 100, 0), g=2) == (LOOKUP_OK, ["a", "b"], "", 2, 4, 0)  # > global -> global
    assert exp(("docs", "view", bob, 0, 100, 0)) == (LOOKUP_OK, ["d"], "", 1, 4, 0)
    assert exp(("docs", "view", eng, 0, 100, 0)) == (LOOKUP_OK, ["b", "c"], "", 2, 4, 0)
    assert exp(("docs", "view", SubjectID("nobody"), 0, 100, 0)) == (LOOKUP_OK, [], "", 0, 4, 0)
    assert exp(("docs", "edit", alice, 0, 100, 0)) == (LOOKUP_OK, [], "", 0, 0, 0)
    assert exp(("nope", "view", alice, 0, 100, 0)) == (LOOKUP_UNKNOWN_NAMESPACE, [], "", 0, 0, 0)
    # pages: size 0 is the store's page size (2); the token is "" on the last page and past the end
    assert exp(("docs", "view", alice, 0, 0, 0)) == (LOOKUP_OK, ["a", "b"], "2", 3, 4, 0)
    assert exp(("docs", "view", alice, 0, 0, 2)) == (LOOKUP_OK, ["c"], "", 3, 4, 0)
    assert exp(("docs", "view", alice, 0, 0, 3)) == (LOOKUP_OK, [], "", 3, 4, 0)
    assert exp(("docs", "view", alice, 0, 1, 2)) == (LOOKUP_OK, ["b"], "3", 3, 4, 0)
    assert exp(("grp", "member", alice, 0, 100, 0)) == (LOOKUP_OK, ["eng", "ops"], "", 2, 2, 0)
