"""keto_subjects_batch without a GPU: the entry points exist next to an unchanged ABI version, the ctypes
struct has the header's layout, the call refuses a snapshot without a device, and the oracle expectation
the GPU tests compare with (tests/subjects_util.py, yardstick (A)) agrees with an example worked out by
hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import keto_amd
from keto_amd import capi
from oracle.oracle_sql import RelationTuple, SQLStore, SubjectID, SubjectSet
from tests import subjects_util
from tests.engine_util import rows_from_tuples
from tests.subjects_util import SUBJECTS_NOT_FOUND, SUBJECTS_OK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["keto_subjects_batch", "keto_subjects_batch_ids", "keto_subjects_free", "keto_subjects_count",
                "keto_subjects_ids", "keto_subjects_offsets", "keto_subjects_status", "keto_subjects_next_page",
                "keto_subjects_totals", "keto_subjects_leaves", "keto_subjects_set_leaves", "keto_subjects_timing",
                "keto_subjects_stages"]


def test_header_declares_and_library_exports_the_subjects_calls():
    hdr = open(os.path.join(ROOT, "include", "keto_mi355x.h")).read()
    lib = keto_amd.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    # every keto_subjects_* function the header declares is one of them, and none took a lookup name
    assert set(re.findall(r"\b(keto_subjects_[a-z_]+)\(", hdr)) == set(ENTRY_POINTS)
    assert not [n for n in ENTRY_POINTS if re.match(r"keto_look(up|ed)_", n)]
    for macro, val in (("KETO_SUBJECTS_OK", 0), ("KETO_SUBJECTS_NOT_FOUND", 1), ("KETO_SUBJECTS_UNDECIDED", 2)):
        assert re.search(r"#define %s\s+%d\b" % (macro, val), hdr), macro
    assert (capi.SUBJECTS_OK, capi.SUBJECTS_NOT_FOUND, capi.SUBJECTS_UNDECIDED) == (0, 1, 2)
    for typ in ("keto_subjects_req", "keto_subjects"):
        assert re.search(r"\b%s;" % typ, hdr), typ
    # additive: the ABI version does not move
    assert int(re.search(r"#define KETO_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert lib.keto_abi_version() == 8 == capi.KETO_ABI_VERSION


def test_ctypes_struct_has_the_header_layout(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "keto_mi355x.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(keto_subjects_req), sizeof(keto_str),\n'
                   "           offsetof(keto_subjects_req, object), offsetof(keto_subjects_req, relation),\n"
                   "           offsetof(keto_subjects_req, max_depth), offsetof(keto_subjects_req, page_size),\n"
                   "           offsetof(keto_subjects_req, page));\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]
    R = capi.KSubjectsReq
    assert got == [C.sizeof(R), C.sizeof(capi.KStr), R.object.offset, R.relation.offset, R.max_depth.offset,
                   R.page_size.offset, R.page.offset]


def test_subjects_need_a_device():
    snap = keto_amd.Snapshot.build([(1, "n")], [(1, "a", "r", "u")], device=-1)
    with pytest.raises(keto_amd.KetoError) as e:
        snap.subjects([("n", "a", "r", 0, 0, 0)])
    assert e.value.code == -2                                             # KETO_E_HIP
    # n = 0 too: a host-only snapshot is KETO_E_HIP whatever n is
    with pytest.raises(keto_amd.KetoError) as e:
        snap.subjects_raw([])
    assert e.value.code == -2
    empty32 = np.zeros(0, dtype=np.uint32)
    with pytest.raises(keto_amd.KetoError) as e:
        snap.subjects_ids_raw(empty32, np.zeros(0, dtype=np.int32), empty32, empty32)
    assert e.value.code == -2
    with pytest.raises(keto_amd.KetoError) as e:
        snap.subjects_ids_raw(np.array([0x80000000], dtype=np.uint32), np.zeros(1, dtype=np.int32),
                              np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32))
    assert e.value.code == -2
    # NULL arguments are refused before anything else
    lib = keto_amd.load()
    one = (C.c_uint32 * 1)(0x80000000)
    out = C.c_void_p()
    assert lib.keto_subjects_batch(snap.h, None, C.c_uint32(1), C.c_int32(5), C.byref(out)) == -1
    assert lib.keto_subjects_batch(snap.h, None, C.c_uint32(1), C.c_int32(5), None) == -1
    assert lib.keto_subjects_batch(None, None, C.c_uint32(0), C.c_int32(5), C.byref(out)) == -1
    assert lib.keto_subjects_batch_ids(snap.h, one, None, one, one, C.c_uint32(1), C.c_int32(5), C.byref(out)) == -1
    assert lib.keto_subjects_batch_ids(snap.h, one, one, one, one, C.c_uint32(1), C.c_int32(5), None) == -1
    # accessors on NULL
    assert lib.keto_subjects_count(None) == 0 and lib.keto_subjects_ids(None, None) is None
    total = C.c_uint64(7)
    assert lib.keto_subjects_ids(None, C.byref(total)) is None and total.value == 0
    for f in (lib.keto_subjects_offsets, lib.keto_subjects_status, lib.keto_subjects_next_page, lib.keto_subjects_totals,
              lib.keto_subjects_leaves, lib.keto_subjects_set_leaves, lib.keto_subjects_stages):
        assert f(None) is None
    assert lib.keto_subjects_timing(None, None, None) == -1
    lib.keto_subjects_free(None)


def test_subjects_util_on_a_hand_written_example():
    """The six tuples of tests/test_lookup_cpu.py; who has `view` on which doc, by Expand?
         docs:a#view@alice
         docs:b#view@(grp:eng#member)
         grp:eng#member@alice
         docs:c#view@(grp:ops#member)         ops -> eng -> alice: three levels under the root
         grp:ops#member@(grp:eng#member)
         docs:d#view@bob
    docs:c#view at the global depth (5) reaches alice.  At request depth 2 the root's child grp:ops#member is
    built with one level left and becomes a leaf: no subject id, one subject-set leaf.  At depth 1 the root
    itself is that leaf.  The wildcard root docs:#view sees alice under a and under b's group, bob under d, and
    c's group ops, whose only child eng was visited under b: a nil child, kept as a subject-set leaf."""
    ns = [(1, "docs"), (2, "grp")]
    T = RelationTuple
    eng, ops = SubjectSet("grp", "eng", "member"), SubjectSet("grp", "ops", "member")
    tuples = [T("docs", "a", "view", SubjectID("alice")), T("docs", "b", "view", eng), T("grp", "eng", "member", SubjectID("alice")),
              T("docs", "c", "view", ops), T("grp", "ops", "member", eng), T("docs", "d", "view", SubjectID("bob"))]
    store = SQLStore(ns, tuples, page_size=2)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), page_size=2, device=-1)

    def exp(q, g=5):
        st, words, token, total, leaves, sets = subjects_util.expected_oracle(store, snap, q, g)
        return (st, [f[1] for f in snap.subject_fields(np.array(words, dtype=np.uint32))] if words else [], token, total,
                leaves, sets)

    assert exp(("docs", "c", "view", 0, 100, 0)) == (SUBJECTS_OK, ["alice"], "", 1, 1, 0)
    assert exp(("docs", "c", "view", 3, 100, 0)) == (SUBJECTS_OK, [], "", 0, 0, 1)      # eng is the leaf
    assert exp(("docs", "c", "view", 2, 100, 0)) == (SUBJECTS_OK, [], "", 0, 0, 1)      # ops is the leaf
    assert exp(("docs", "c", "view", 1, 100, 0)) == (SUBJECTS_OK, [], "", 0, 0, 1)      # the root is
    assert exp(("docs", "c", "view", 0, 100, 0), g=2) == (SUBJECTS_OK, [], "", 0, 0, 1)  # the global depth clamps
    assert exp(("docs", "c", "view", 9, 100, 0), g=2) == (SUBJECTS_OK, [], "", 0, 0, 1)  # > global -> global
    assert exp(("docs", "zz", "view", 0, 100, 0)) == (SUBJECTS_OK, [], "", 0, 0, 0)     # no tuples: nil
    assert exp(("nope", "c", "view", 0, 100, 0)) == (SUBJECTS_NOT_FOUND, [], "", 0, 0, 0)
    assert exp(("grp", "ops", "member", 0, 100, 0)) == (SUBJECTS_OK, ["alice"], "", 1, 1, 0)
    # pages: size 0 is the store's page size (2); the token is "" on the last page and past the end
    assert exp(("docs", "a", "view", 0, 0, 0)) == (SUBJECTS_OK, ["alice"], "", 1, 1, 0)
    assert exp(("docs", "a", "view", 0, 1, 1)) == (SUBJECTS_OK, ["alice"], "", 1, 1, 0)
    assert exp(("docs", "a", "view", 0, 1, 2)) == (SUBJECTS_OK, [], "", 1, 1, 0)
    wild = lambda size, page: exp(("docs", "", "view", 0, size, page))
    assert wild(100, 0) == (SUBJECTS_OK, ["alice", "bob"], "", 2, 3, 1)
    assert wild(0, 0) == (SUBJECTS_OK, ["alice", "bob"], "", 2, 3, 1)
    assert wild(1, 0) == (SUBJECTS_OK, ["alice"], "2", 2, 3, 1)
    assert wild(1, 2) == (SUBJECTS_OK, ["bob"], "", 2, 3, 1)
    assert wild(1, 3) == (SUBJECTS_OK, [], "", 2, 3, 1)
