"""keto_list_batch / keto_list_plan without a GPU: the entry points exist next to an unchanged ABI
version, the resolver's plans (host-only snapshots) agree with SQLite's counts for the namespace /
object / relation part of a query, and the scan refuses a snapshot without a device."""
import itertools
import os
import re

import pytest

import keto_amd
from keto_amd import capi
from tests import list_util
from tests.engine_util import rows_from_tuples
from tests.randgraph import random_store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["keto_list_batch", "keto_listed_free", "keto_listed_count", "keto_listed_tuples",
                "keto_listed_offsets", "keto_listed_status", "keto_listed_next_page", "keto_listed_totals",
                "keto_listed_timing", "keto_list_plan"]


def test_header_declares_and_library_exports_the_list_calls():
    hdr = open(os.path.join(ROOT, "include", "keto_mi355x.h")).read()
    lib = keto_amd.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    for macro, val in (("KETO_LIST_OK", 0), ("KETO_LIST_NOT_FOUND", 1), ("KETO_LIST_UNDECIDED", 2)):
        assert re.search(r"#define %s %d\b" % (macro, val), hdr), macro
    for typ in ("keto_list_req", "keto_list_tuple", "keto_listed", "keto_list_plan_t"):
        assert re.search(r"\b%s;" % typ, hdr), typ
    # additive: the ABI version does not move
    assert int(re.search(r"#define KETO_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert lib.keto_abi_version() == 8 == capi.KETO_ABI_VERSION


def _host_snapshot(seed):
    store, ns, tuples, raw, ps, alph = random_store(seed)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=-1)
    return store, snap, alph


@pytest.mark.parametrize("seed", range(40))
def test_list_plan_against_sqlite_counts(seed):
    store, snap, (names, objs, rels, users) = _host_snapshot(seed)
    keys = list(itertools.product(sorted(set(names) | {""}), objs + [""], rels + [""]))
    plans = snap.list_plan([(n, o, r, None, 0, 0) for n, o, r in keys])
    for (n, o, r), p in zip(keys, plans):
        assert p["status"] == list_util.LIST_OK
        count = list_util.count_key_part(store, n, o, r)
        assert p["hi"] - p["lo"] >= count, (n, o, r)
        if n != "" and o != "" and r != "":
            # one row: the range is exactly its tuples, nothing is left to compare
            assert p["hi"] - p["lo"] == count, (n, o, r)
            assert p["obj"] is None and p["rel"] is None
        if n != "" and o != "":
            assert p["obj"] is None                     # the range alone implies namespace and object
    # a subject never changes the range, only the word the scan compares
    sub_plans = snap.list_plan([(n, o, r, ("id", users[0]), 0, 0) for n, o, r in keys])
    for p, q in zip(plans, sub_plans):
        assert (q["lo"], q["hi"]) == (p["lo"], p["hi"]) or q["lo"] == q["hi"]

    # unknown namespaces: herodot.ErrNotFound, whatever else the query says
    name = next(n for n in names if n != "") if any(n != "" for n in names) else ""
    nf = snap.list_plan([("nope", "", "", None, 0, 0), ("nope", objs[0], rels[0], ("id", users[0]), 0, 0),
                         (name, "", "", ("set", "nope", objs[0], rels[0]), 0, 0),
                         ("", objs[0], "", ("set", "nope", "", ""), 0, 0)])
    assert [p["status"] for p in nf] == [list_util.LIST_NOT_FOUND] * 4
    # a field whose string the snapshot has never seen matches nothing
    unknown = snap.list_plan([(name, "zz-unknown", "", None, 0, 0), (name, "", "zz-unknown", None, 0, 0),
                              ("", "zz-unknown", rels[0], None, 0, 0), (name, objs[0], rels[0], ("id", "zz-unknown"), 0, 0),
                              (name, "", "", ("set", name, "zz-unknown", rels[0]), 0, 0)] if name != "" else
                             [("", "zz-unknown", "", None, 0, 0), ("", "", "zz-unknown", None, 0, 0)])
    for p in unknown:
        assert p["status"] == list_util.LIST_OK and p["lo"] == p["hi"]


def test_list_plan_subject_words():
    ns = [(1, "n"), (2, "m")]
    rows = [(1, "a", "r", "u"), (1, "a", "r", None, 2, "b", "s"), (2, "b", "s", "v"), (1, "c", "r", None, 1, "", "r")]
    snap = keto_amd.Snapshot.build(ns, rows, device=-1)
    plans = snap.list_plan([("", "", "", ("id", "u"), 0, 0), ("", "", "", ("set", "m", "b", "s"), 0, 0),
                            ("", "", "", ("set", "n", "", "r"), 0, 0), ("", "", "", ("set", "n", "x", "r"), 0, 0),
                            ("", "", "", ("set", "", "b", "s"), 0, 0)])
    # a subject id is its string id, a subject set its row (bit 31), a stored wildcard set its materialized row
    assert plans[0]["subject"] < 0x80000000 and snap.subject_fields([plans[0]["subject"]]) == [("id", "u")]
    assert snap.subject_fields([plans[1]["subject"]]) == [("set", "m", "b", "s")]
    assert snap.subject_fields([plans[2]["subject"]]) == [("set", "n", "", "r")]
    assert plans[3]["lo"] == plans[3]["hi"]                               # no stored subject set names it
    assert plans[4]["status"] == list_util.LIST_NOT_FOUND                 # no namespace is named ""
    assert all((p["lo"], p["hi"]) == (0, 4) for p in plans[:3])


def test_list_batch_needs_a_device():
    snap = keto_amd.Snapshot.build([(1, "n")], [(1, "a", "r", "u")], device=-1)
    with pytest.raises(keto_amd.KetoError) as e:
        snap.list_batch([("n", "", "", None, 0, 0)])
    assert e.value.code == -2                                             # KETO_E_HIP
    assert [p["hi"] - p["lo"] for p in snap.list_plan([("n", "", "", None, 0, 0)])] == [1]
