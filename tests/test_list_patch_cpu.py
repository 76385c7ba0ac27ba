"""The list index across writes, without a GPU: keto_list_index_info next to an unchanged ABI version,
and the host half (the rows in key order and their first entries) patched from the journal of written
rows on host-only snapshots -- random transactions and the edge ones against SQLite and against a
snapshot built afresh, the journal's row bound and KETO_LIST_PATCH=0 (subprocesses), refused writes."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import keto_amd
from keto_amd import capi
from oracle.oracle_sql import RelationTuple as T, SQLStore, SubjectID, SubjectSet
from tests import delete_util, list_patch_util as lp
from tests.engine_util import rows_from_tuples
from tests.randgraph import random_store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_call():
    hdr = open(os.path.join(ROOT, "include", "keto_mi355x.h")).read()
    lib = keto_amd.load()
    assert re.search(r"\bint keto_list_index_info\(const keto_snapshot\* s, keto_list_index_info_t\* out\);", hdr)
    assert hasattr(lib, "keto_list_index_info") and "keto_list_index_info" in capi.EXPORTS
    body = re.search(r"typedef struct \{([^}]*)\} keto_list_index_info_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(uint64_t|uint32_t|float)\s+([\w,\s]+);", body):
        fields += [(typ, n.strip()) for n in names.split(",")]
    assert fields == [("uint32_t", "host_built"), ("uint32_t", "host_current"), ("uint32_t", "dev_built"),
                      ("uint32_t", "dev_current"), ("uint64_t", "host_version"), ("uint64_t", "dev_version"),
                      ("uint64_t", "entries"), ("uint64_t", "device_bytes"), ("uint32_t", "journal_valid"),
                      ("uint32_t", "journal_rows"), ("uint64_t", "host_builds"), ("uint64_t", "host_patches"),
                      ("uint64_t", "dev_builds"), ("uint64_t", "dev_patches"), ("uint64_t", "last_segments"),
                      ("uint64_t", "last_staged_entries"), ("float", "last_host_ms"), ("float", "last_device_ms")]
    # the ctypes struct follows the header field by field: natural alignment gives the C offsets
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    assert [(n, t) for n, t in capi.KListIndexInfo._fields_] == [(n, ctype[t]) for t, n in fields]
    at = 0
    for typ, name in fields:
        size = ctypes.sizeof(ctype[typ])
        at = (at + size - 1) // size * size
        assert getattr(capi.KListIndexInfo, name).offset == at, name
        at += size
    assert capi.KListIndexInfo.host_version.offset == 16 and capi.KListIndexInfo.journal_valid.offset == 48
    assert capi.KListIndexInfo.last_device_ms.offset == 108 and ctypes.sizeof(capi.KListIndexInfo) == 112
    # additive: the ABI version does not move
    assert int(re.search(r"#define KETO_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert lib.keto_abi_version() == 8 == capi.KETO_ABI_VERSION


def test_a_snapshot_never_listed_reports_zeros():
    snap = keto_amd.Snapshot.build([(1, "n")], [(1, "a", "r", "u")], device=-1)
    snap.apply([(1, "b", "r", "u")], [])                          # no index state: nothing is recorded
    info = snap.list_index_info()
    assert set(info) == {n for n, _ in capi.KListIndexInfo._fields_} and not any(info.values()), info


@pytest.mark.parametrize("seed", range(40))
def test_host_half_parity(seed):
    store, ns, tuples, raw, ps, alph = random_store(seed, allow_poison=False)
    assert not raw
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), page_size=ps, device=-1)
    keys = delete_util.plan_keys(lp.wider(alph))
    lp.check_host(snap, store, ns, ps, keys)                       # builds the host half
    info = snap.list_index_info()
    assert (info["host_builds"], info["host_patches"], info["host_current"], info["journal_valid"]) == (1, 0, 1, 1)
    rng = lp.seeded(seed)
    for step in range(7):
        ins, dels = lp.random_transaction(rng, alph, store)
        assert lp.apply(snap, store, ns, ins, dels) == step + 1    # returned normally: nothing is refused
        stale = snap.list_index_info()
        assert (stale["host_current"], stale["journal_valid"], stale["host_version"]) == (0, 1, step)
        lp.check_host(snap, store, ns, ps, keys)
        info = snap.list_index_info()
        assert (info["host_patches"], info["host_builds"]) == (step + 1, 1), (seed, step, info)
        assert (info["host_current"], info["host_version"], info["journal_rows"]) == (1, step + 1, 0)
        assert snap.stats()["n_tuples"] == delete_util.n_tuples(store)


NS = [(1, "n"), (2, "m")]
BASE = [T("n", "b", "r", SubjectID("u")), T("n", "b", "r", SubjectID("v")), T("n", "d", "r", SubjectID("u")),
        T("n", "d", "s", SubjectID("w")), T("m", "g", "s", SubjectID("u")), T("n", "f", "r", SubjectSet("m", "g", "s"))]
KEYS = [(n, o, r) for n in ("n", "m") for o in ("", "0", "b", "c", "d", "f", "g", "zz") for r in ("", "r", "s")
        if o or not r]
# (what, inserts, deletes) in sequence on one snapshot
EDGE_WRITES = [
    ("a new row sorting before every row", [T("n", "0", "r", SubjectID("u"))], []),        # namespace id 1 sorts first
    ("a new row sorting after every row", [T("m", "zz", "s", SubjectID("u"))], []),
    ("a new row between two rows, its string before the build's", [T("n", "c", "0", SubjectID("0"))], []),
    ("a base row emptied", [], [T("n", "d", "r", SubjectID("u"))]),
    ("and refilled", [T("n", "d", "r", SubjectID("x")), T("n", "d", "r", SubjectID("x"))], []),
    ("a row added by a write is emptied by a later one", [], [T("n", "c", "0", SubjectID("0"))]),
    ("two adjacent rows changed in one write", [T("n", "b", "r", SubjectID("w")), T("n", "d", "r", SubjectID("a"))],
     [T("n", "b", "r", SubjectID("u"))]),
    ("a write that changes nothing", [T("n", "q", "r", SubjectID("tmp"))], [T("n", "q", "r", SubjectID("tmp"))]),
    ("a wildcard subject set: its materialized row is dirty, not a tuple row", [T("n", "f", "r", SubjectSet("n", "", "r"))],
     []),
    ("a row the wildcard row's query returns changes", [T("n", "zz", "r", SubjectID("u"))], [T("n", "0", "r", SubjectID("u"))]),
    ("everything of a namespace leaves", [], [T("m", "g", "s", SubjectID("u")), T("m", "zz", "s", SubjectID("u"))]),
]


def test_edge_transactions():
    store = SQLStore(NS, BASE, page_size=3)
    snap = keto_amd.Snapshot.build(NS, rows_from_tuples(NS, BASE), page_size=3, device=-1)
    lp.check_host(snap, store, NS, 3, KEYS)
    for k, (what, ins, dels) in enumerate(EDGE_WRITES):
        assert lp.apply(snap, store, NS, ins, dels) == k + 1, what
        assert snap.list_index_info()["journal_rows"] >= 1, what
        lp.check_host(snap, store, NS, 3, KEYS)
        info = snap.list_index_info()
        assert (info["host_patches"], info["host_builds"], info["host_current"]) == (k + 1, 1, 1), (what, info)
    # several writes between two plans collapse into one patch
    for ins in ([T("n", "b", "s", SubjectID("u"))], [T("n", "b", "s", SubjectID("v"))], [T("m", "a", "s", SubjectID("v"))]):
        lp.apply(snap, store, NS, ins, [])
    assert snap.list_index_info()["journal_rows"] == 2
    lp.check_host(snap, store, NS, 3, KEYS + [("m", "a", "s")])
    info = snap.list_index_info()
    assert (info["host_patches"], info["host_builds"]) == (len(EDGE_WRITES) + 1, 1)


def run_journal_rules(device=-1):
    """In a process with KETO_LIST_PATCH_MAX_ROWS=2 or KETO_LIST_PATCH=0 in its environment: returns
    (journal_valid after the write, host_builds, host_patches) after a 3-row write and the plan behind it."""
    store = SQLStore(NS, BASE, page_size=3)
    snap = keto_amd.Snapshot.build(NS, rows_from_tuples(NS, BASE), page_size=3, device=device)
    lp.check_host(snap, store, NS, 3, KEYS)
    lp.apply(snap, store, NS, [T("n", "b", "r", SubjectID("w"))], [T("n", "d", "s", SubjectID("w"))])      # 2 rows
    two = snap.list_index_info()["journal_valid"]
    lp.check_host(snap, store, NS, 3, KEYS)
    lp.apply(snap, store, NS, [T("n", "b", "r", SubjectID("x")), T("n", "c", "r", SubjectID("x")),
                               T("m", "g", "s", SubjectID("x"))], [])                                      # 3 rows
    info = snap.list_index_info()
    lp.check_host(snap, store, NS, 3, KEYS)                        # equal answers, patched or rebuilt
    after = snap.list_index_info()
    assert after["host_current"] == 1
    return two, info["journal_valid"], after["host_builds"], after["host_patches"]


def _in_subprocess(env, what):
    code = f"import tests.test_list_patch_cpu as t; print('{what}:', t.run_journal_rules())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_journal_row_bound():
    # two rows fit (a patch), three do not: the journal is invalid and the next plan rebuilds
    assert "bound: (1, 0, 2, 1)" in _in_subprocess({"KETO_LIST_PATCH_MAX_ROWS": "2"}, "bound")


def test_patching_disabled_never_patches():
    assert "off: (0, 0, 3, 0)" in _in_subprocess({"KETO_LIST_PATCH": "0"}, "off")


def test_journal_rules_with_the_defaults():
    assert "KETO_LIST_PATCH" not in os.environ and "KETO_LIST_PATCH_MAX_ROWS" not in os.environ
    assert run_journal_rules() == (1, 1, 1, 2)


def test_refused_writes_leave_the_journal_alone():
    from tests.test_delete_query_cpu import POISON_NS, POISON_RAW
    snap = keto_amd.Snapshot.build(POISON_NS, rows_from_tuples(POISON_NS, [], POISON_RAW), page_size=2, device=-1)
    plans = [("n", "", "", None, 0, 0), ("n", "b", "r", None, 0, 0)]
    before = snap.list_plan(plans)
    snap.apply([(1, "b", "r", "u3")], [])                          # noted: the host half is one version behind
    noted = snap.list_index_info()
    assert (noted["journal_rows"], noted["journal_valid"], noted["host_version"], noted["host_current"]) == (1, 1, 0, 0)
    for ins in ([(1, "a", "r", "u9")], [(1, "b", "r", "u4"), (1, "a", "r", "u9")]):
        with pytest.raises(keto_amd.KetoError) as e:               # n:a#r holds a poisoned tuple
            snap.apply(ins, [])
        assert e.value.code == delete_util.E_REBUILD
        assert snap.version() == 1 and snap.list_index_info() == noted
    with pytest.raises(keto_amd.KetoError) as e:
        snap.apply([(42, "b", "r", "u4")], [])                     # KETO_E_INVALID: an unknown namespace id
    assert e.value.code == delete_util.E_INVALID and snap.list_index_info() == noted
    after = snap.list_plan(plans)
    assert [p["hi"] - p["lo"] for p in after] == [p["hi"] - p["lo"] + 1 for p in before]
    info = snap.list_index_info()
    assert (info["host_patches"], info["host_builds"], info["host_version"], info["journal_rows"]) == (1, 1, 1, 0)
