"""keto_snapshot_delete_query without a GPU (host-only snapshots, the host path) against
DeleteAllRelationTuples restated on SQLite (tests/delete_util.py): the entry point next to an unchanged
ABI version, random graphs under sequences of deletes over every filter shape, unknown namespaces,
poisoned tuples and the row cap."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import keto_amd
from keto_amd import capi
from oracle.oracle_sql import NotFoundError, SQLStore, SubjectID, SubjectSet
from tests import delete_util, list_util
from tests.delete_util import E_INVALID, E_REBUILD, PATH_HOST
from tests.engine_util import rows_from_tuples
from tests.randgraph import random_store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_call():
    hdr = open(os.path.join(ROOT, "include", "keto_mi355x.h")).read()
    lib = keto_amd.load()
    assert re.search(r"\bketo_snapshot_delete_query\(keto_snapshot\* s, const keto_list_req\* query, keto_delete_info\* out",
                     hdr)
    assert hasattr(lib, "keto_snapshot_delete_query") and "keto_snapshot_delete_query" in capi.EXPORTS
    assert re.search(r"#define KETO_DELETE_PATH_HOST 0\b", hdr) and re.search(r"#define KETO_DELETE_PATH_DEVICE 1\b", hdr)
    # the struct as the header lays it out: 3 x u64, 2 x u32, 2 x float
    body = re.search(r"typedef struct \{([^}]*)\} keto_delete_info;", hdr).group(1)
    fields = re.findall(r"(uint64_t|uint32_t|float)\s+(\w+);", body)
    assert fields == [("uint64_t", "deleted"), ("uint64_t", "rows_touched"), ("uint64_t", "version"), ("uint32_t", "path"),
                      ("uint32_t", "index_kept"), ("float", "scan_ms"), ("float", "apply_ms")]
    assert [f[0] for f in capi.KDeleteInfo._fields_] == [n for _, n in fields]
    assert ctypes.sizeof(capi.KDeleteInfo) == 40 and capi.KDeleteInfo.path.offset == 24
    assert capi.KDeleteInfo.apply_ms.offset == 36
    # additive: the ABI version does not move
    assert int(re.search(r"#define KETO_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert lib.keto_abi_version() == 8 == capi.KETO_ABI_VERSION


@pytest.mark.parametrize("seed", range(40))
def test_random_deletes_against_sqlite(seed):
    store, ns, tuples, raw, ps, alph = random_store(seed, allow_poison=False)
    assert not raw and len(tuples) <= 40
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), page_size=ps, device=-1)
    keys = delete_util.plan_keys(alph)
    version, some = 0, 0
    for q in delete_util.query_sequence(seed, alph, tuples):
        want_deleted, want_rows = delete_util.sql_delete(store, *q)
        info = snap.delete_query(*delete_util.request(q))
        version += 1
        assert (info["deleted"], info["rows_touched"], info["version"]) == (want_deleted, want_rows, version), (q, info)
        assert info["path"] == PATH_HOST and info["index_kept"] == 0
        assert snap.version() == version
        assert snap.stats()["n_tuples"] == delete_util.n_tuples(store), q
        delete_util.check_plans(snap, store, keys)
        some += want_deleted > 0
    assert delete_util.n_tuples(store) == 0 and snap.stats()["n_tuples"] == 0
    assert some or not tuples


def test_fully_keyed_query_and_duplicates():
    ns = [(1, "n"), (2, "m")]
    rows = [(1, "a", "r", "u"), (1, "a", "r", "u"), (1, "a", "r", "v"), (1, "a", "r", None, 2, "g", "s"),
            (1, "a", "r", None, 2, "g", "s"), (2, "g", "s", "u"), (1, "b", "r", "u"), (1, "c", "r", None, 2, "", "s")]
    snap = keto_amd.Snapshot.build(ns, rows, device=-1)
    info = snap.delete_query("n", "a", "r", ("id", "u"))                 # every equal tuple
    assert (info["deleted"], info["rows_touched"], info["path"], info["version"]) == (2, 1, PATH_HOST, 1)
    info = snap.delete_query("n", "a", "r", ("set", "m", "g", "s"))
    assert (info["deleted"], info["rows_touched"], info["version"]) == (2, 1, 2)
    # a stored subject set with an empty field is a tuple, matched by its subject word; its materialized
    # row is a view and is never matched itself
    info = snap.delete_query("", "", "", ("set", "m", "", "s"))
    assert (info["deleted"], info["rows_touched"]) == (1, 1)
    info = snap.delete_query("m", "", "s")
    assert (info["deleted"], info["rows_touched"]) == (1, 1)
    assert snap.stats()["n_tuples"] == 2
    info = snap.delete_query()
    assert (info["deleted"], info["rows_touched"], info["version"]) == (2, 2, 5)
    assert snap.delete_query()["deleted"] == 0 and snap.version() == 6


def _unchanged(snap, before):
    assert (snap.version(), snap.stats(), snap.list_plan(PLAN_QUERIES)) == before


PLAN_QUERIES = [("", "", "", None, 0, 0), ("n", "", "", None, 0, 0), ("n", "a", "", None, 0, 0), ("n", "a", "r", None, 0, 0),
                ("n", "b", "r", ("id", "u1"), 0, 0)]


def _state(snap):
    return snap.version(), snap.stats(), snap.list_plan(PLAN_QUERIES)


def test_unknown_namespace_is_invalid_and_changes_nothing():
    ns = [(1, "n")]
    rows = [(1, "a", "r", "u1"), (1, "b", "r", "u1"), (1, "b", "r", None, 1, "a", "r")]
    store = SQLStore(ns, raw_rows=[r + (None, None, None) if len(r) == 4 else r for r in rows])
    snap = keto_amd.Snapshot.build(ns, rows, device=-1)
    before = _state(snap)
    for q in (("nope", "", "", None), ("nope", "a", "r", SubjectID("u1")), ("n", "", "", SubjectSet("nope", "a", "r")),
              ("", "a", "", SubjectSet("", "a", "r"))):
        with pytest.raises(NotFoundError):
            delete_util.sql_delete(store, *q)
        with pytest.raises(keto_amd.KetoError) as e:
            snap.delete_query(*delete_util.request(q))
        assert e.value.code == E_INVALID, q
        name = q[0] if q[0] == "nope" else q[3].namespace
        assert f"Unknown namespace with name {name}." in str(e.value)
        _unchanged(snap, before)
    assert snap.delete_query("n", "b", "r", ("id", "u1"))["deleted"] == 1


POISON_NS = [(1, "n")]
POISON_RAW = [(1, "a", "r", "u1", None, None, None), (1, "a", "r", "u2", None, None, None),
              (1, "a", "r", None, 99, "x", "y"),          # a subject set of namespace id 99
              (1, "b", "r", "u1", None, None, None), (1, "b", "r", "u2", None, None, None),
              (1, "d", "r", "u1", None, None, None),
              (7, "c", "r", "u1", None, None, None)]      # a tuple whose own namespace id is not configured
U1, U2 = SubjectID("u1"), SubjectID("u2")
# a matched tuple is a poisoned one, or -- with a subject -- a poisoned tuple lies among the tuples
# matching the namespace / object / relation part (the list call's UNDECIDED cases)
POISON_REBUILD = [("n", "a", "r", None), ("n", "a", "", None), ("n", "", "", None), ("", "c", "", None), ("", "", "", None),
                  ("", "", "r", None), ("n", "a", "r", U1), ("n", "a", "", U1), ("n", "", "", U1), ("", "c", "", U1),
                  ("", "", "r", U1), ("", "", "", U2)]
POISON_OK = [(("n", "b", "r", U1), 1), (("n", "b", "", U2), 1), (("", "d", "", U1), 1), (("", "b", "r", U1), 0),
             (("n", "d", "r", None), 0), (("", "b", "", None), 0)]


def poison_cases(snap, store):
    """The graph of tests/test_gpu_list.py::test_poisoned_tuples; returns the number of refused deletes."""
    for q in POISON_REBUILD:
        before = _state(snap)
        with pytest.raises(keto_amd.KetoError) as e:
            snap.delete_query(*delete_util.request(q))
        assert e.value.code == E_REBUILD, q
        _unchanged(snap, before)
    for q, want in POISON_OK:
        deleted, rows = delete_util.sql_delete(store, *q)
        info = snap.delete_query(*delete_util.request(q))
        assert (info["deleted"], info["rows_touched"]) == (deleted, rows) and deleted == want, (q, info)
    assert snap.stats()["n_tuples"] == delete_util.n_tuples(store) == 4
    return len(POISON_REBUILD)


def test_poisoned_tuples():
    store = SQLStore(POISON_NS, raw_rows=POISON_RAW, page_size=2)
    snap = keto_amd.Snapshot.build(POISON_NS, rows_from_tuples(POISON_NS, [], POISON_RAW), page_size=2, device=-1)
    assert poison_cases(snap, store) == 12


def run_cap(device):
    """With KETO_DELETE_QUERY_MAX_ROWS=3 in the environment: four touched rows are refused, three pass."""
    ns = [(1, "n")]
    rows = [(1, f"o{i}", "r", "u") for i in range(4)] + [(1, f"o{i}", "r", "v") for i in range(3)]
    snap = keto_amd.Snapshot.build(ns, rows, device=device)
    if device >= 0:
        snap.list_batch([("n", "", "", None, 0, 0)])
    before = _state(snap)
    try:
        snap.delete_query("", "", "", ("id", "u"))
        raise AssertionError("four rows passed a cap of three")
    except keto_amd.KetoError as e:
        assert e.code == E_REBUILD, e
    _unchanged(snap, before)
    if device >= 0:
        assert snap.list_batch_raw([("n", "", "", None, 0, 0)])[5][0] == 0      # the index is still current
    info = snap.delete_query("n", "", "", ("id", "v"))
    assert (info["deleted"], info["rows_touched"], info["version"]) == (3, 3, 1)
    assert info["path"] == (delete_util.PATH_DEVICE if device >= 0 else PATH_HOST)
    return info["rows_touched"]


def test_row_cap():
    env = dict(os.environ, KETO_DELETE_QUERY_MAX_ROWS="3")
    code = "import tests.test_delete_query_cpu as t; print('cap ok:', t.run_cap(-1))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cap ok: 3" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
