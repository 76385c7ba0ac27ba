"""keto_snapshot_delete_query on the GPU against DeleteAllRelationTuples restated on SQLite
(tests/delete_util.py): random graphs (wildcard subject sets included) with the device list index
current (the device path, the index patched) and not (the host path), every listing, check and
expand after every delete; the kernels' tile / wave / pair edges (default tile and KETO_LIST_TILE=256);
poisoned tuples and the row cap on the device path; deletes interleaved with writes and lists; and two
shared-rows parts that take the same delete."""
import itertools
import os
import subprocess
import sys

import pytest

from oracle.oracle_sql import (CheckEngine, ExpandEngine, NotFoundError, RelationTuple, SQLStore, SubjectID,
                               SubjectSet)
from tests import delete_util, list_util
from tests.delete_util import PATH_DEVICE, PATH_HOST
from tests.engine_util import rows_from_tuples, subj
from tests.randgraph import random_store

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 5


def _listings(snap, store, queries):
    got = snap.list_batch([list_util.to_request(q) for q in queries])
    for q, g in zip(queries, got):
        assert g == list_util.expected(store, q), (q, g)


def _index_is_current(snap):
    """A list call that finds the device index current builds nothing."""
    return snap.list_batch_raw([("", "", "", None, 1, 0)])[5][0] == 0


def _gpu_sequence(seed, alph, tuples):
    """The CPU test's sequence thinned to a dozen deletes: the unknown-subject ones, then every third,
    and always the two empty queries at the end."""
    seq = delete_util.query_sequence(seed, alph, tuples)
    return seq[:2] + seq[12:-2:3] + seq[-2:]


@pytest.mark.parametrize("indexed", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("seed", range(40))
def test_random_parity(seed, indexed):
    import keto_amd
    from tests.test_gpu_list import _all_pages
    store, ns, tuples, raw, ps, alph = random_store(seed, allow_poison=False)
    names, objs, rels, users = alph
    assert not raw and len(tuples) <= 40
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), page_size=ps, device=0)
    keys = list(itertools.product(sorted(set(names) | {""}), objs[:2] + [""], rels[:2] + [""]))
    stored = sorted({t.subject for t in tuples if isinstance(t.subject, SubjectSet)}, key=lambda s: s.string())
    list_subjects = [None, SubjectID(users[0])] + stored[:1]
    pages = lambda: _all_pages(store, keys, list_subjects, sizes=(0,))     # every page of every filtered listing
    # every (row, subject) pair of the graph; rows of a namespace named "" and subject sets with an
    # empty field are left to the traversal below them
    rows = sorted({(t.namespace, t.object, t.relation) for t in tuples if t.namespace})
    subjects = sorted({subj(t.subject) for t in tuples if isinstance(t.subject, SubjectID) or
                       (t.subject.namespace and t.subject.object and t.subject.relation)})
    pairs = [RelationTuple(n, o, r, SubjectID(s[1]) if s[0] == "id" else SubjectSet(*s[1:])) for (n, o, r), s in
             itertools.product(rows, subjects)]
    roots = [s for s in stored if s.namespace and s.object and s.relation]
    # a write that changes no tuple (an insert and its delete in one transaction): the list index of
    # the version before it is not current any more
    tmp = rows_from_tuples(ns, [RelationTuple(names[0], "zz-tmp", rels[0], SubjectID("zz-tmp"))])
    version = 0
    for q in _gpu_sequence(seed, alph, tuples):
        if indexed:
            snap.list_batch([("", "", "", None, 1, 0)])                 # the index is current before the delete
        else:
            snap.apply(tmp, tmp)
            version += 1
        # a range the resolver finds empty needs no scan, and a fully keyed one is the host's
        plan = snap.list_plan([delete_util.request(q) + (0, 0)])[0]
        on_host = plan["lo"] == plan["hi"] or (q[0] != "" and q[1] != "" and q[2] != "")
        want_deleted, want_rows = delete_util.sql_delete(store, *q)
        info = snap.delete_query(*delete_util.request(q))
        version += 1
        assert (info["deleted"], info["rows_touched"], info["version"]) == (want_deleted, want_rows, version), (q, info)
        if indexed:
            assert info["path"] == (PATH_HOST if on_host else PATH_DEVICE) and info["index_kept"] == 1, (q, info)
            assert _index_is_current(snap), q
        else:
            assert info["path"] == PATH_HOST and info["index_kept"] == 0, (q, info)
        assert snap.stats()["n_tuples"] == delete_util.n_tuples(store)
        _listings(snap, store, [("", "", "", None, 1000, 1)] + pages())
        if pairs:
            allowed, _ = snap.check_batch([(t.namespace, t.object, t.relation, subj(t.subject), 0) for t in pairs], G)
            eng = CheckEngine(store, G)
            for t, a in zip(pairs, allowed):
                assert bool(a) == eng.subject_is_allowed(t, 0), (seed, q, t)
        if roots:
            got = snap.expand_batch([(subj(s), 3) for s in roots], G)
            for s, (st, js) in zip(roots, got):
                try:
                    tr = ExpandEngine(store, G).build_tree(s, 3)
                    want = ("tree", tr.to_json()) if tr is not None else ("nil", None)
                except NotFoundError:
                    want = ("error", None)
                assert ({0: "tree", 1: "nil", 2: "error"}[st], js) == want, (seed, q, s)
    assert delete_util.n_tuples(store) == 0
    snap.close()


# ---------------------------------------------------------------------------------- kernel edges
def run_edges():
    """Deletes on the graph of tests/test_gpu_list.py::_edge_graph -- 5,000 rows, every third also
    holding `u`, and one row of 3 * 4096 + 5 more entries -- with whatever KETO_LIST_TILE the process
    has.  Every delete runs on the device (none names all three key fields) with the index current."""
    import keto_amd
    from tests.test_gpu_list import BIG, _edge_graph
    ns, raw = _edge_graph()
    store = SQLStore(ns, raw_rows=raw)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, [], raw), device=0)
    everything = [("n", "", "", None, 10 ** 6, 1)]
    _listings(snap, store, everything)
    n_u = len(range(0, 5000, 3))

    def plan(q):
        return snap.list_plan([(q[0], q[1], q[2], None, 0, 0)])[0]

    def delete(q, deleted, rows):
        before = snap.stats()["device_bytes"]
        want = delete_util.sql_delete(store, *q)
        assert want == (deleted, rows), (q, want)
        info = snap.delete_query(*delete_util.request(q))
        assert (info["deleted"], info["rows_touched"], info["path"], info["index_kept"]) == (deleted, rows, PATH_DEVICE, 1), \
            (q, info)
        # 8 B less per deleted tuple, up to the padding of T to an even entry count
        assert abs((before - snap.stats()["device_bytes"]) - 8 * deleted) <= 8, q
        assert _index_is_current(snap), q
        _listings(snap, store, everything)

    # key predicates through keys[]: no namespace, so object / relation are compared per entry
    delete(("", "", "r", SubjectID("x5")), 1, 1)
    delete(("", "o0007", "", SubjectID("x7")), 1, 1)
    # one subject inside the big row
    delete(("n", "o2500", "", SubjectID("b00007")), 1, 1)
    # a range whose first and last entries are odd ones: o0002's single entry is entry 3, behind
    # o0000's two and o0001's one
    p = plan(("n", "o0002", ""))
    assert p["lo"] % 2 == 1 and (p["hi"] - 1) % 2 == 1, p
    delete(("n", "o0002", "", None), 1, 1)
    # a one-entry range at an even entry: o0001 holds x1 alone
    p = plan(("n", "o0001", ""))
    assert p["hi"] - p["lo"] == 1 and p["lo"] % 2 == 0, p
    delete(("n", "o0001", "", None), 1, 1)
    # the first match is lo itself (`u` sorts before `x0` in the namespace's first row); 1,667 heads
    # spread over every tile
    first = snap.list_batch([("n", "", "", None, 1, 1)])[0][1]
    assert first == [("n", "o0000", "r", ("id", "u"))]
    delete(("n", "", "", SubjectID("u")), n_u, n_u)
    # the big row: one head whose run crosses wave-quarter, 128-entry-step and tile boundaries
    p = plan(("n", "o2500", ""))
    assert p["hi"] - p["lo"] == BIG + 1 - 1                     # x2500 and the b's, less b00007
    delete(("n", "o2500", "", None), BIG, 1)
    # what is left, from an odd or even start alike: a whole-namespace delete with nothing kept
    left = delete_util.n_tuples(store)
    delete(("n", "", "", None), left, left)
    assert snap.stats()["n_tuples"] == 0
    return 8


def test_kernel_edges():
    assert "KETO_LIST_TILE" not in os.environ
    assert run_edges() == 8


def test_kernel_edges_tile_256():
    env = dict(os.environ, KETO_LIST_TILE="256")
    code = "import tests.test_gpu_delete_query as t; print('delete edges ok:', t.run_edges())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "delete edges ok: 8" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------- poison, cap
def test_poisoned_tuples_on_the_device_path():
    import keto_amd
    from tests.test_delete_query_cpu import POISON_NS, POISON_RAW, poison_cases
    store = SQLStore(POISON_NS, raw_rows=POISON_RAW, page_size=2)
    snap = keto_amd.Snapshot.build(POISON_NS, rows_from_tuples(POISON_NS, [], POISON_RAW), page_size=2, device=0)
    snap.list_batch([("n", "d", "r", None, 0, 0)])
    assert poison_cases(snap, store) == 12
    assert _index_is_current(snap)                  # refused deletes left it alone, the others patched it
    _listings(snap, store, [("n", "b", "", None, 0, 1), ("n", "d", "", None, 0, 1), ("n", "a", "r", None, 1, 2)])


def test_row_cap_on_the_device_path():
    env = dict(os.environ, KETO_DELETE_QUERY_MAX_ROWS="3")
    code = "import tests.test_delete_query_cpu as t; print('cap ok:', t.run_cap(0))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cap ok: 3" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------- interleaving
def test_deletes_interleaved_with_writes_and_lists():
    import keto_amd
    ns = [(1, "n"), (2, "m")]
    T = RelationTuple
    tuples = [T("n", "a", "r", SubjectID("u")), T("n", "a", "r", SubjectID("v")), T("n", "b", "r", SubjectSet("m", "g", "s")),
              T("m", "g", "s", SubjectID("u")), T("n", "c", "t", SubjectID("w")), T("n", "a", "r", SubjectID("u")),
              T("n", "d", "r", SubjectSet("m", "", "s"))]
    store = SQLStore(ns, tuples, page_size=3)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), page_size=3, device=0)
    keys = list(itertools.product(["n", "m", ""], ["a", "b", "g", "aa", ""], ["r", "s", ""]))
    subjects = [None, SubjectID("u"), SubjectSet("m", "g", "s"), SubjectSet("n", "aa", "r")]
    queries = lambda: [(n, o, r, s, 2, p) for (n, o, r), s in itertools.product(keys, subjects) for p in (1, 2, 3)]
    _listings(snap, store, queries())
    old = snap.list_batch_raw([("", "", "", None, 100, 0)])
    old_dec = snap.decode_list_tuples(old[2])
    assert len(old_dec) == len(tuples)

    def apply(ins, dels):
        snap.apply([rows_from_tuples(ns, [t])[0] for t in ins], [rows_from_tuples(ns, [t])[0] for t in dels])
        for t in ins:
            store.insert(t)
        for t in dels:
            store.delete(t)

    def delete(q, path):
        want = delete_util.sql_delete(store, *q)
        info = snap.delete_query(*delete_util.request(q))
        assert (info["deleted"], info["rows_touched"], info["path"]) == want + (path,), (q, info)
        return info

    # a write: new rows, a new string, a new subject set whose target row is new; the index goes stale
    apply([T("n", "aa", "r", SubjectID("zed")), T("m", "g", "s", SubjectSet("n", "aa", "r")), T("n", "0", "r", SubjectID("u"))],
          [T("n", "c", "t", SubjectID("w"))])
    v = snap.version()
    info = delete(("", "", "", SubjectID("u")), PATH_HOST)            # stale index: the host finds the rows
    assert info["deleted"] == 4 and info["index_kept"] == 0 and info["version"] == v + 1
    _listings(snap, store, queries())                                 # rebuilds the index
    info = delete(("n", "", "r", None), PATH_DEVICE)                  # a, aa, b, d -- also rows a write added
    assert info["index_kept"] == 1 and _index_is_current(snap)
    _listings(snap, store, queries())
    # a row the delete emptied takes tuples again, the wildcard set's row is re-materialized
    apply([T("n", "a", "r", SubjectID("u")), T("m", "g2", "s", SubjectID("q")), T("n", "d", "r", SubjectSet("m", "", "s"))], [])
    _listings(snap, store, queries() + [("m", "g2", "", None, 0, 1)])
    allowed, _ = snap.check_batch([("n", "d", "r", ("id", "q"), 0), ("n", "d", "r", ("id", "u"), 0),
                                   ("n", "a", "r", ("id", "u"), 0)], G)
    eng = CheckEngine(store, G)
    want = [eng.subject_is_allowed(T("n", "d", "r", SubjectID(s)), 0) for s in ("q", "u")] + [True]
    assert [bool(a) for a in allowed] == want
    info = delete(("m", "", "", None), PATH_DEVICE)
    assert info["index_kept"] == 1
    _listings(snap, store, queries())
    allowed, _ = snap.check_batch([("n", "d", "r", ("id", "q"), 0)], G)
    assert not allowed[0] and not eng.subject_is_allowed(T("n", "d", "r", SubjectID("q")), 0)
    # row ids and string ids are only appended: the result taken before all of it decodes as before
    assert snap.decode_list_tuples(old[2]) == old_dec


# ---------------------------------------------------------------------------------- parts
def test_shared_parts_take_the_same_delete():
    import keto_amd
    from keto_amd.capi import PART_SHARED
    from tests.randgraph import random_checks
    from tests.test_gpu_comm import _local_comms, _ok, _ranks
    P = 2
    os.environ.setdefault("KETO_COMM_TIMEOUT_MS", "60000")
    for seed in (4200, 4203, 4206):
        store, ns, tuples, raw, ps, alph = random_store(seed, allow_poison=False, n_tuples=40)
        names, objs, rels, users = alph
        names = [n for n in names if n]
        if not names:
            continue
        rows = rows_from_tuples(ns, tuples)
        whole = keto_amd.Snapshot.build(ns, rows, page_size=ps, device=0)
        parts = [keto_amd.Snapshot.build(ns, rows, page_size=ps, device=-1).upload_part(r, P, 0, mode=PART_SHARED)
                 for r in range(P)]
        comms = _local_comms(P)
        deletes = [(names[0], objs[0], "", None), ("", "", "", SubjectID(users[0])), ("", "", rels[0], None)]
        for step, q in enumerate(deletes):
            want = delete_util.sql_delete(store, *q)
            infos = [s.delete_query(*delete_util.request(q)) for s in [whole] + parts]
            for info in infos:
                assert (info["deleted"], info["rows_touched"], info["version"]) == want + (step + 1,), (q, info)
            assert all(info["path"] == PATH_HOST for info in infos[1:])           # a part scans on the host
            checks = random_checks(seed * 41 + step, (names, objs, rels, users), k=60)
            reqs = [(t.namespace, t.object, t.relation, subj(t.subject), d) for t, d, _ in checks]
            replicated, _ = whole.check_batch(reqs, G)
            mine = [list(range(r, len(reqs), P)) for r in range(P)]
            res = _ok(_ranks(P, lambda r: comms[r].check_batch_routed(parts[r], [reqs[i] for i in mine[r]], G)))
            for r, (got, _) in enumerate(res):
                for k, i in enumerate(mine[r]):
                    t, d, _ = checks[i]
                    assert bool(got[k]) == bool(replicated[i]) == CheckEngine(store, G).subject_is_allowed(t, d), (seed, q, t)
        for c in comms:
            c.close()
        for s in parts + [whole]:
            s.close()
