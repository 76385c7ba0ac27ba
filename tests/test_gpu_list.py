"""keto_list_batch on the GPU against Persister.GetRelationTuples restated on SQLite (tests/list_util.py):
the reference's own manager test as golden data, random graphs with every filter combination and
every page, poisoned tuples, tile / wave / page-window edges (default tile and KETO_LIST_TILE=256),
lists after writes, batch independence and the error paths."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.oracle_sql import NotFoundError, RelationTuple, SQLStore, SubjectID, SubjectSet
from tests import list_util
from tests.engine_util import rows_from_tuples
from tests.list_util import LIST_NOT_FOUND, LIST_OK, LIST_UNDECIDED
from tests.randgraph import random_store

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compare(snap, store, queries, allow=(LIST_OK, LIST_NOT_FOUND)):
    """One list_batch call for `queries` (list_util form); every answer equals SQLite's."""
    got = snap.list_batch([list_util.to_request(q) for q in queries])
    assert len(got) == len(queries)
    for q, g in zip(queries, got):
        want = list_util.expected(store, q)
        assert g[0] in allow, (q, g[0])
        assert g == want, (q, g, want)
    return got


# ---------------------------------------------------------------------------------- golden
def _golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "list_cases.json")))


def _golden_store(group):
    ns = [(0, group["namespace"])]
    tuples = [RelationTuple(t["namespace"], t["object"], t["relation"], SubjectID(t["subject_id"]))
              for t in group["tuples"]]
    return ns, tuples, SQLStore(ns, tuples)


def _golden_query(q, size=0, page=0):
    sub = SubjectID(q["subject_id"]) if "subject_id" in q else None
    return (q.get("namespace", ""), q.get("object", ""), q.get("relation", ""), sub, size, page)


def test_golden_queries():
    import keto_amd
    g = _golden()["queries"]
    ns, tuples, store = _golden_store(g)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), device=0)
    queries = [_golden_query(c["query"]) for c in g["cases"]]
    got = _compare(snap, store, queries, allow=(LIST_OK,))
    for c, (status, tup, token, total) in zip(g["cases"], got):
        want = sorted(list_util.tuple_key(tuples[i]) for i in c["expected"])
        assert sorted(tup) == want and token == c["next_page"] and total == len(want)


def test_golden_pagination_walk():
    import keto_amd
    g = _golden()["pagination"]
    ns, tuples, store = _golden_store(g)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), device=0)
    left = [list_util.tuple_key(t) for t in tuples]
    token, non_empty = "", 0
    for _ in range(g["pages"]):
        q = _golden_query(g["query"], size=g["page_size"], page=int(token or 0))
        (status, tup, token, total), = _compare(snap, store, [q], allow=(LIST_OK,))
        assert len(tup) == g["tuples_per_page"] and total == len(tuples)
        left.remove(tup[0])
        non_empty += token != ""
    assert non_empty == g["non_empty_tokens"] and token == g["last_token"] and left == []


def test_golden_empty_list():
    import keto_amd
    g = _golden()["empty_list"]
    ns, tuples, store = _golden_store(g)
    snap = keto_amd.Snapshot.build(ns, [], device=0)
    (status, tup, token, total), = _compare(snap, store, [_golden_query(g["query"])], allow=(LIST_OK,))
    assert (status, tup, token, total) == (LIST_OK, g["expected"], g["next_page"], 0)


# ---------------------------------------------------------------------------------- random parity
def _all_pages(store, keys, subjects, sizes=(0, 1, 3)):
    out = []
    for (n, o, r), sub, size in itertools.product(keys, subjects, sizes):
        try:
            last = list_util.last_page(store, n, o, r, sub, size)
        except NotFoundError:
            last = 0
        out += [(n, o, r, sub, size, page) for page in range(1, last + 2)]
    return out


@pytest.mark.parametrize("seed", range(60))
def test_random_parity(seed):
    import keto_amd
    # unfiltered queries: poisoned tuples allowed, the answer is always exact
    store, ns, tuples, raw, ps, (names, objs, rels, users) = random_store(seed)
    assert len(tuples) <= 40
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=0)
    keys = list(itertools.product(sorted(set(names) | {"", "nope"}), objs[:2] + [""], rels[:2] + [""]))
    _compare(snap, store, _all_pages(store, keys, [None]))
    snap.close()
    # subject-filtered queries: no poisoned tuple, and then never undecided
    store, ns, tuples, raw, ps, (names, objs, rels, users) = random_store(seed, allow_poison=False)
    assert not raw and len(tuples) <= 40
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), page_size=ps, device=0)
    stored = [t.subject for t in tuples if isinstance(t.subject, SubjectSet)]
    subjects = [SubjectID(u) for u in (users * 2)[:2]] + stored[:1] + [SubjectSet("nope", objs[0], rels[0])]
    keys = list(itertools.product(sorted(set(names) | {"", "nope"}), objs[:2] + [""], rels[:2] + [""]))
    _compare(snap, store, _all_pages(store, keys, subjects))


# ---------------------------------------------------------------------------------- poison
def test_poisoned_tuples():
    import keto_amd
    ns = [(1, "n")]
    raw = [(1, "a", "r", "u1", None, None, None), (1, "a", "r", "u2", None, None, None),
           (1, "a", "r", None, 99, "x", "y"),            # a subject set of namespace id 99: sorts first in n:a#r
           (1, "b", "r", "u1", None, None, None), (1, "b", "r", "u2", None, None, None),
           (1, "d", "r", "u1", None, None, None),
           (7, "c", "r", "u1", None, None, None)]        # a tuple whose own namespace id is not configured
    store = SQLStore(ns, raw_rows=raw, page_size=2)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, [], raw), page_size=2, device=0)
    u1 = SubjectID("u1")
    fixed = [
        # unfiltered: NOT_FOUND iff the page holds the poisoned tuple
        (("n", "a", "r", None, 1, 1), (LIST_NOT_FOUND, [], "", 0)),
        (("n", "a", "r", None, 1, 2), (LIST_OK, [("n", "a", "r", ("id", "u1"))], "3", 3)),
        (("n", "a", "r", None, 1, 3), (LIST_OK, [("n", "a", "r", ("id", "u2"))], "", 3)),
        (("n", "", "", None, 0, 1), (LIST_NOT_FOUND, [], "", 0)),
        (("n", "", "", None, 0, 2), (LIST_OK, [("n", "a", "r", ("id", "u2")), ("n", "b", "r", ("id", "u1"))], "3", 6)),
        (("", "c", "", None, 0, 1), (LIST_NOT_FOUND, [], "", 0)),
        (("", "", "", None, 6, 1), (LIST_NOT_FOUND, [], "", 0)),
        (("", "", "", None, 6, 2), (LIST_NOT_FOUND, [], "", 0)),       # the page is the tuple of namespace id 7
        (("", "", "", None, 5, 1), (LIST_NOT_FOUND, [], "", 0)),
        (("", "d", "", None, 0, 1), (LIST_OK, [("n", "d", "r", ("id", "u1"))], "", 1)),
        # filtered: UNDECIDED iff a poisoned tuple matches the namespace / object / relation part
        (("n", "a", "r", u1, 0, 1), (LIST_UNDECIDED, [], "", 0)),
        (("n", "a", "", u1, 0, 1), (LIST_UNDECIDED, [], "", 0)),
        (("n", "", "", u1, 0, 1), (LIST_UNDECIDED, [], "", 0)),
        (("n", "b", "r", u1, 0, 1), (LIST_OK, [("n", "b", "r", ("id", "u1"))], "", 1)),
        (("n", "b", "", SubjectID("u2"), 0, 1), (LIST_OK, [("n", "b", "r", ("id", "u2"))], "", 1)),
        # the row of the unconfigured namespace keeps its object and relation: only queries matching them
        (("", "c", "", u1, 0, 1), (LIST_UNDECIDED, [], "", 0)),
        (("", "", "r", u1, 0, 1), (LIST_UNDECIDED, [], "", 0)),
        (("", "d", "", u1, 0, 1), (LIST_OK, [("n", "d", "r", ("id", "u1"))], "", 1)),
        (("", "b", "r", u1, 1, 1), (LIST_OK, [("n", "b", "r", ("id", "u1"))], "", 1)),
    ]
    got = snap.list_batch([list_util.to_request(q) for q, _ in fixed])
    for (q, want), g in zip(fixed, got):
        assert g == want, (q, g, want)
        if q[3] is None or want[0] == LIST_OK:      # SQLite agrees wherever the snapshot answers
            assert g == list_util.expected(store, q), q


# ---------------------------------------------------------------------------------- tile / wave / window edges
BIG = 3 * 4096 + 5


def _edge_graph():
    ns = [(1, "n")]
    raw = []
    for i in range(5000):
        raw.append((1, f"o{i:04d}", "r", f"x{i}", None, None, None))
        if i % 3 == 0:
            raw.append((1, f"o{i:04d}", "r", "u", None, None, None))
    raw += [(1, "o2500", "r", f"b{j:05d}", None, None, None) for j in range(BIG)]
    return ns, raw


def _edge_queries(store):
    big = ("n", "o2500", "r")
    q = [big + (None, 4096, p) for p in range(1, 6)]
    total = list_util.count_key_part(store, "n", "", "")
    # windows whose first or last entry is 63, 64, 65 (lane and wave-step edges) and 4095, 4096, 4097 (tile edges),
    # over the whole namespace (tiles start at its first entry) and over the big row (an entry range that
    # starts anywhere)
    for key in (("n", "", ""), big):
        q += [key + (None, 64, p) for p in (1, 2, 64, 65)]              # [0,64) [64,128) [4032,4096) [4096,4160)
        q += [key + (None, 63, p) for p in (1, 2, 65, 66)]              # [0,63) [63,126) [4032,4095) [4095,4158)
        q += [key + (None, 65, p) for p in (1, 2)]                      # [0,65) [65,130)
        q += [key + (None, 4097, p) for p in (1, 2)]                    # [0,4097) [4097,8194)
    u = SubjectID("u")
    n_u = len([i for i in range(5000) if i % 3 == 0])
    q += [("n", "", "", u, 1, p) for p in (1, 2, n_u // 2, n_u - 1, n_u, n_u + 1)]
    q += [("n", "", "", u, 100, p) for p in range(1, n_u // 100 + 3)]
    q += [("n", "", "", u, 10 ** 6, p) for p in (1, 2)]
    q += [("", "", "r", u, 100, 3), ("", "o0003", "", u, 0, 1), ("n", "", "", SubjectID("b00007"), 0, 1)]
    # past the end, and the largest sizes and pages the request can carry
    q += [("n", "", "", None, 100, total // 100 + 2), ("n", "", "", None, 2 ** 31 - 1, 1),
          ("n", "", "", None, 2 ** 31 - 1, 2 ** 32 - 1), big + (None, 1, 2 ** 32 - 1)]
    return q


def run_edges():
    """The edge queries against SQLite, with whatever KETO_LIST_TILE the process has."""
    import keto_amd
    ns, raw = _edge_graph()
    store = SQLStore(ns, raw_rows=raw)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, [], raw), device=0)
    before = snap.stats()["device_bytes"]
    queries = _edge_queries(store)
    got = _compare(snap, store, queries, allow=(LIST_OK,))
    assert [len(g[1]) for g in got[:5]] == [4096, 4096, 4096, 6, 0] and got[3][2] == ""
    # the index is counted as device memory: 8 B per tuple at least
    assert snap.stats()["device_bytes"] >= before + 8 * len(raw)
    return len(queries)


def test_tile_wave_and_window_edges():
    assert "KETO_LIST_TILE" not in os.environ
    run_edges()


def test_tile_wave_and_window_edges_tile_256():
    env = dict(os.environ, KETO_LIST_TILE="256")
    code = "import tests.test_gpu_list as t; print('edge queries ok:', t.run_edges())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "edge queries ok:" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_bad_tile_is_an_error():
    env = dict(os.environ, KETO_LIST_TILE="100")
    code = ("import keto_amd\n"
            "s = keto_amd.Snapshot.build([(1, 'n')], [(1, 'a', 'r', 'u')], device=0)\n"
            "try:\n    s.list_batch([('n', '', '', None, 0, 0)])\nexcept keto_amd.KetoError as e:\n    print('code', e.code)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "code -1" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------- after writes
def test_lists_after_writes():
    import keto_amd
    ns = [(1, "n"), (2, "m")]
    T = RelationTuple
    tuples = [T("n", "a", "r", SubjectID("u")), T("n", "a", "r", SubjectID("v")), T("n", "b", "r", SubjectSet("m", "g", "s")),
              T("m", "g", "s", SubjectID("u")), T("n", "c", "t", SubjectID("w")), T("n", "a", "r", SubjectID("u"))]
    store = SQLStore(ns, tuples, page_size=3)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), page_size=3, device=0)
    keys = list(itertools.product(["n", "m", ""], ["a", "b", "g", "aa", ""], ["r", "s", ""]))
    subjects = [None, SubjectID("u"), SubjectID("zed"), SubjectSet("m", "g", "s"), SubjectSet("n", "aa", "r")]
    _compare(snap, store, _all_pages(store, keys, subjects, sizes=(0, 2)), allow=(LIST_OK,))
    old = snap.list_batch_raw([("", "", "", None, 100, 0)])
    old_dec = snap.decode_list_tuples(old[2])
    assert len(old_dec) == len(tuples)

    # a new row between existing ones, a new string sorting before the build's, a duplicate, a new subject
    # set (its target row is new too); then deletes: every equal tuple, and a tuple that does not exist
    ins = [T("n", "aa", "r", SubjectID("zed")), T("n", "a", "r", SubjectID("A")), T("n", "a", "r", SubjectID("v")),
           T("m", "g", "s", SubjectSet("n", "aa", "r")), T("n", "0", "r", SubjectID("u"))]
    dels = [T("n", "a", "r", SubjectID("u")), T("n", "c", "t", SubjectID("nobody"))]
    v0 = snap.version()
    assert snap.apply([rows_from_tuples(ns, [t])[0] for t in ins], [rows_from_tuples(ns, [t])[0] for t in dels]) == v0 + 1
    for t in ins:
        store.insert(t)
    for t in dels:
        store.delete(t)
    _compare(snap, store, _all_pages(store, keys + [("n", "0", "r"), ("", "0", "")], subjects, sizes=(0, 2)),
             allow=(LIST_OK,))
    # a second write, so that the index is rebuilt from rows a write already changed
    snap.apply([rows_from_tuples(ns, [T("n", "aa", "r", SubjectID("u"))])[0]],
               [rows_from_tuples(ns, [T("n", "aa", "r", SubjectID("zed"))])[0]])
    store.insert(T("n", "aa", "r", SubjectID("u")))
    store.delete(T("n", "aa", "r", SubjectID("zed")))
    _compare(snap, store, _all_pages(store, keys, subjects, sizes=(0, 2)), allow=(LIST_OK,))
    # row ids and string ids are only appended: the result taken before the writes decodes as before
    assert snap.decode_list_tuples(old[2]) == old_dec


# ---------------------------------------------------------------------------------- batch independence
def test_batch_independence():
    import keto_amd
    store, ns, tuples, raw, ps, (names, objs, rels, users) = random_store(1234, n_tuples=40)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=0)
    stored = [t.subject for t in tuples if isinstance(t.subject, SubjectSet)]
    subs = [None, None] + [list_util.subject_key(s) for s in [SubjectID(u) for u in users] + stored[:3]]
    subs.append(("set", "nope", "a", "r"))
    import random
    rng = random.Random(5)
    queries = [(rng.choice(names + ["", "nope"]), rng.choice(objs + ["", "zz"]), rng.choice(rels + [""]),
                rng.choice(subs), rng.choice([0, 1, 2, 7]), rng.randrange(0, 6)) for _ in range(500)]
    together = snap.list_batch(queries)
    assert len(together) == 500
    for q, t in zip(queries, together):
        assert snap.list_batch([q]) == [t], q
    assert {t[0] for t in together} >= {LIST_OK, LIST_NOT_FOUND}


# ---------------------------------------------------------------------------------- errors
def test_partitioned_snapshot_is_invalid_and_empty_batch_is_fine():
    import keto_amd
    ns = [(1, "n")]
    rows = [(1, "a", "r", "u"), (1, "b", "r", None, 1, "a", "r")]
    part = keto_amd.Snapshot.build(ns, rows, device=-1).upload_part(0, 2, device=0)
    with pytest.raises(keto_amd.KetoError) as e:
        part.list_batch([("n", "", "", None, 0, 0)])
    assert e.value.code == -1                                   # KETO_E_INVALID
    snap = keto_amd.Snapshot.build(ns, rows, device=0)
    status, offs, tup, nxt, tot, _ = snap.list_batch_raw([])
    assert len(status) == 0 and list(offs) == [0] and len(tup) == 0 and len(nxt) == 0 and len(tot) == 0
    assert snap.list_batch([]) == []
    got = snap.list_batch([("n", "", "", None, 0, 0)])
    assert got == [(LIST_OK, [("n", "a", "r", ("id", "u")), ("n", "b", "r", ("set", "n", "a", "r"))], "", 2)]
