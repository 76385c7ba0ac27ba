"""keto_allowed_subjects_batch on the GPU against two oracles: one SubjectIsAllowed per subject id of the store
on the SQL oracle (tests/allowed_util.py), and on the device the brute force -- keto_check_batch_pairs over
(the query's row, every string id of the snapshot), whose allowed ids in ascending order must equal the call's
and whose undecided count must be 0 (every test but the KETO_ALLOWED_UNDECIDED one; the graphs are small)."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.oracle_sql import ExpandEngine, RelationTuple, SQLStore, SubjectID, SubjectSet
from tests import allowed_util, staircase
from tests.allowed_util import ALLOWED_OK, ALLOWED_UNDECIDED, ALLOWED_UNKNOWN_NAMESPACE, ALLOWED_UNSUPPORTED
from tests.engine_util import rows_from_tuples
from tests.randgraph import random_store

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = RelationTuple


def _build(ns, tuples, raw=(), page_size=100):
    import keto_amd
    store = SQLStore(ns, tuples, page_size=page_size, raw_rows=list(raw))
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, list(raw)), page_size=page_size, device=0)
    return store, snap


def _row_of(snap, ns, obj, rel):
    """The row id of (ns, obj, rel), from the first tuple the list call returns for it; None without one."""
    status, offs, tuples = snap.list_batch_raw([(ns, obj, rel, None, 1, 0)])[:3]
    if status[0] != 0 or offs[1] == offs[0]:
        return None
    return int(tuples["row"][0])


def brute_force(snap, ns, obj, rel, depth, gmd):
    """(the string ids keto_check_batch_pairs allows on the row of (ns, obj, rel), ascending; undecided checks)
    over every string id of the snapshot; None when the list call shows no tuple of the row."""
    from keto_amd.capi import CHECK_PAIR_DTYPE, UNDECIDED
    row = _row_of(snap, ns, obj, rel)
    if row is None:
        return None
    n = snap.stats()["n_strings"]
    pairs = np.zeros(n, dtype=CHECK_PAIR_DTYPE)
    pairs["row"], pairs["subject"] = row, np.arange(n, dtype=np.uint32)
    dec = snap.check_batch_pairs(pairs, depth, gmd)
    return np.nonzero(dec == 1)[0].astype(np.uint32), int((dec == UNDECIDED).sum())


def _all_pages(store, heads, sizes, gmd, cache):
    """heads: (namespace, object, relation, depth) -> every page of each at every size, one past the last."""
    out = []
    for (ns, obj, rel, depth), size in itertools.product(heads, sizes):
        total = allowed_util.expected(store, (ns, obj, rel, depth, size, 1), gmd, cache)[3]
        last = allowed_util.last_page(total, size if size else store.page_size)
        out += [(ns, obj, rel, depth, size, page) for page in range(1, last + 2)]
    return out


def _compare(snap, store, queries, gmd=5, cache=None, brute=True):
    """One call for `queries`; every answer equals the SQL oracle's, and the whole set of every distinct
    (namespace, object, relation, depth) equals the device brute force.  Returns allowed_subjects' tuples."""
    cache = {} if cache is None else cache
    got = snap.allowed_subjects(list(queries), gmd)
    raw = snap.allowed_subjects_raw(list(queries), gmd)
    assert len(got) == len(queries)
    for i, (q, g) in enumerate(zip(queries, got)):
        want = allowed_util.expected(store, q, gmd, cache)
        assert g[:4] == want, (q, gmd, g, want)
        assert g[5] == 0 and g[4] >= g[3], (q, g)
        ids = raw["ids"][int(raw["offsets"][i]):int(raw["offsets"][i + 1])]
        assert np.all(ids[1:] > ids[:-1]), (q, ids)                      # ascending string ids
    if brute:
        heads = {}
        for i, q in enumerate(queries):
            if got[i][0] == ALLOWED_OK:
                heads.setdefault(q[:4], []).append(i)
        whole = snap.allowed_subjects_raw([h + (2 ** 31 - 1, 1) for h in heads], gmd)
        for k, h in enumerate(heads):
            bf = brute_force(snap, h[0], h[1], h[2], h[3], gmd)
            ids = whole["ids"][int(whole["offsets"][k]):int(whole["offsets"][k + 1])]
            if bf is None:
                continue
            assert bf[1] == 0, (h, bf)
            assert np.array_equal(ids, bf[0]), (h, gmd, ids, bf[0])
            assert int(whole["totals"][k]) == len(bf[0]) and int(whole["candidates"][k]) >= len(bf[0])
    return got


# ---------------------------------------------------------------------------------- the hand example
def _hand():
    ns = [(1, "docs"), (2, "grp")]
    eng, ops = SubjectSet("grp", "eng", "member"), SubjectSet("grp", "ops", "member")
    tuples = [T("docs", "a", "view", SubjectID("alice")), T("docs", "b", "view", eng), T("grp", "eng", "member", SubjectID("alice")),
              T("grp", "eng", "member", SubjectID("carol")), T("docs", "c", "view", ops), T("docs", "c", "view", SubjectID("bob")),
              T("grp", "ops", "member", eng), T("docs", "d", "view", SubjectID("bob"))]
    return ns, tuples


def test_hand_example_statuses_pages_and_candidates():
    """The example of tests/test_allowed_cpu.py.  candidates = the distinct ids of the rows within depth - 1
    hops: docs:c#view reads c (bob) at depth 1, c and ops (no id) at depth 2, c, ops and eng (alice, carol)
    at depth 3."""
    ns, tuples = _hand()
    store, snap = _build(ns, tuples, page_size=2)
    queries = [("docs", "c", "view", 0, 100, 0), ("nope", "c", "view", 0, 100, 0), ("docs", "c", "view", 2, 100, 0),
               ("docs", "", "view", 0, 100, 0), ("docs", "c", "view", 1, 100, 0), ("docs", "zz", "view", 0, 100, 0),
               ("", "c", "view", 0, 100, 0), ("docs", "c", "", 0, 100, 0), ("docs", "c", "edit", 0, 100, 0),
               ("docs", "c", "view", 3, 100, 0), ("docs", "b", "view", 1, 100, 0), ("docs", "b", "view", 2, 100, 0),
               ("docs", "c", "view", 0, 0, 0), ("docs", "c", "view", 0, 0, 2), ("docs", "c", "view", 0, 0, 3),
               ("docs", "c", "view", 0, 1, 2), ("grp", "ops", "member", 0, 100, 0), ("docs", "a", "view", 1, 100, 0)]
    got = _compare(snap, store, queries, 5)
    assert got[0] == (ALLOWED_OK, ["alice", "bob", "carol"], "", 3, 3, 0)
    assert got[1] == (ALLOWED_UNKNOWN_NAMESPACE, [], "", 0, 0, 0)
    assert got[2] == (ALLOWED_OK, ["bob"], "", 1, 1, 0)
    assert got[3] == got[6] == got[7] == (ALLOWED_UNSUPPORTED, [], "", 0, 0, 0)
    assert got[4] == (ALLOWED_OK, ["bob"], "", 1, 1, 0)
    assert got[5] == got[8] == (ALLOWED_OK, [], "", 0, 0, 0)              # unknown object / relation string
    assert got[9] == got[0]
    assert got[10] == (ALLOWED_OK, [], "", 0, 0, 0) and got[11] == (ALLOWED_OK, ["alice", "carol"], "", 2, 2, 0)
    assert got[12] == (ALLOWED_OK, ["alice", "bob"], "2", 3, 3, 0) and got[13] == (ALLOWED_OK, ["carol"], "", 3, 3, 0)
    assert got[14] == (ALLOWED_OK, [], "", 3, 3, 0) and got[15] == (ALLOWED_OK, ["bob"], "3", 3, 3, 0)
    # the global clamp; every query alone answers as in the batch
    clamped = _compare(snap, store, [("docs", "c", "view", 0, 100, 0), ("docs", "c", "view", 7, 100, 0)], 2)
    assert clamped == [(ALLOWED_OK, ["bob"], "", 1, 1, 0)] * 2
    for q, g in zip(queries, got):
        assert snap.allowed_subjects([q], 5) == [g], q
    # batches that need no device work, and the empty batch
    assert snap.allowed_subjects([queries[3], queries[1]], 5) == [got[3], got[1]]
    r = snap.allowed_subjects_raw([])
    assert len(r["status"]) == 0 and list(r["offsets"]) == [0] and len(r["ids"]) == 0
    assert snap.allowed_subjects([], 5) == []
    t = snap.allowed_subjects_raw(queries[:1])["timing"]
    assert len(t) == 4 and all(x >= 0 for x in t) and t[2] > 0


# ---------------------------------------------------------------------------------- the depth edge
def test_depth_edge_on_a_chain():
    """top -> g1 -> g2 -> g3 -> g4 -> user: user is 4 hops from top's row and needs depth 5.  Under a global
    max-depth of 5: request depth 4 stops one hop short, 5 reaches it, 6 and 0 are clamped to 5.  A search that
    stopped a level early would lose user at 5."""
    L = 4
    ns = [(1, "n")]
    tuples = [T("n", "top", "r", SubjectSet("n", "g1", "r"))]
    tuples += [T("n", f"g{k}", "r", SubjectSet("n", f"g{k + 1}", "r")) for k in range(1, L)]
    tuples += [T("n", f"g{L}", "r", SubjectID("user")), T("n", "g2", "r", SubjectID("near"))]
    store, snap = _build(ns, tuples)
    got = _compare(snap, store, [("n", "top", "r", d, 100, 0) for d in (L, L + 1, L + 2, 0, 3, 2, 1)], 5)
    assert [g[1] for g in got] == [["near"], ["near", "user"], ["near", "user"], ["near", "user"], ["near"], [], []]
    assert [g[4] for g in got] == [1, 2, 2, 2, 1, 0, 0]
    # from g1 user is 3 hops away
    got = _compare(snap, store, [("n", "g1", "r", d, 100, 0) for d in (3, 4)], 5)
    assert [g[1] for g in got] == [["near"], ["near", "user"]]


# ---------------------------------------------------------------------------------- the visited-map quirk
@pytest.mark.parametrize("gmd", (4, 5))
def test_staircase_twins(gmd):
    """tests/staircase.py: with first_visit the check denies user although X -> user is within reach (X entered
    the visited map where no depth was left to open it); without, it allows.  This call follows the check in
    both.  keto_subjects_batch follows Expand instead (the oracle's ExpandEngine says what it returns), and
    Expand differs from the check in both directions.  At global max-depth 5 its tree opens X under z whether
    or not the chain met X first, so it returns user in the first_visit case, where every check denies.  At 4
    X sits where Expand's depth cut makes it a leaf, so it returns nobody, also without first_visit, where the
    check allows user."""
    cases = []
    for k1, k2 in ((0, 0), (3, 2), (5, 1), (9, 4)):
        for fv in (True, False):
            i = len(cases)
            cases.append(staircase.Case(i, f"s{i:03d}_", k1, k2, gmd, fv))
    tuples = staircase.all_tuples(cases)
    store, snap = _build(staircase.NS, tuples)
    queries = [("n", c.tag + "top", "r", 0, 100, 0) for c in cases]
    got = _compare(snap, store, queries, gmd)
    flat = snap.subjects(queries, gmd)
    for c, g, f in zip(cases, got, flat):
        assert g[0] == ALLOWED_OK and (g[1] == [] if c.first_visit else g[1] == ["user"]), (c, g)
        tree = ExpandEngine(store, gmd).build_tree(SubjectSet("n", c.tag + "top", "r"), 0)
        in_tree = '"user"' in json.dumps(tree.to_json())
        assert (f[1] == ["user"]) == in_tree and f[1] in ([], ["user"]), (c, f)
        if gmd == 5 and c.first_visit:
            assert f[1] == ["user"] and g[1] == []   # Expand's flatten has user, the check denies
        if gmd == 4 and not c.first_visit:
            assert f[1] == [] and g[1] == ["user"]   # the check allows, Expand's depth cut loses user


# ---------------------------------------------------------------------------------- cycles and shared substructure
def test_cycles_and_a_ladder_of_diamonds():
    """A 2-cycle, a self-loop, and a ladder of 20 diamonds (d_k -> l_k, r_k -> d_k+1: 2^20 paths, 61 rows) at
    global max-depth 45: every row is expanded once per query, candidates = the distinct reachable ids."""
    ns = [(1, "n")]
    S = lambda o: SubjectSet("n", o, "r")
    tuples = [T("n", "p", "r", S("q")), T("n", "q", "r", S("p")), T("n", "p", "r", SubjectID("up")), T("n", "q", "r", SubjectID("uq")),
              T("n", "self", "r", S("self")), T("n", "self", "r", SubjectID("us"))]
    K = 20
    for k in range(K):
        tuples += [T("n", f"d{k:02d}", "r", S(f"l{k:02d}")), T("n", f"d{k:02d}", "r", S(f"r{k:02d}")),
                   T("n", f"l{k:02d}", "r", S(f"d{k + 1:02d}")), T("n", f"r{k:02d}", "r", S(f"d{k + 1:02d}")),
                   T("n", f"l{k:02d}", "r", SubjectID(f"m{k:02d}"))]
    tuples.append(T("n", f"d{K:02d}", "r", SubjectID("bottom")))
    store, snap = _build(ns, tuples)
    # (the SQL oracle walks every path: it is asked only where the paths are few)
    got = _compare(snap, store, [("n", "p", "r", 0, 100, 0), ("n", "q", "r", 2, 100, 0), ("n", "self", "r", 0, 100, 0),
                                 ("n", "d17", "r", 0, 100, 0)], 45)
    assert got[0][1] == ["up", "uq"] and got[1][1] == ["up", "uq"] and got[2][1] == ["us"]
    assert got[3][1] == ["bottom", "m17", "m18", "m19"] and got[3][4] == 4
    r = snap.allowed_subjects([("n", "d00", "r", 0, 100, 0), ("n", "d00", "r", 40, 100, 0), ("n", "d00", "r", 41, 100, 0)], 45)
    bf = brute_force(snap, "n", "d00", "r", 0, 45)
    every = sorted(["bottom"] + [f"m{k:02d}" for k in range(K)])
    assert bf[1] == 0 and [f[1] for f in snap.subject_fields(bf[0])] == every
    assert r[0] == (ALLOWED_OK, every, "", K + 1, K + 1, 0) and r[2] == r[0]
    assert r[1] == (ALLOWED_OK, every[1:], "", K, K, 0)                  # d20 is 40 hops away: depth 41


# ---------------------------------------------------------------------------------- row shapes
def test_row_shapes_small():
    """Rows of every layout on the path, against both oracles: sets and an id inside the header's window, a
    frontier of 65 set rows (a wave's edge), a ROW_SEQ row (a subject id whose text is a stored set's String()),
    a materialized wildcard row (a stored subject set with an empty object), and a poisoned row (a subject set
    of a namespace id the config lacks)."""
    ns = [(1, "n"), (2, "g")]
    S = lambda o, nsn="g": SubjectSet(nsn, o, "m")
    tuples = [T("n", "win", "r", S("w1")), T("n", "win", "r", S("w2")), T("n", "win", "r", S("w3")), T("n", "win", "r", SubjectID("direct")),
              T("g", "w1", "m", SubjectID("a1")), T("g", "w2", "m", SubjectID("a2")), T("g", "w3", "m", SubjectID("a3"))]
    tuples += [T("n", "fan65", "r", S(f"f{i:03d}")) for i in range(65)]
    tuples += [T("g", f"f{i:03d}", "m", SubjectID(f"u{i % 50:02d}")) for i in range(65)]
    tuples += [T("g", f"f{i:03d}", "m", S("w3")) for i in range(0, 65, 7)]
    # ROW_SEQ: the id "g:w1#m" prints like the set g:w1#m
    tuples += [T("n", "seq", "r", S("w1")), T("n", "seq", "r", SubjectID("g:w1#m")), T("n", "seq", "r", SubjectID("plain")),
               T("n", "viaseq", "r", SubjectSet("n", "seq", "r"))]
    # a materialized wildcard row: every g:*#m row
    tuples += [T("n", "wild", "r", SubjectSet("g", "", "m")), T("n", "viawild", "r", SubjectSet("n", "wild", "r"))]
    # a poisoned row on the path (namespace id 99 is not configured), next to a healthy one
    raw = [(1, "pois", "m", None, 99, "x", "m")]
    tuples += [T("n", "pois", "m", SubjectID("behind")), T("n", "viapois", "r", SubjectSet("n", "pois", "m")), T("n", "viapois", "r", S("w2"))]
    store, snap = _build(ns, tuples, raw)
    st = snap.stats()
    assert st["n_seq_rows"] >= 1 and st["n_wildcard_rows"] >= 1 and st["n_poisoned_rows"] >= 1
    heads = [("n", o, "r", d) for o in ("win", "fan65", "seq", "viaseq", "viapois", "wild", "viawild") for d in (0, 1, 2, 3)]
    heads += [("n", "pois", "m", 0), ("g", "f007", "m", 2)]
    got = _compare(snap, store, [h + (2 ** 31 - 1, 0) for h in heads], 5)
    by = {h: g for h, g in zip(heads, got)}
    assert by[("n", "win", "r", 1)][1] == ["direct"] and by[("n", "win", "r", 2)][1] == ["a1", "a2", "a3", "direct"]
    assert by[("n", "fan65", "r", 2)][3] == 50 and by[("n", "fan65", "r", 3)][3] == 51
    assert "plain" in by[("n", "seq", "r", 1)][1] and "g:w1#m" in by[("n", "seq", "r", 1)][1]
    assert "a1" in by[("n", "viaseq", "r", 3)][1] and "a1" not in by[("n", "viaseq", "r", 2)][1]
    assert "a2" in by[("n", "viapois", "r", 2)][1]
    assert by[("n", "wild", "r", 2)][3] > 50


def test_row_shapes_large():
    """An id table past a 256-thread step (300 ids), a row of several tiles (5,000 ids, and a set behind them),
    a frontier of 257 set rows (a block's edge).  The SQL oracle would spend 5,000 walks over 5,000 tuples per
    query here, so these are held against the device brute force and against lists written by hand."""
    ns = [(1, "n"), (2, "g")]
    S = lambda o: SubjectSet("g", o, "m")
    tuples = [T("g", "w1", "m", SubjectID("a1")), T("g", "w2", "m", SubjectID("a2")), T("g", "w3", "m", SubjectID("a3"))]
    tuples += [T("n", "tab", "r", SubjectID(f"t{i:04d}")) for i in range(300)]
    tuples += [T("n", "big", "r", S("bigset")), T("n", "big", "r", S("w1"))]
    tuples += [T("g", "bigset", "m", SubjectID(f"b{i:05d}")) for i in range(5000)] + [T("g", "bigset", "m", S("w2"))]
    tuples += [T("n", "fan257", "r", S(f"f{i:03d}")) for i in range(257)]
    tuples += [T("g", f"f{i:03d}", "m", SubjectID(f"u{i % 50:02d}")) for i in range(257)]
    tuples += [T("g", f"f{i:03d}", "m", S("w3")) for i in range(0, 257, 7)]
    store, snap = _build(ns, tuples)
    tab, big, fan = [f"t{i:04d}" for i in range(300)], [f"b{i:05d}" for i in range(5000)], [f"u{i:02d}" for i in range(50)]
    want = {("n", "tab", "r", 1): tab, ("n", "tab", "r", 0): tab, ("n", "big", "r", 1): [], ("n", "big", "r", 2): ["a1"] + big,
            ("n", "big", "r", 3): ["a1", "a2"] + big, ("g", "bigset", "m", 1): big, ("g", "bigset", "m", 0): ["a2"] + big,
            ("n", "fan257", "r", 1): [], ("n", "fan257", "r", 2): fan, ("n", "fan257", "r", 0): ["a3"] + fan}
    heads = list(want)
    got = snap.allowed_subjects([h + (2 ** 31 - 1, 0) for h in heads], 5)
    for h, g in zip(heads, got):
        assert g == (ALLOWED_OK, want[h], "", len(want[h]), len(want[h]), 0), (h, g[1][:5], g[2:])
        bf = brute_force(snap, h[0], h[1], h[2], h[3], 5)
        assert bf[1] == 0 and [f[1] for f in snap.subject_fields(bf[0])] == want[h], h
    # pages across the 5,000-id row: sizes on both sides of a 256 step, the last page short, one past the end
    for size in (2047, 2560):
        last = -(-5000 // size)
        got = snap.allowed_subjects([("g", "bigset", "m", 1, size, p) for p in range(1, last + 2)], 5)
        assert sum((g[1] for g in got), []) == big and got[-1][1] == [] and got[-2][2] == "" and got[0][2] == "2"
        assert all(g[3] == 5000 and g[4] == 5000 for g in got)


def test_forwarded_row_and_a_subject_written_after_the_build():
    """keto_snapshot_apply grows g:grp#m past its place in the arena (its identity header becomes a forward,
    which every subject set still points at); the subjects it adds are new strings, whose ids lie behind every
    older one whatever their bytes: the call's order is the string id's."""
    ns = [(1, "n"), (2, "g")]
    grp = SubjectSet("g", "grp", "m")
    tuples = [T("n", "doc", "r", grp), T("n", "doc", "r", SubjectID("zed")), T("g", "grp", "m", SubjectID("mid")),
              T("g", "other", "m", SubjectID("o1")), T("n", "doc2", "r", SubjectSet("g", "other", "m"))]
    store, snap = _build(ns, tuples)
    before = _compare(snap, store, [("n", "doc", "r", 0, 100, 0)], 5)
    assert before[0][1] == ["mid", "zed"]
    assert snap.allowed_subjects_raw([("n", "doc", "r", 0, 100, 0), ("g", "grp", "m", 1, 100, 0)], 5)["bfs"]["forwards"] == 0
    ins = [T("g", "grp", "m", SubjectID(f"added{i:02d}")) for i in range(40)]
    v0 = snap.version()
    assert snap.apply([rows_from_tuples(ns, [t])[0] for t in ins], []) == v0 + 1
    for t in ins:
        store.insert(t)
    queries = [("n", "doc", "r", 0, 100, 0), ("g", "grp", "m", 1, 100, 0), ("n", "doc2", "r", 0, 100, 0)]
    got = snap.allowed_subjects(queries, 5)
    new = [f"added{i:02d}" for i in range(40)]
    assert got[0] == (ALLOWED_OK, ["mid", "zed"] + new, "", 42, 42, 0)   # "added.." sorts first by bytes, last by id
    assert got[1] == (ALLOWED_OK, ["mid"] + new, "", 41, 41, 0) and got[2][1] == ["o1"]
    raw = snap.allowed_subjects_raw(queries, 5)
    assert np.all(np.diff(raw["ids"][:42].astype(np.int64)) > 0)
    # the BFS met the moved row through its forward: as level 1 of the first query, as level 0 of the second
    assert raw["bfs"]["forwards"] == 2 and raw["bfs"]["reruns"] == 0
    assert snap.allowed_subjects_raw(queries[2:], 5)["bfs"]["forwards"] == 0
    for q, g in zip(queries, got):
        want = allowed_util.expected(store, q, 5)
        assert g[0] == want[0] and sorted(g[1]) == sorted(want[1]) and g[3] == want[3], (q, g, want)
        bf = brute_force(snap, q[0], q[1], q[2], q[3], 5)
        assert bf[1] == 0 and [f[1] for f in snap.subject_fields(bf[0])] == g[1]


# ---------------------------------------------------------------------------------- random graphs, knobs
def _random_queries(seed, gmd, cache, store, alph):
    names, objs, rels, users = alph
    named = [n for n in names if n != ""]
    keys = list(itertools.product(named + ["nope"], objs, rels))
    heads = [k + (d,) for k in keys for d in ((seed + len(k[1])) % 6, (seed + 3) % 6)]
    return _all_pages(store, heads, (1, 3, 0), gmd, cache)


@pytest.mark.parametrize("seed", range(20))
def test_random_graphs(seed):
    """tests/randgraph.py (cycles, duplicates, collisions, wildcard sets, poisoned pages): every (namespace,
    object, relation) of the alphabet and an unknown namespace, two of the depths 0..5 each (all of them over
    the seeds), every page at sizes 1, 3 and the snapshot's, at global max-depth 5 and 3."""
    import keto_amd
    store, ns, tuples, raw, ps, alph = random_store(seed)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=0)
    for gmd in (5, 3):
        cache = {}
        _compare(snap, store, _random_queries(seed, gmd, cache, store, alph), gmd, cache)
    snap.close()


def _knob_batch():
    """64 queries over one random graph big enough for several levels: (raw arrays, tuples) of the call."""
    import keto_amd
    store, ns, tuples, raw, ps, alph = random_store(77, n_tuples=400, allow_wildcards=False, allow_poison=False)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=0)
    names, objs, rels, users = alph
    keys = list(itertools.product(names, objs, rels))
    queries = [keys[i % len(keys)] + ((i // len(keys)) % 6, (0, 2, 100)[i % 3], i % 3) for i in range(64)]
    return snap, store, queries


def test_knobs_change_nothing(monkeypatch):
    """KETO_ALLOWED_VISITED_SLOTS=64 (the table starts too small and is enlarged: keto_allowed_bfs says so), KETO_ALLOWED_CHUNK=64
    (several check chunks): the arrays of the default run, bit for bit.  KETO_ALLOWED_MAX_CANDIDATES=8:
    KETO_E_INVALID and no result.  The knobs are read by every call."""
    import keto_amd
    snap, store, queries = _knob_batch()
    base = snap.allowed_subjects_raw(queries, 5)
    assert int(base["candidates"].sum()) > 64 and len(base["ids"]) > 0
    cache = {}
    for q, g in zip(queries, snap.allowed_subjects(queries, 5)):
        assert g[:4] == allowed_util.expected(store, q, 5, cache), q
    assert base["bfs"]["reruns"] == 0 and base["bfs"]["visited"] > 128      # (under 2^16 keys the table is sized for a level's bound)
    for name, val in (("KETO_ALLOWED_VISITED_SLOTS", "64"), ("KETO_ALLOWED_CHUNK", "64")):
        monkeypatch.setenv(name, val)
        r = snap.allowed_subjects_raw(queries, 5)
        monkeypatch.delenv(name)
        if name == "KETO_ALLOWED_VISITED_SLOTS":
            # 64 seeds start on 128 slots; the visited keys do not fit in half of that
            assert r["bfs"]["regrows"] + r["bfs"]["reruns"] >= 1 and r["bfs"]["slots"] >= 2 * r["bfs"]["visited"]
            assert r["bfs"]["visited"] == base["bfs"]["visited"] and r["bfs"]["levels"] == base["bfs"]["levels"]
        for k in ("status", "offsets", "ids", "next_page", "totals", "candidates", "undecided"):
            assert np.array_equal(r[k], base[k]), (name, k)
    monkeypatch.setenv("KETO_ALLOWED_MAX_CANDIDATES", "8")
    with pytest.raises(keto_amd.KetoError) as e:
        snap.allowed_subjects_raw(queries, 5)
    assert e.value.code == -1
    h = __import__("ctypes").c_void_p(123)
    arr = (keto_amd.capi.KAllowedReq * 1)()
    arr[0].namespace_ = keto_amd.capi.KStr(queries[0][0].encode(), len(queries[0][0].encode()))
    arr[0].object = keto_amd.capi.KStr(b"a", 1)
    arr[0].relation = keto_amd.capi.KStr(b"r", 1)
    monkeypatch.setenv("KETO_ALLOWED_CHUNK", "7")                        # below 64: refused, *out cleared
    assert snap.lib.keto_allowed_subjects_batch(snap.h, arr, 1, 5, __import__("ctypes").byref(h)) == -1 and not h.value
    monkeypatch.delenv("KETO_ALLOWED_CHUNK")
    monkeypatch.delenv("KETO_ALLOWED_MAX_CANDIDATES")
    r = snap.allowed_subjects_raw(queries, 5)
    assert np.array_equal(r["ids"], base["ids"])


# ---------------------------------------------------------------------------------- thousands of queries, a fanning frontier
FAN_ROOTS, FAN_KIDS, FAN_GRAND, FAN_POOL = 2048, 8, 4, 512


def _fan_snapshot():
    """2,048 roots, each over 8 rows of its own, each of those over 4 of 512 shared rows that hold one id each:
    per query 1 + 8 + (at most 32) visited rows, the frontier growing eightfold and then fourfold."""
    import keto_amd
    ns = [(1, "n")]
    rows = [(1, f"g{k:03d}", "r", f"u{k:03d}") for k in range(FAN_POOL)]
    want = []
    for i in range(FAN_ROOTS):
        pool = set()
        for j in range(FAN_KIDS):
            c = i * FAN_KIDS + j
            rows.append((1, f"root{i:04d}", "r", None, 1, f"c{c:05d}", "r"))
            for t in range(FAN_GRAND):
                k = (c * 5 + t * 131) % FAN_POOL
                rows.append((1, f"c{c:05d}", "r", None, 1, f"g{k:03d}", "r"))
                pool.add(k)
        want.append(sorted(pool))
    return keto_amd.Snapshot.build(ns, rows, device=0), want


def test_thousands_of_queries_with_a_fanning_frontier(monkeypatch):
    """The visited table under a frontier that outgrows it: every level is run at most twice, the table ends no
    larger than a small multiple of the visited keys, and the answer is the hand-computed one for all 2,048
    queries (a sample is held against the device brute force) -- with the table started at 64 slots too, where
    it is both enlarged ahead of a level and found too small by one."""
    snap, want = _fan_snapshot()
    queries = [("n", f"root{i:04d}", "r", 3, 2 ** 31 - 1, 0) for i in range(FAN_ROOTS)]
    visited = sum(1 + FAN_KIDS + len(w) for w in want)

    def check(r):
        assert not r["status"].any() and not r["undecided"].any()
        for i in (0, 1, 777, FAN_ROOTS - 1):
            ids = r["ids"][int(r["offsets"][i]):int(r["offsets"][i + 1])]
            assert [f[1] for f in snap.subject_fields(ids)] == [f"u{k:03d}" for k in want[i]]
        assert r["totals"].tolist() == [len(w) for w in want] == r["candidates"].tolist()
        b = r["bfs"]
        assert b["visited"] == visited and b["levels"] == 3 and b["reruns"] <= b["levels"], b
        assert 2 * visited <= b["slots"] <= 16 * visited, b            # sized for the keys, within the bound's slack
        return b

    base = snap.allowed_subjects_raw(queries, 5)
    check(base)
    for i in (0, 777):
        bf = brute_force(snap, "n", f"root{i:04d}", "r", 3, 5)
        assert bf[1] == 0 and np.array_equal(bf[0], base["ids"][int(base["offsets"][i]):int(base["offsets"][i + 1])])
    # depth 2 stops above the shared rows: nothing is allowed, and the third level is not run
    short = snap.allowed_subjects_raw([q[:3] + (2,) + q[4:] for q in queries], 5)
    assert not short["totals"].any() and short["bfs"]["visited"] == FAN_ROOTS * (1 + FAN_KIDS)
    monkeypatch.setenv("KETO_ALLOWED_VISITED_SLOTS", "64")
    small = snap.allowed_subjects_raw(queries, 5)
    monkeypatch.delenv("KETO_ALLOWED_VISITED_SLOTS")
    b = check(small)
    assert b["regrows"] >= 1 and b["reruns"] >= 1, b
    for k in ("status", "offsets", "ids", "next_page", "totals", "candidates", "undecided"):
        assert np.array_equal(small[k], base[k]), k


# ---------------------------------------------------------------------------------- undecided
UNDECIDED_ENV = {"KETO_T0_CAP": "256", "KETO_T1_CAP": "1024", "KETO_NO_POOL": "1", "KETO_TEST_T2_FRAMES": "3"}


def _reachable_ids(snap, row, depth):
    """The distinct subject ids of the rows within depth - 1 hops of `row`, from the list call's tuples."""
    ids, seen, frontier = set(), {row}, [row]
    for _ in range(depth):
        fields = snap.subject_fields(np.array(frontier, dtype=np.uint32) | np.uint32(0x80000000))
        out = snap.list_batch_raw([(f[1], f[2], f[3], None, 2 ** 31 - 1, 0) for f in fields])
        subs = out[2]["subject"]
        ids.update(int(s) for s in subs[subs < 0x80000000])
        nxt = {int(s) & 0x7FFFFFFF for s in subs[subs >= 0x80000000]} - seen
        seen |= nxt
        frontier = sorted(nxt)
        if not frontier:
            break
    return np.array(sorted(ids), dtype=np.uint32)


def run_undecided():
    """The nested synthetic graph and the knobs of tests/test_gpu_lookup.py (the check's tiers shrunk), at global
    max-depth 40: group rows as roots at request depths 0, 16 and 1.  Per query the candidates are worked out
    from list calls, and `undecided` must equal the KETO_UNDECIDED decisions of keto_check_batch_rows on the
    same (row, id) pairs."""
    from keto_amd.capi import CHECK_IDS_DTYPE, UNDECIDED
    from tools import synth
    g = synth.SynthGraph(dict(n_docs=0, n_folders=0, n_groups=1 << 14, n_users=1 << 14, target_edges=0, seed=3),
                         threads=16, kind="nested", chain=32)
    u = g.unified(threads=16)
    snap = g.snapshot_unified(u, device=0)
    rows = snap.list_batch_raw([("groups", "", "member", None, 2 ** 31 - 1, 0)])[2]["row"]
    rows = rows[np.r_[True, rows[1:] != rows[:-1]]]
    roots = [int(r) for r in rows[:: len(rows) // 24][:24]]
    names = [f[2] for f in snap.subject_fields(np.array(roots, dtype=np.uint32) | np.uint32(0x80000000))]
    queries = [("groups", o, "member", d, 2 ** 31 - 1, 0) for d in (0, 16, 1) for o in names]
    r = snap.allowed_subjects_raw(queries, 40)
    n_und = n_ok = 0
    for i, (_, _, _, d, _, _) in enumerate(queries):
        row = roots[i % len(roots)]
        cand = _reachable_ids(snap, row, d if d else 40)
        ids = np.zeros(len(cand), dtype=CHECK_IDS_DTYPE)
        ids["row"], ids["target"], ids["max_depth"] = row, cand, d
        dec = snap.check_batch_rows(ids, 40) if len(cand) else np.zeros(0, dtype=np.uint8)
        und = int((dec == UNDECIDED).sum())
        got = r["ids"][int(r["offsets"][i]):int(r["offsets"][i + 1])]
        assert int(r["candidates"][i]) == len(cand) and int(r["undecided"][i]) == und, (i, len(cand), und, r["candidates"][i], r["undecided"][i])
        if und:
            assert r["status"][i] == ALLOWED_UNDECIDED and len(got) == 0 and r["totals"][i] == 0 and r["next_page"][i] == 0, i
            n_und += 1
        else:
            assert r["status"][i] == ALLOWED_OK and np.array_equal(got, cand[dec == 1]) and r["totals"][i] == len(got), i
            n_ok += 1
    assert n_und >= 1 and n_ok >= 1, (n_und, n_ok, r["undecided"].tolist())
    return f"undecided queries {n_und}, decided queries {n_ok}, undecided checks {r['undecided'].tolist()}"


def test_undecided_candidates_fail_their_query():
    """KETO_ALLOWED_UNDECIDED: no ids, total 0, and `undecided` equal to the KETO_UNDECIDED decisions of
    keto_check_batch_rows on the same candidates; a query of the batch without one is answered."""
    env = dict(os.environ, **UNDECIDED_ENV)
    code = "import tests.test_gpu_allowed as t; print('undecided ok:', t.run_undecided())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "undecided ok:" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------- lifetime and errors
def test_result_outlives_writes_and_the_snapshot():
    import keto_amd
    ns, tuples = _hand()
    store, snap = _build(ns, tuples, page_size=2)
    q = [("docs", "c", "view", 0, 100, 0), ("docs", "b", "view", 0, 100, 0)]
    want = snap.allowed_subjects_raw(q, 5)
    h = snap.allowed_subjects_handle(q, 5)
    lib = snap.lib
    try:
        snap.apply([rows_from_tuples(ns, [T("grp", "eng", "member", SubjectID("dave"))])[0]], [])
        after = snap.allowed_subjects(q, 5)
        assert after[0][1] == ["alice", "bob", "carol", "dave"] and after[1][1] == ["alice", "carol", "dave"]
        mid = snap._allowed_arrays(h)
        snap.close()
        late = keto_amd.Snapshot._allowed_arrays(type("L", (), {"lib": lib})(), h)
        for k in ("status", "offsets", "ids", "next_page", "totals", "candidates", "undecided"):
            assert np.array_equal(mid[k], want[k]) and np.array_equal(late[k], want[k]), k
    finally:
        lib.keto_allowed_free(h)


def test_partitioned_snapshot_is_invalid():
    import keto_amd
    ns = [(1, "n")]
    rows = [(1, "a", "r", "u"), (1, "b", "r", None, 1, "a", "r")]
    part = keto_amd.Snapshot.build(ns, rows, device=-1).upload_part(0, 2, device=0)
    with pytest.raises(keto_amd.KetoError) as e:
        part.allowed_subjects([("n", "b", "r", 0, 0, 0)])
    assert e.value.code == -1                                   # KETO_E_INVALID
    snap = keto_amd.Snapshot.build(ns, rows, device=0)
    assert snap.allowed_subjects([("n", "b", "r", 0, 0, 0)]) == [(ALLOWED_OK, ["u"], "", 1, 1, 0)]


def test_interleaved_with_lookup_and_subjects():
    """The three calls share a snapshot, not a workspace: interleaved, each answers as it did alone."""
    ns, tuples = _hand()
    store, snap = _build(ns, tuples)
    qa = [("docs", "c", "view", 0, 100, 0), ("docs", "b", "view", 2, 1, 2)]
    ql = [("docs", "view", ("id", "alice"), 0, 100, 0)]
    a0, l0, s0 = snap.allowed_subjects(qa, 5), snap.lookup_objects(ql, 5), snap.subjects(qa, 5)
    assert a0[0][1] == ["alice", "bob", "carol"] and a0[1] == (ALLOWED_OK, ["carol"], "", 2, 2, 0)
    assert l0[0][1] == ["a", "b", "c"] and s0[0][1] == ["alice", "bob", "carol"]
    for _ in range(3):
        assert snap.lookup_objects(ql, 5) == l0
        assert snap.allowed_subjects(qa, 5) == a0
        assert snap.subjects(qa, 5) == s0
        assert snap.allowed_subjects(qa[::-1], 5) == a0[::-1]
