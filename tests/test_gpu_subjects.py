"""keto_subjects_batch on the GPU against the two yardsticks of tests/subjects_util.py: (A) the SQL oracle's
ExpandEngine tree flattened, (B) keto_expand_batch nodes flattened with numpy.  Random graphs with every
quirk, every depth, global depth and page; agreement with check_batch at ample depth; the three sort classes
at their edges (also with KETO_SUBJECTS_LDS=128, in a child process); the expand's staging regimes; the ids
form; writes and a delete by query; partitions; two threads.

KETO_SUBJECTS_UNDECIDED: no environment switch forces an undecided expand root at small size (see the
docstring of tests/test_gpu_expand_encoded.py), so no case here holds one; the mapping from
KETO_EXPAND_UNDECIDED is implemented and such a root, having no nodes, answers with no ids and total 0.
"""
import itertools
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

from oracle.oracle_sql import RelationTuple, SQLStore, SubjectID, SubjectSet
from tests import delete_util, subjects_util
from tests.engine_util import rows_from_tuples
from tests.randgraph import random_expands, random_store
from tests.subjects_util import SUBJECTS_NOT_FOUND, SUBJECTS_OK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = RelationTuple
SET = np.uint32(0x80000000)
KETO_E_INVALID = -1


def _with_pages(heads, sizes, total_of, page_size):
    """heads: (namespace, object, relation, depth) -> every page of each at every size, one past the last."""
    out = []
    for h, size in itertools.product(heads, sizes):
        last = subjects_util.last_page(total_of(h), size if size else page_size)
        out += [h + (size, page) for page in range(1, last + 2)]
    return out


def _child(code, marker, **env):
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


# ---------------------------------------------------------------------------------- random parity
@pytest.mark.parametrize("seed", range(60))
def test_random_parity(seed):
    """Every (namespace, object, relation) of the alphabet plus wildcard objects and an unknown namespace,
    request depths {0, 1, 2, 3, 6}, every page at sizes {1, 2, 100}, at each global max-depth of {1, 3, 5}: one
    call per seed and global max-depth, equal to the oracle (A) and to the two-step path (B)."""
    import keto_amd
    store, ns, tuples, raw, ps, (names, objs, rels, users) = random_store(seed)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=0)
    heads = [(n, o, r, d) for n, o, r, d in itertools.product(names + ["nope"], objs + [""], rels, (0, 1, 2, 3, 6))]
    memo = {}
    seen = set()
    for gmd in (1, 3, 5):
        cache = {}
        total_of = lambda h: subjects_util.expected_oracle(store, snap, h + (100, 1), gmd, cache, memo)[3]
        queries = _with_pages(heads, (1, 2, 100), total_of, ps)
        got = subjects_util.answers(snap.subjects_raw(queries, gmd))
        want_b = subjects_util.expected_two_step(snap, queries, gmd, ps)
        assert len(got) == len(queries)
        for q, g, b in zip(queries, got, want_b):
            a = subjects_util.expected_oracle(store, snap, q, gmd, cache, memo)
            assert g == a, (q, gmd, g, a)
            assert g == b, (q, gmd, g, b)
            seen.add(g[0])
    assert SUBJECTS_NOT_FOUND in seen and seen <= {SUBJECTS_OK, SUBJECTS_NOT_FOUND}
    snap.close()


# ---------------------------------------------------------------------------------- agreement with check
@pytest.mark.parametrize("seed", range(60))
def test_agrees_with_check_at_ample_depth(seed):
    """Without wildcards, poison and visit-key collisions, at global max-depth 32 and request depth 0: the
    subjects returned for every tuple row key are exactly the users check_batch allows on it."""
    import keto_amd
    store, ns, tuples, raw, ps, (names, objs, rels, users) = random_store(seed, allow_wildcards=False, allow_poison=False,
                                                                         allow_collisions=False)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=0)
    keys = sorted({(t.namespace, t.object, t.relation) for t in tuples})
    if keys:
        got = snap.subjects([k + (0, 1000, 0) for k in keys], 32)
        reqs = [k + (("id", u), 0) for k in keys for u in users]
        allowed, status = snap.check_batch(reqs, 32)
        assert not status.any()
        for i, (k, g) in enumerate(zip(keys, got)):
            want = {u for j, u in enumerate(users) if allowed[i * len(users) + j]}
            assert g[0] == SUBJECTS_OK and set(g[1]) == want and g[3] == len(want) and g[2] == "", (k, g, want)
    snap.close()


# ---------------------------------------------------------------------------------- the sort classes' edges
EDGE_LEAVES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 5000)


def _edge_graph():
    """One root r<L> per target id-leaf count L: a direct run of users and four groups g<L>_<k> holding seeded
    random, overlapping subsets of one user pool -- the root's id leaves are several ascending runs, unsorted
    as a whole, with many duplicates.  r0 holds one empty group (a nil child: a subject-set leaf, no id leaf)."""
    rng = random.Random(4242)
    tuples = []
    for L in EDGE_LEAVES:
        root = f"r{L}"
        part = L // 5
        direct = L - 4 * part
        pool = [f"u{i:05d}" for i in range(max(8, L // 2))]
        at = rng.randrange(len(pool) - direct + 1)
        tuples += [T("n", root, "m", SubjectID(u)) for u in pool[at:at + direct]]
        for k in range(4):
            tuples.append(T("n", root, "m", SubjectSet("n", f"g{L}_{k}", "m")))
            tuples += [T("n", f"g{L}_{k}", "m", SubjectID(u)) for u in rng.sample(pool, part)]
    return [(1, "n")], tuples


def run_edges():
    """All roots in one call, shuffled, a NOT_FOUND root and a nil root between them, first and last (empty
    segments on the boundaries); every page at sizes {1, 63, 64, 65, 2^31}; against (B).  The sort classes are
    whatever KETO_SUBJECTS_LDS in the process makes them."""
    import keto_amd
    ns, tuples = _edge_graph()
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), device=0)
    heads = [("n", f"r{L}", "m", 0) for L in EDGE_LEAVES]
    empties = [("nope", "x", "m", 0), ("n", "nothing", "m", 0)]
    trees = dict(zip(heads + empties, subjects_util.expand_nodes(snap, [(("set", n, o, r), d) for n, o, r, d in heads + empties], 5)))
    flat = {h: subjects_util.flatten_nodes(trees[h][1]) for h in heads}
    assert [flat[h][1] for h in heads] == list(EDGE_LEAVES)              # the id-leaf counts are the targets
    assert all(len(flat[h][0]) < L for h, L in zip(heads, EDGE_LEAVES) if L >= 63)   # with duplicates
    rng = random.Random(7)
    n = 0
    for size in (1, 63, 64, 65, 2 ** 31):
        queries = _with_pages(heads, (size,), lambda h: len(flat[h][0]), 100)
        rng.shuffle(queries)
        k = len(queries) // 2
        pad = [e + (size, 1) for e in empties]
        queries = pad + queries[:k] + pad[::-1] + queries[k:] + pad
        got = subjects_util.answers(snap.subjects_raw(queries, 5))
        want = subjects_util.answers_from_trees(trees, queries, 100)
        assert len(got) == len(queries)
        for q, g, w in zip(queries, got, want):
            assert g == w, (q, g[0], g[2:], w[0], w[2:], g[1][:8], w[1][:8])
        assert got[0] == (SUBJECTS_NOT_FOUND, [], "", 0, 0, 0) and got[1] == (SUBJECTS_OK, [], "", 0, 0, 0)
        n += len(queries)
    return n


def test_class_edges():
    assert run_edges() > 3000


def test_class_edges_with_a_small_lds_class():
    """KETO_SUBJECTS_LDS=128: segments of 129 leaves and more take the radix-sorted class."""
    _child("import tests.test_gpu_subjects as t; print('edge queries ok:', t.run_edges())", "edge queries ok:",
           KETO_SUBJECTS_LDS="128")


def run_bad_lds():
    import keto_amd
    snap = keto_amd.Snapshot.build([(1, "n")], [(1, "a", "r", "u")], device=0)
    try:
        snap.subjects([("n", "a", "r", 0, 0, 0)])
    except keto_amd.KetoError as e:
        return f"code {e.code}"
    return "no error"


@pytest.mark.parametrize("value", ["100", "64", "16384", "2048x", ""])
def test_bad_lds_limit_is_an_error(value):
    out = _child("import tests.test_gpu_subjects as t; print('lds:', t.run_bad_lds())", "lds:", KETO_SUBJECTS_LDS=value)
    assert "lds: code -1" in out, out


# ---------------------------------------------------------------------------------- staging regimes
def run_regime():
    """Random expands over quirk-heavy graphs, with whatever staging regime the process has: equal to (B)."""
    import keto_amd
    n = 0
    for seed in range(3400, 3404):
        store, ns, tuples, raw, ps, alph = random_store(seed, wide=seed % 3 == 0)
        snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=0)
        exps = [(s, d, g) for s, d, g in random_expands(seed, alph, k=200) if isinstance(s, SubjectSet)]
        for g in sorted({e[2] for e in exps}):
            queries = [(s.namespace, s.object, s.relation, d, size, page) for s, d, gg in exps if gg == g
                       for size, page in ((0, 0), (1, 2), (2 ** 31, 1))]
            got = subjects_util.answers(snap.subjects_raw(queries, g))
            want = subjects_util.expected_two_step(snap, queries, g, ps)
            assert got == want, (seed, g)
            n += len(queries)
        snap.close()
    return n


@pytest.mark.parametrize("env", ["two_pass", "tiny_regions", "split_chunks", "split_pool_full", "no_chunks"])
def test_staging_regimes(env):
    """The resident arena is produced differently in each regime of tests/test_gpu_expand_encoded.py's table."""
    from tests.test_gpu_expand_encoded import STAGE_ENVS
    _child("import tests.test_gpu_subjects as t; print('regime ok:', t.run_regime())", "regime ok:", **STAGE_ENVS[env])


# ---------------------------------------------------------------------------------- the ids form
def test_ids_form():
    """keto_subjects_batch_ids equals the named form on the same roots; a root with bit 31 clear is
    KETO_E_INVALID and nothing is written to *out."""
    import ctypes as C
    import keto_amd
    ns, tuples = _edge_graph()
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), device=0)
    n_rows = snap.stats()["n_rows"]
    rows = np.arange(n_rows, dtype=np.uint32)
    keys = snap.subject_fields(rows | SET)
    rng = np.random.default_rng(5)
    depths = rng.integers(0, 4, size=n_rows).astype(np.int32)
    sizes = rng.choice(np.array([0, 1, 7, 2 ** 31], dtype=np.uint32), size=n_rows)
    pages = rng.integers(0, 3, size=n_rows).astype(np.uint32)
    by_id = subjects_util.answers(snap.subjects_ids_raw(rows | SET, depths, sizes, pages, 5))
    named = subjects_util.answers(snap.subjects_raw([(k[1], k[2], k[3], int(d), int(s), int(p))
                                                     for k, d, s, p in zip(keys, depths, sizes, pages)], 5))
    assert by_id == named and any(g[1] for g in by_id)
    one = lambda v, t: (t * 2)(*v)
    out = C.c_void_p(0x1234)
    rc = snap.lib.keto_subjects_batch_ids(snap.h, one([int(rows[0]) | 0x80000000, 3], C.c_uint32), one([0, 0], C.c_int32),
                                          one([0, 0], C.c_uint32), one([0, 0], C.c_uint32), C.c_uint32(2), C.c_int32(5),
                                          C.byref(out))
    assert rc == KETO_E_INVALID and out.value == 0x1234
    with pytest.raises(keto_amd.KetoError) as e:                           # a row out of range, as for the expand
        snap.subjects_ids_raw(np.array([n_rows], dtype=np.uint32) | SET, [0], [0], [0])
    assert e.value.code == KETO_E_INVALID
    empty = snap.subjects_raw([])
    assert len(empty["status"]) == 0 and empty["offsets"].tolist() == [0] and len(empty["ids"]) == 0
    snap.close()


# ---------------------------------------------------------------------------------- after writes
def test_after_writes_and_results_outlive_the_snapshot():
    """An apply adds a brand-new user under a group: its string id is the largest, so it sorts last although
    its bytes sort first.  A delete by query follows.  The answers match (A) after each step; a result taken
    before the write reads the same after it and after the snapshot is closed."""
    import keto_amd
    ns = [(1, "docs"), (2, "grp")]
    eng = SubjectSet("grp", "eng", "member")
    tuples = [T("docs", "a", "view", SubjectID("bob")), T("docs", "a", "view", eng), T("grp", "eng", "member", SubjectID("carol")),
              T("grp", "eng", "member", SubjectID("dave")), T("docs", "b", "view", SubjectSet("grp", "ops", "member")),
              T("grp", "ops", "member", eng), T("grp", "ops", "member", SubjectID("bob"))]
    store = SQLStore(ns, tuples, page_size=2)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), page_size=2, device=0)
    heads = [(n, o, r, d) for n, o, r in (("docs", "a", "view"), ("docs", "b", "view"), ("grp", "eng", "member"),
                                          ("grp", "ops", "member"), ("docs", "", "view")) for d in (0, 1, 2, 3)]

    def sweep():
        cache, memo = {}, {}
        total_of = lambda h: subjects_util.expected_oracle(store, snap, h + (100, 1), 5, cache, memo)[3]
        queries = _with_pages(heads, (0, 1, 100), total_of, 2)
        got = subjects_util.answers(snap.subjects_raw(queries, 5))
        for q, g in zip(queries, got):
            assert g == subjects_util.expected_oracle(store, snap, q, 5, cache, memo), q
        return snap.subjects([h + (100, 0) for h in heads], 5)

    before = sweep()
    assert before[0][1] == ["bob", "carol", "dave"]
    held = snap.subjects_handle([h + (100, 0) for h in heads], 5)
    held_before = snap._subjects_arrays(held)
    ins = [T("grp", "eng", "member", SubjectID("aaa-new")), T("docs", "a", "view", SubjectID("zed"))]
    v0 = snap.version()
    assert snap.apply([rows_from_tuples(ns, [t])[0] for t in ins], []) == v0 + 1
    for t in ins:
        store.insert(t)
    after = sweep()
    assert after[0][1] == ["bob", "carol", "dave", "aaa-new", "zed"]        # string-id order: new strings last
    assert after[4][1] == ["bob", "carol", "dave", "aaa-new"]                # docs:b through ops -> eng
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in ("status", "offsets", "ids", "next_page", "totals", "leaves"))
    assert same(snap._subjects_arrays(held), held_before)
    assert [f[1] for f in snap.subject_fields(held_before["ids"][:3])] == ["bob", "carol", "dave"]
    q = ("grp", "eng", "", SubjectID("carol"))
    n_del, _ = delete_util.sql_delete(store, *q)
    assert snap.delete_query(*delete_util.request(q))["deleted"] == n_del == 1
    last = sweep()
    assert last[0][1] == ["bob", "dave", "aaa-new", "zed"]
    assert same(snap._subjects_arrays(held), held_before)
    lib = snap.lib
    snap.close()
    assert lib.keto_subjects_count(held) == len(heads)
    assert same(snap._subjects_arrays(held), held_before)                  # (reads the handle alone)
    lib.keto_subjects_free(held)


# ---------------------------------------------------------------------------------- partitions
def test_parts():
    """A 2-part shared-rows upload answers the roots this part owns and the roots every part holds as the
    replicated snapshot does, and refuses the other part's; a migrating part refuses the call."""
    from keto_amd.capi import PART_MIGRATE, KetoError
    from tools import synth
    g = synth.SynthGraph(synth.scaled(synth.POWERLAW_1B, 1 / 4096), threads=16)
    full = g.snapshot(device=0)
    rng = np.random.default_rng(52)
    rows = rng.integers(0, g.n_rows, size=2000).astype(np.uint32)
    own = full.row_owner(rows, 2)
    depths = rng.integers(-1, 7, size=len(rows)).astype(np.int32)
    sizes = rng.choice(np.array([0, 1, 3, 2 ** 31], dtype=np.uint32), size=len(rows))
    pages = rng.integers(0, 3, size=len(rows)).astype(np.uint32)
    part = g.snapshot_part(0, 2, device=0)
    assert (own == 0).any() and (own < 0).any() and (own == 1).any()
    for mine in (own == 0, own < 0):
        args = (rows[mine] | SET, depths[mine], sizes[mine], pages[mine], 5)
        got, want = subjects_util.answers(part.subjects_ids_raw(*args)), subjects_util.answers(full.subjects_ids_raw(*args))
        assert got == want and any(g_[1] for g_ in got)
    other = rows[own == 1][:4] | SET
    zeros = np.zeros(len(other), dtype=np.uint32)
    with pytest.raises(KetoError) as err:
        part.subjects_ids_raw(other, zeros.astype(np.int32), zeros, zeros, 5)
    assert err.value.code == KETO_E_INVALID
    del part
    mig = g.snapshot_part(0, 2, device=0, mode=PART_MIGRATE)
    with pytest.raises(KetoError) as err:
        mig.subjects_ids_raw(np.array([0], dtype=np.uint32) | SET, [0], [0], [0], 5)
    assert err.value.code == KETO_E_INVALID and "migrating" in str(err.value)


# ---------------------------------------------------------------------------------- two threads
def test_two_threads():
    """Two threads on one snapshot, 20 calls each: one keto_subjects_batch, the other keto_expand_encode_batch
    (both keep the expand's arena on the device).  Every result equals the single-threaded one."""
    import keto_amd
    ns, tuples = _edge_graph()
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), device=0)
    queries = [("n", f"r{L}", "m", 0, size, 1) for L in EDGE_LEAVES for size in (3, 2 ** 31)] + [("nope", "x", "m", 0, 0, 0)]
    reqs = [(("set", "n", f"r{L}", "m"), 3) for L in EDGE_LEAVES[::-1]]
    want_s = snap.subjects(queries, 5)
    want_e = [x.tolist() if hasattr(x, "tolist") else x for x in snap.expand_batch_encoded(reqs, 5, "json")]
    words = subjects_util.expected_two_step(snap, queries, 5, 100)          # (string ids; want_s holds the strings)
    assert [(g[0], len(g[1])) + g[2:] for g in want_s] == [(w[0], len(w[1])) + w[2:] for w in words]
    results, errors = {"s": [], "e": []}, []

    def flatten():
        try:
            for _ in range(20):
                results["s"].append(snap.subjects(queries, 5))
        except Exception as e:                                              # reported by the main thread
            errors.append(e)

    def encode():
        try:
            for _ in range(20):
                results["e"].append([x.tolist() if hasattr(x, "tolist") else x for x in snap.expand_batch_encoded(reqs, 5, "json")])
        except Exception as e:
            errors.append(e)

    ts = [threading.Thread(target=flatten), threading.Thread(target=encode)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert len(results["s"]) == len(results["e"]) == 20
    assert all(r == want_s for r in results["s"]) and all(r == want_e for r in results["e"])
    snap.close()
