"""keto_lookup_objects_batch on the GPU against one SubjectIsAllowed per candidate object on the SQL oracle
(tests/lookup_util.py): random graphs with every depth, global depth and page, tile / wave / chunk / window
edges at unaligned candidate offsets (KETO_LIST_TILE=256, KETO_LOOKUP_CHUNK=128), unsupported queries and batch
independence, lookups after writes and after a delete by query, the candidate cap, a deep chain through the
reach pretest, and KETO_LOOKUP_UNDECIDED on the nested synthetic graph with the check's tiers shrunk."""
import itertools
import os
import random
import subprocess
import sys

import pytest

from oracle.oracle_sql import RelationTuple, SQLStore, SubjectID, SubjectSet
from tests import delete_util, lookup_util
from tests.engine_util import rows_from_tuples
from tests.lookup_util import LOOKUP_OK, LOOKUP_UNDECIDED, LOOKUP_UNKNOWN_NAMESPACE, LOOKUP_UNSUPPORTED
from tests.randgraph import random_store

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = RelationTuple


def _all_pages(store, heads, sizes, gmd, cache):
    """heads: (namespace, relation, subject, depth) -> every page of each at every size, one past the last."""
    out = []
    for (ns, rel, sub, depth), size in itertools.product(heads, sizes):
        total = lookup_util.expected(store, (ns, rel, sub, depth, size, 1), gmd, cache)[3]
        last = lookup_util.last_page(total, size if size else store.page_size)
        out += [(ns, rel, sub, depth, size, page) for page in range(1, last + 2)]
    return out


def _compare(snap, store, queries, gmd=5, cache=None, allow=(LOOKUP_OK, LOOKUP_UNKNOWN_NAMESPACE)):
    """One lookup call for `queries` (lookup_util form); every answer equals the oracle's."""
    cache = {} if cache is None else cache
    got = snap.lookup_objects([lookup_util.to_request(q) for q in queries], gmd)
    assert len(got) == len(queries)
    for q, g in zip(queries, got):
        want = lookup_util.expected(store, q, gmd, cache)
        assert g[0] in allow, (q, g)
        assert g == want, (q, gmd, g, want)
    return got


# ---------------------------------------------------------------------------------- random parity
@pytest.mark.parametrize("seed", range(60))
def test_random_parity(seed):
    """Every (namespace, relation) of the alphabet plus an unknown namespace, users and fully named subject
    sets, request depths {0, 1, 2, 5, 7}, every page at sizes {1, 2, 100}, at each global max-depth of
    {1, 3, 5}: one batch call per seed and global max-depth (a call has one).  A namespace literally named ""
    is left out as a query namespace and as a subject set's: both are wildcard forms."""
    import keto_amd
    store, ns, tuples, raw, ps, (names, objs, rels, users) = random_store(seed)
    rng = random.Random(seed * 977 + 11)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=0)
    named = [n for n in names if n != ""]
    stored = [t.subject for t in tuples if isinstance(t.subject, SubjectSet)
              and t.subject.namespace != "" and t.subject.object != "" and t.subject.relation != ""]
    subjects = [SubjectID(u) for u in rng.sample(users, min(2, len(users)))] + rng.sample(stored, min(2, len(stored)))
    if named:
        subjects.append(SubjectSet(rng.choice(named), rng.choice(objs), rng.choice(rels)))
    keys = list(itertools.product(named + ["nope"], rels))
    heads = [(n, r, s, d) for (n, r), s, d in itertools.product(keys, subjects, (0, 1, 2, 5, 7))]
    for gmd in (1, 3, 5):
        cache = {}
        queries = _all_pages(store, heads, (1, 2, 100), gmd, cache)
        got = _compare(snap, store, queries, gmd, cache)
        assert {g[0] for g in got} == ({LOOKUP_OK, LOOKUP_UNKNOWN_NAMESPACE} if named else {LOOKUP_UNKNOWN_NAMESPACE})
        # the same objects are a filter over check_batch on the candidates
        full = {(q[0], q[1], q[2], q[3]): g for q, g in zip(queries, got) if q[4] == 100 and q[5] == 1}
        reqs, owner = [], []
        for (n, r, s, d), g in full.items():
            if g[0] != LOOKUP_OK:
                continue
            for o in lookup_util.candidates(store, n, r):
                reqs.append((n, o, r, lookup_util.subject_key(s), d))
                owner.append(((n, r, s, d), o))
        if reqs:
            allowed, status = snap.check_batch(reqs, gmd)
            assert not status.any()
            kept = {}
            for (head, o), a in zip(owner, allowed):
                if a:
                    kept.setdefault(head, []).append(o)
            for head, g in full.items():
                if g[0] == LOOKUP_OK:
                    assert g[1] == kept.get(head, []) and g[3] == len(g[1]), head
    snap.close()


# ---------------------------------------------------------------------------------- tile / wave / chunk / window edges
N_OBJ = 600


def _edge_graph():
    """docs:oNNNN#view for 600 objects: every third granted to u directly, every fifth through two groups
    (g1 -> g2 -> u), the rest to somebody else.  280 of them are u's."""
    ns = [(1, "docs"), (2, "grp")]
    tuples = [T("grp", "g1", "m", SubjectSet("grp", "g2", "m")), T("grp", "g2", "m", SubjectID("u"))]
    for i in range(N_OBJ):
        o = f"o{i:04d}"
        if i % 3 == 0:
            tuples.append(T("docs", o, "view", SubjectID("u")))
        if i % 5 == 0:
            tuples.append(T("docs", o, "view", SubjectSet("grp", "g1", "m")))
        if i % 3 and i % 5:
            tuples.append(T("docs", o, "view", SubjectID(f"x{i}")))
    return ns, tuples


def run_edges():
    """Every page at the edge sizes, with whatever KETO_LIST_TILE / KETO_LOOKUP_CHUNK the process has.  Each
    call begins and ends with a second query (grp#m: 2 candidates) whose subject the snapshot does not know:
    in front it puts every 600-candidate query at an offset of 2 modulo 4, so the tiles, quarter-waves and
    4-byte decision words start unaligned; behind, its own candidates start mid-chunk."""
    import keto_amd
    ns, tuples = _edge_graph()
    store = SQLStore(ns, tuples)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), device=0)
    u = SubjectID("u")
    cache = {}
    want_all = [f"o{i:04d}" for i in range(N_OBJ) if i % 3 == 0 or i % 5 == 0]
    assert lookup_util.expected(store, ("docs", "view", u, 0, 2 ** 31, 1), 5, cache) == (LOOKUP_OK, want_all, "", 280, N_OBJ, 0)
    tail = ("grp", "m", SubjectID("zz-unknown"), 0, 0, 0)
    n = 0
    for size in (1, 63, 64, 65, 127, 128, 129, 600, 2 ** 31):
        queries = [tail] + _all_pages(store, [("docs", "view", u, 0)], (size,), 5, cache) + [tail]
        got = _compare(snap, store, queries, 5, cache, allow=(LOOKUP_OK,))
        assert got[0] == got[-1] == (LOOKUP_OK, [], "", 0, 2, 0)
        assert sum((g[1] for g in got), []) == want_all
        n += len(queries)
    # request depth 2 stops one hop short of the groups' grant: only the direct third is left
    got = _compare(snap, store, [("docs", "view", u, 2, 600, 1), tail, ("docs", "view", u, 3, 600, 1)], 5, cache)
    assert got[0][3] == 200 and got[2][3] == 280
    return n


def test_tile_wave_chunk_and_window_edges():
    env = dict(os.environ, KETO_LIST_TILE="256", KETO_LOOKUP_CHUNK="128")
    code = "import tests.test_gpu_lookup as t; print('edge queries ok:', t.run_edges())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "edge queries ok:" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_bad_chunk_is_an_error():
    env = dict(os.environ, KETO_LOOKUP_CHUNK="7")
    code = ("import keto_amd\n"
            "s = keto_amd.Snapshot.build([(1, 'n')], [(1, 'a', 'r', 'u')], device=0)\n"
            "try:\n    s.lookup_objects([('n', 'r', ('id', 'u'), 0, 0, 0)])\nexcept keto_amd.KetoError as e:\n    print('code', e.code)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "code -1" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------- unsupported inputs, batch independence
def test_unsupported_inputs_and_batch_independence():
    import keto_amd
    store, ns, tuples, raw, ps, (names, objs, rels, users) = random_store(4321, n_tuples=40, allow_wildcards=False)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=0)
    rng = random.Random(17)
    stored = [t.subject for t in tuples if isinstance(t.subject, SubjectSet)]
    subs = [SubjectID(u) for u in users] + stored[:3] + [SubjectSet("nope", "a", "r"), SubjectID("zz-unknown")]
    good = [(rng.choice(names + ["nope"]), rng.choice(rels + ["zz-unknown"]), rng.choice(subs), rng.choice([0, 1, 2, 5]),
             rng.choice([0, 1, 2, 7]), rng.randrange(0, 4)) for _ in range(200)]
    n0, r0, u0 = names[0], rels[0], SubjectID(users[0])
    bad = [("", r0, u0, 0, 0, 0), (n0, "", u0, 0, 0, 0), ("", "", u0, 0, 0, 0),
           (n0, r0, SubjectSet("", objs[0], r0), 0, 0, 0), (n0, r0, SubjectSet(n0, "", r0), 0, 0, 0),
           (n0, r0, SubjectSet(n0, objs[0], ""), 0, 0, 0), ("nope", "", u0, 0, 0, 0)]
    queries = good[:]
    for k, b in enumerate(bad):
        queries.insert(3 + 29 * k, b)
    together = snap.lookup_objects([lookup_util.to_request(q) for q in queries], 5)
    cache = {}
    for q, t in zip(queries, together):
        if q in bad:
            assert t == (LOOKUP_UNSUPPORTED, [], "", 0, 0, 0), (q, t)
        else:
            assert t == lookup_util.expected(store, q, 5, cache), (q, t)
            assert snap.lookup_objects([lookup_util.to_request(q)], 5) == [t], q
    assert {t[0] for t in together} == {LOOKUP_OK, LOOKUP_UNKNOWN_NAMESPACE, LOOKUP_UNSUPPORTED}
    assert any(t[1] for t in together)
    # a batch of unsupported queries alone, and an empty batch
    assert snap.lookup_objects([lookup_util.to_request(b) for b in bad], 5) == [(LOOKUP_UNSUPPORTED, [], "", 0, 0, 0)] * len(bad)
    raw_out = snap.lookup_objects_raw([])
    assert len(raw_out["status"]) == 0 and list(raw_out["offsets"]) == [0] and len(raw_out["rows"]) == 0
    assert snap.lookup_objects([]) == []


def test_partitioned_snapshot_is_invalid():
    import keto_amd
    ns = [(1, "n")]
    rows = [(1, "a", "r", "u"), (1, "b", "r", None, 1, "a", "r")]
    part = keto_amd.Snapshot.build(ns, rows, device=-1).upload_part(0, 2, device=0)
    with pytest.raises(keto_amd.KetoError) as e:
        part.lookup_objects([("n", "r", ("id", "u"), 0, 0, 0)])
    assert e.value.code == -1                                   # KETO_E_INVALID
    snap = keto_amd.Snapshot.build(ns, rows, device=0)
    assert snap.lookup_objects([("n", "r", ("id", "u"), 0, 0, 0)]) == [(LOOKUP_OK, ["a", "b"], "", 2, 2, 0)]


# ---------------------------------------------------------------------------------- after writes
def test_lookups_after_writes_and_delete_query():
    import keto_amd
    ns = [(1, "docs"), (2, "grp")]
    eng = SubjectSet("grp", "eng", "member")
    tuples = [T("docs", "a", "view", SubjectID("alice")), T("docs", "b", "view", eng), T("grp", "eng", "member", SubjectID("alice")),
              T("docs", "c", "view", SubjectSet("grp", "ops", "member")), T("grp", "ops", "member", eng),
              T("docs", "d", "view", SubjectID("bob")), T("docs", "e", "edit", SubjectID("alice"))]
    store = SQLStore(ns, tuples, page_size=2)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), page_size=2, device=0)
    subjects = [SubjectID("alice"), SubjectID("bob"), SubjectID("carol"), eng]
    heads = [(n, r, s, d) for n, r in (("docs", "view"), ("docs", "edit"), ("grp", "member")) for s in subjects for d in (0, 1, 2)]

    def sweep():
        cache = {}
        return _compare(snap, store, _all_pages(store, heads, (0, 1, 100), 5, cache), 5, cache, allow=(LOOKUP_OK,))

    got = sweep()
    assert any(g[1] == ["a", "b", "c"] for g in got)
    info0 = snap.list_index_info()
    assert info0["dev_current"] == 1

    # a grant (bob on b), a revoke (alice's direct grant on a), a new object row between existing ones (bb), a
    # new member (carol in eng: every object reached through eng is hers now)
    ins = [T("docs", "b", "view", SubjectID("bob")), T("docs", "bb", "view", SubjectID("alice")), T("grp", "eng", "member", SubjectID("carol"))]
    dels = [T("docs", "a", "view", SubjectID("alice"))]
    v0 = snap.version()
    assert snap.apply([rows_from_tuples(ns, [t])[0] for t in ins], [rows_from_tuples(ns, [t])[0] for t in dels]) == v0 + 1
    for t in ins:
        store.insert(t)
    for t in dels:
        store.delete(t)
    got = sweep()
    info1 = snap.list_index_info()
    assert info1["dev_current"] == 1 and info1["dev_patches"] == info0["dev_patches"] + 1      # the journal patch
    assert info1["dev_builds"] == info0["dev_builds"]
    full = {(q[2], q[3]): g[1] for q, g in zip(_all_pages(store, heads, (0, 1, 100), 5, {}), got)
            if q[:2] == ("docs", "view") and q[4] == 100 and q[5] == 1}
    assert full[(SubjectID("alice"), 0)] == ["b", "bb", "c"] and full[(SubjectID("carol"), 0)] == ["b", "c"]
    assert full[(SubjectID("bob"), 0)] == ["b", "d"]

    # delete by query: every view tuple of b; then the eng group's members
    for q in (("docs", "b", "view", None), ("grp", "eng", "", SubjectID("alice"))):
        n_del, _ = delete_util.sql_delete(store, *q)
        assert snap.delete_query(*delete_util.request(q))["deleted"] == n_del > 0
        got = sweep()
    assert not any("b" in g[1] for g in got)


# ---------------------------------------------------------------------------------- candidate cap
def run_cap():
    import keto_amd
    ns, tuples = _edge_graph()
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), device=0)
    u = ("id", "u")
    try:
        snap.lookup_objects([("docs", "view", u, 0, 0, 0)])
        return "no error"
    except keto_amd.KetoError as e:
        code = e.code
    # under the cap the same snapshot answers: grp#m has 2 candidates; 50 such queries are 100
    small = snap.lookup_objects([("grp", "m", u, 0, 0, 0)] * 50)
    assert small == [(LOOKUP_OK, ["g1", "g2"], "", 2, 2, 0)] * 50, small[:2]
    try:
        snap.lookup_objects([("grp", "m", u, 0, 0, 0)] * 51)
        return "no error at 102"
    except keto_amd.KetoError as e:
        assert e.code == code
    return f"code {code}"


def test_candidate_cap():
    env = dict(os.environ, KETO_LOOKUP_MAX_CANDIDATES="100")
    code = "import tests.test_gpu_lookup as t; print('cap:', t.run_cap())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cap: code -1" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------- undecided
UNDECIDED_ENV = {"KETO_T0_CAP": "256", "KETO_T1_CAP": "1024", "KETO_NO_POOL": "1", "KETO_TEST_T2_FRAMES": "3"}


def run_undecided():
    """The nested synthetic graph of tests/test_gpu_host_api.py (2^14 groups in chains of up to 32) with its
    strings, under the knobs that test uses to shrink the check's tiers (tier-0 / tier-1 tables of 256 / 1024
    entries without the borrowing pool, a tier-2 stack of 3 frames), at global max-depth 40: for four users at request depths 0, 16 and 1
    (direct members only: never undecided),
    groups#member over all 16K group rows, against keto_check_batch_rows on the same rows and subject."""
    import numpy as np
    from keto_amd.capi import CHECK_IDS_DTYPE, UNDECIDED
    from tools import synth
    g = synth.SynthGraph(dict(n_docs=0, n_folders=0, n_groups=1 << 14, n_users=1 << 14, target_edges=0, seed=3),
                         threads=16, kind="nested", chain=32)
    u = g.unified(threads=16)
    snap = g.snapshot_unified(u, device=0)
    targets = g.queries_nested(4, seed=91, depths=(0,))["target"]
    users = [f"u{int(t):08x}" for t in targets]
    words = [p["subject"] for p in snap.list_plan([("", "", "", ("id", x), 0, 0) for x in users])]
    assert words == [int(t) + u.user_base for t in targets]
    rows = snap.list_batch_raw([("groups", "", "member", None, 2 ** 31 - 1, 0)])[2]["row"]
    rows = rows[np.r_[True, rows[1:] != rows[:-1]]]                # key order; a row's tuples follow one another
    assert len(rows) > 16000
    queries = [("groups", "member", ("id", x), d, 2 ** 31 - 1, 0) for d in (0, 16, 1) for x in users]
    r = snap.lookup_objects_raw(queries, 40)
    n_und = n_ok = 0
    for i, (_, _, _, d, _, _) in enumerate(queries):
        ids = np.zeros(len(rows), dtype=CHECK_IDS_DTYPE)
        ids["row"], ids["target"], ids["max_depth"] = rows, words[i % len(users)], d
        dec = snap.check_batch_rows(ids, 40)
        und = int((dec == UNDECIDED).sum())
        got = r["rows"][int(r["offsets"][i]):int(r["offsets"][i + 1])]
        assert int(r["candidates"][i]) == len(rows) and int(r["undecided"][i]) == und, (i, und, r["undecided"])
        if und:
            assert r["status"][i] == LOOKUP_UNDECIDED and len(got) == 0 and r["totals"][i] == 0 and r["next_page"][i] == 0, i
            n_und += 1
        else:
            assert r["status"][i] == LOOKUP_OK and np.array_equal(got, rows[dec == 1]) and r["totals"][i] == len(got), i
            n_ok += 1
    assert n_und >= 1 and n_ok >= 1, (n_und, n_ok, r["undecided"].tolist())
    return f"undecided queries {n_und}, decided queries {n_ok}, undecided checks {r['undecided'].tolist()}"


def test_undecided_candidates_fail_their_query():
    """KETO_LOOKUP_UNDECIDED: no rows, total 0, and `undecided` equal to the KETO_UNDECIDED decisions of
    keto_check_batch_rows on the same candidates; a query of the batch without one is answered."""
    env = dict(os.environ, **UNDECIDED_ENV)
    code = "import tests.test_gpu_lookup as t; print('undecided ok:', t.run_undecided())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "undecided ok:" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------- deep path
def test_deep_chain_through_the_reach_pretest():
    """A nested-group chain c00 -> c01 -> ... -> c11 -> u and 40 objects that enter it at every link, at global
    max-depth 32 (past 9 the check splits top-level items and pretests reachability): an object entering at
    link k needs depth 13 - k."""
    import keto_amd
    ns = [(1, "docs"), (2, "grp")]
    links = 12
    tuples = [T("grp", f"c{k:02d}", "m", SubjectSet("grp", f"c{k + 1:02d}", "m")) for k in range(links - 1)]
    tuples.append(T("grp", f"c{links - 1:02d}", "m", SubjectID("u")))
    for i in range(40):
        tuples.append(T("docs", f"o{i:02d}", "view", SubjectSet("grp", f"c{i % links:02d}", "m")))
        if i % 7 == 0:
            tuples.append(T("docs", f"o{i:02d}", "view", SubjectID("w")))
    store = SQLStore(ns, tuples)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), device=0)
    u, w, mid = SubjectID("u"), SubjectID("w"), SubjectSet("grp", "c06", "m")
    cache = {}
    heads = [("docs", "view", s, d) for s in (u, w, mid, SubjectID("nobody")) for d in (0, 5, 12, 13, 40)]
    got = _compare(snap, store, _all_pages(store, heads, (7, 100), 32, cache), 32, cache, allow=(LOOKUP_OK,))
    by_head = {(q[2], q[3]): g for q, g in zip(_all_pages(store, heads, (7, 100), 32, cache), got) if q[4] == 100 and q[5] == 1}
    assert by_head[(u, 0)][3] == 40 and by_head[(u, 13)][3] == 40
    assert by_head[(u, 12)][1] == [f"o{i:02d}" for i in range(40) if i % links]        # entering at c00 needs 13
    assert by_head[(u, 5)][1] == [f"o{i:02d}" for i in range(40) if 13 - i % links <= 5]
    assert by_head[(w, 0)][1] == [f"o{i:02d}" for i in range(40) if i % 7 == 0]
    assert by_head[(mid, 0)][1] == [f"o{i:02d}" for i in range(40) if i % links <= 6]
    assert snap.last_timing_full()["items"] > 0                                            # the item split ran
