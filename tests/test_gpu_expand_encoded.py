"""keto_expand_encode_batch[_ids]: roots in, encoded trees out, the node arena never leaving the device.

The yardstick is never the fused call itself: keto_expand_batch[_ids] + keto_tree_status + the host
encoders keto_tree_proto_all / keto_tree_json_all, which the rest of the suite pins to the oracle.
Statuses, offsets and bytes are compared for equality, for both encodings, in every case.

KETO_EXPAND_UNDECIDED: no environment switch forces an undecided expand root at small size (the last
tier's stack is sized from the snapshot's own depth bound, and KETO_TEST_T2_FRAMES is read by the
check path only), so no case here holds one; device_expand refuses, for this form, a root that is
not a tree and yet has nodes.
"""
import ctypes as C
import os
import random
import threading

import numpy as np
import pytest

from tests.engine_util import rows_from_tuples, subj
from tests.randgraph import random_expands, random_store

pytestmark = pytest.mark.gpu

KETO_E_INVALID = -1
ENCODINGS = ("json", "proto")
SET = np.uint32(0x80000000)


def _snapshot(namespaces, rows, page_size=100):
    import keto_amd
    return keto_amd.Snapshot.build(namespaces, rows, page_size=page_size, device=0)


def _two_step(snap, reqs, g):
    """{"json" / "proto": (statuses, offsets, bytes)} of keto_expand_batch + keto_tree_status + the host
    encoders."""
    from keto_amd import capi
    keep = capi._Keep()
    n = len(reqs)
    a = C.c_void_p()
    capi._check(snap.lib.keto_expand_batch(snap.h, snap._expand_reqs(keep, reqs), C.c_uint32(n), C.c_int32(g), C.byref(a)))
    try:
        status = [snap.lib.keto_tree_status(a, C.c_uint32(i)) for i in range(n)]
        j_offs, j_raw, _ = snap._json_all_raw(a, n, device=False)
        p_offs, p_raw, _ = snap._proto_all(a, n, device=False)
    finally:
        snap.lib.keto_tree_arena_free(a)
    return {"json": (status, j_offs.tolist(), j_raw), "proto": (status, p_offs.tolist(), p_raw)}


def _two_step_ids(snap, roots, depths, g):
    st, j_offs, j_raw, _, _ = snap.expand_batch_ids_json(roots, depths, g, device=False)
    st2, p_offs, p_raw, _, _ = snap.expand_batch_ids_proto(roots, depths, g, device=False)
    assert st.tolist() == st2.tolist()
    return {"json": (st.tolist(), j_offs.tolist(), j_raw), "proto": (st.tolist(), p_offs.tolist(), p_raw)}


def _fused(snap, reqs, g, enc):
    st, offs, raw = snap.expand_batch_encoded(reqs, g, enc)
    return st.tolist(), offs.tolist(), raw


def _fused_ids(snap, roots, depths, g, enc):
    st, offs, raw = snap.expand_batch_ids_encoded(roots, depths, g, enc)
    return st.tolist(), offs.tolist(), raw


def _same(snap, reqs, g, what=None):
    """The fused call equals the two-step path for both encodings; returns the two-step results."""
    want = _two_step(snap, reqs, g)
    for enc in ENCODINGS:
        got = _fused(snap, reqs, g, enc)
        assert got[0] == want[enc][0], (what, enc)
        assert got[1] == want[enc][1], (what, enc)
        assert got[2] == want[enc][2], (what, enc)
    return want


def _texts(res):
    _, offs, raw = res
    return [raw[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


# ---------------------------------------------------------------- 1. random graphs
@pytest.mark.parametrize("seed", range(2400, 2420))
def test_random_graphs(seed):
    """Quirk-heavy random graphs: wildcard roots answered by batch-local rows, subject ids the snapshot
    does not know, empty fields, a namespace named "", collisions."""
    store, ns, tuples, raw, ps, alph = random_store(seed, wide=seed % 3 == 0)
    snap = _snapshot(ns, rows_from_tuples(ns, tuples, raw), ps)
    exps = random_expands(seed, alph, k=24)
    for g in sorted({e[2] for e in exps}):
        _same(snap, [(subj(s), d) for s, d, gg in exps if gg == g], g, (seed, g))


# ---------------------------------------------------------------- 2. staging regimes
# (the values of tests/test_gpu_parity.py's STAGE_ENVS)
STAGE_ENVS = {
    "two_pass": {"KETO_EXPAND_STAGE": "0"},
    "tiny_regions": {"KETO_EXPAND_STAGE": "3"},
    "split_chunks": {"KETO_EXPAND_STAGE": "3", "KETO_EXPAND_OVF_CHUNK": "40"},
    "split_pool_full": {"KETO_EXPAND_STAGE": "8", "KETO_SLOTS": "256", "KETO_EXPAND_OVF_CHUNK": "64",
                        "KETO_EXPAND_OVF_NODES": "256"},
    "no_chunks": {"KETO_EXPAND_STAGE": "5", "KETO_EXPAND_OVF_NODES": "0"},
}


@pytest.mark.parametrize("env", sorted(STAGE_ENVS))
@pytest.mark.parametrize("seed", range(3400, 3406))
def test_staging_regimes(monkeypatch, env, seed):
    """The two-pass form (handles_to_rows_direct) and the spilling regimes (handles_to_rows_ranges,
    copy_stage_pieces): the overlay and root fix-ups compose with each."""
    for k, v in STAGE_ENVS[env].items():
        monkeypatch.setenv(k, v)
    store, ns, tuples, raw, ps, alph = random_store(seed, wide=seed % 3 == 0)
    snap = _snapshot(ns, rows_from_tuples(ns, tuples, raw), ps)
    exps = random_expands(seed, alph, k=200)
    for g in sorted({e[2] for e in exps}):
        _same(snap, [(subj(s), d) for s, d, gg in exps if gg == g], g, (env, seed, g))


# ---------------------------------------------------------------- 3. overlay and unknown-id roots
def test_hand_made_overlay_and_unknown_id_roots():
    """One batch: a set root with an empty object and one with an empty relation (wildcard queries,
    answered by batch-local rows), a subject id the snapshot does not know, an ordinary tree, a nil
    root, an unknown namespace."""
    from keto_amd.capi import EXPAND_NIL, EXPAND_NOT_FOUND, EXPAND_TREE
    ns = [(1, "n")]
    snap = _snapshot(ns, [(1, "doc", "view", "alice"), (1, "doc2", "edit", "bob"),
                          (1, "team", "member", None, 1, "doc", "view")])
    reqs = [(("set", "n", "", "view"), 2), (("set", "n", "doc2", ""), 2), (("id", "nobody"), 2),
            (("set", "n", "team", "member"), 3), (("set", "n", "nothing", "here"), 3), (("set", "nope", "x", "y"), 3)]
    want = _same(snap, reqs, 5)
    assert want["json"][0] == [EXPAND_TREE] * 4 + [EXPAND_NIL, EXPAND_NOT_FOUND]
    got = _texts(_fused(snap, reqs, 5, "json"))
    assert got[0] == (b'{"type":"union","children":[{"type":"leaf","subject_id":"alice"}],'
                      b'"subject_set":{"namespace":"n","object":"","relation":"view"}}')
    assert got[1] == (b'{"type":"union","children":[{"type":"leaf","subject_id":"bob"}],'
                      b'"subject_set":{"namespace":"n","object":"doc2","relation":""}}')
    assert got[2] == b'{"type":"leaf","subject_id":"nobody"}'
    assert got[3].startswith(b'{"type":"union"') and b'"alice"' in got[3]
    assert got[4:] == [b"null", b""]
    assert _texts(_fused(snap, reqs, 5, "proto"))[4:] == [b"", b""]


# ---------------------------------------------------------------- 4. shapes
@pytest.fixture(scope="module")
def shapes():
    """One snapshot: a 3,000-member hub; `top` = a, g2{u1, u2}, b, deep{deeper{...}}, c."""
    ns = [(1, "n")]
    rows = [(1, "hub", "m", f"u{i:04d}") for i in range(3000)]
    rows += [(1, "top", "m", "a"), (1, "top", "m", None, 1, "g2", "m"), (1, "top", "m", "b"),
             (1, "top", "m", None, 1, "deep", "m"), (1, "top", "m", "c"),
             (1, "g2", "m", "u1"), (1, "g2", "m", "u2"),
             (1, "deep", "m", None, 1, "deeper", "m"), (1, "deeper", "m", "z")]
    return _snapshot(ns, rows)


TREE_ROOTS = [(("set", "n", "top", "m"), 3), (("set", "n", "g2", "m"), 2), (("id", "someone"), 2),
              (("set", "n", "top", "m"), 2), (("set", "n", "deep", "m"), 4)]
HUB = (("set", "n", "hub", "m"), 2)
NIL = (("set", "n", "nothing", "m"), 3)                  # no tuples: a nil tree
NOT_FOUND = (("set", "nope", "x", "y"), 3)               # unknown namespace


def _mixed_batch(n, rng):
    """n roots: trees (repeated), nil trees and not-found roots; runs of node-less roots at the start,
    in the middle and at the end."""
    reqs = [NIL, NOT_FOUND, NIL, NIL, NIL, NOT_FOUND]
    while len(reqs) < n // 2:
        reqs.append(rng.choice(TREE_ROOTS + TREE_ROOTS + [NIL, NOT_FOUND]))
    reqs += [NOT_FOUND, NIL, NIL, NIL, NIL, NOT_FOUND, NOT_FOUND, NIL]
    while len(reqs) < n - 6:
        reqs.append(rng.choice(TREE_ROOTS + TREE_ROOTS + [NIL, NOT_FOUND]))
    reqs += [NIL, NIL, NOT_FOUND, NIL, NIL, NOT_FOUND]
    return reqs[:n]


def test_hub_and_mixed_children(shapes):
    """A union with 3,000 leaf children (past the 256-node gather bound and the 512-node piece), and
    the top / g2 / deep graph; the batch timing reports the expand passes as after keto_expand_batch."""
    want = _same(shapes, [HUB] + TREE_ROOTS, 5)
    hub = _texts(want["json"])[0]
    assert hub.count(b'{"type":"leaf"') == 3000
    shapes.expand_batch([HUB] + TREE_ROOTS, 5)
    _, req_two_step = shapes.last_timing()
    _fused(shapes, [HUB] + TREE_ROOTS, 5, "json")
    ms, req_fused = shapes.last_timing()
    assert req_fused == req_two_step and sum(req_fused) > 0 and ms[0] > 0


def test_batch_with_nil_and_error_runs(shapes):
    """600 roots mixing trees, nil trees, not-found roots and repeats, with runs of node-less roots at
    the start, in the middle and at the end."""
    from keto_amd.capi import EXPAND_NIL, EXPAND_NOT_FOUND, EXPAND_TREE
    reqs = _mixed_batch(600, random.Random(7))
    want = _same(shapes, reqs, 5)
    st = want["json"][0]
    assert {EXPAND_NIL, EXPAND_NOT_FOUND, EXPAND_TREE} == set(st)
    for s, txt in zip(st, _texts(_fused(shapes, reqs, 5, "json"))):
        assert (txt == b"null") if s == EXPAND_NIL else (txt == b"") if s == EXPAND_NOT_FOUND else txt.startswith(b"{")


@pytest.mark.parametrize("reqs", [[NIL, NOT_FOUND, NIL, NIL, NIL, NOT_FOUND, NOT_FOUND], [NOT_FOUND, NOT_FOUND], [NIL], []],
                         ids=["nil_and_errors", "errors", "one_nil", "empty"])
def test_batches_without_nodes(shapes, reqs):
    """All-nil and all-error batches, and n = 0 (count 0, offsets {0}, total 0)."""
    _same(shapes, reqs, 5)
    for enc in ENCODINGS:
        st, offs, raw = _fused(shapes, reqs, 5, enc)
        assert len(st) == len(reqs) and len(offs) == len(reqs) + 1 and offs[0] == 0 and offs[-1] == len(raw)
        if enc == "json":
            assert _texts((st, offs, raw)) == [b"null" if r is NIL else b"" for r in reqs]
        else:
            assert raw == b""


# ---------------------------------------------------------------- 5. deep chain
def test_deep_chain():
    """A 2,500-level chain at max-depth 3000, against the text built by hand."""
    from keto_amd.capi import EXPAND_TREE
    from oracle.oracle_sql import RelationTuple, SubjectID, SubjectSet
    k = 2500
    ns = [(1, "n")]
    tuples = [RelationTuple("n", f"g{i}", "m", SubjectSet("n", f"g{i + 1}", "m")) for i in range(k - 1)]
    tuples.append(RelationTuple("n", f"g{k - 1}", "m", SubjectID("user")))
    snap = _snapshot(ns, rows_from_tuples(ns, tuples), 100)
    text = '{"type":"leaf","subject_id":"user"}'
    for i in reversed(range(k)):
        text = ('{"type":"union","children":[' + text +
                '],"subject_set":{"namespace":"n","object":"g%d","relation":"m"}}' % i)
    reqs = [(("set", "n", "g0", "m"), 3000)]
    _same(snap, reqs, 3000)
    st, offs, raw = _fused(snap, reqs, 3000, "json")
    assert st == [EXPAND_TREE] and offs == [0, len(text)] and raw == text.encode()


# ---------------------------------------------------------------- 6. after a write
class _Handle:
    """A keto_encoded result kept open (the Snapshot methods free theirs)."""

    def __init__(self, snap, reqs, g, enc):
        from keto_amd import capi
        self.lib = snap.lib
        keep = capi._Keep()
        self.e = C.c_void_p()
        capi._check(self.lib.keto_expand_encode_batch(snap.h, snap._expand_reqs(keep, reqs), C.c_uint32(len(reqs)),
                                                      C.c_int32(g), C.c_uint32(capi.ENCODINGS[enc]), C.byref(self.e)))

    def read(self):
        n = self.lib.keto_encoded_count(self.e)
        total = C.c_uint64()
        p = self.lib.keto_encoded_bytes(self.e, C.byref(total))
        st = list(C.string_at(self.lib.keto_encoded_status(self.e), n))
        offs = np.frombuffer(C.string_at(self.lib.keto_encoded_offsets(self.e), 8 * (n + 1)), dtype=np.uint64).tolist()
        return st, offs, C.string_at(p, total.value) if total.value else b""

    def free(self):
        self.lib.keto_encoded_free(self.e)
        self.e = None


def test_after_a_write_and_results_outlive_the_snapshot():
    """keto_snapshot_apply adds new strings and a new row: the same requests match the two-step path
    before and after.  A result taken before the write reads the old bytes after it, and after the
    snapshot is released."""
    from keto_amd.capi import EXPAND_TREE
    ns = [(1, "n")]
    snap = _snapshot(ns, [(1, "doc", "view", "alice"), (1, "doc", "view", None, 1, "team", "member"),
                          (1, "team", "member", "bob")])
    reqs = [(("set", "n", "doc", "view"), 4), (("set", "n", "fresh<row>", "rel&new"), 4), (("id", "carol\n"), 1)]
    before = _same(snap, reqs, 5)
    assert _texts(before["json"])[1] == b"null"
    held = {enc: _Handle(snap, reqs, 5, enc) for enc in ENCODINGS}
    for enc in ENCODINGS:
        assert held[enc].read() == before[enc]
    snap.apply(inserts=[(1, "fresh<row>", "rel&new", "carol\n"), (1, "team", "member", None, 1, "fresh<row>", "rel&new"),
                        (1, "doc", "view", "dave \"d\"")])
    after = _same(snap, reqs, 5)
    assert after["json"][0] == [EXPAND_TREE] * 3
    assert _texts(after["json"])[1] == (b'{"type":"union","children":[{"type":"leaf","subject_id":"carol\\n"}],"subject_set":'
                                        b'{"namespace":"n","object":"fresh\\u003crow\\u003e","relation":"rel\\u0026new"}}')
    assert after["json"][2] != before["json"][2]
    for enc in ENCODINGS:
        assert held[enc].read() == before[enc]
    snap.close()
    for enc in ENCODINGS:
        assert held[enc].read() == before[enc]
        held[enc].free()


# ---------------------------------------------------------------- 7. roots past 2^31 units
def test_roots_past_2_31_units():
    """A snapshot laid out with KETO_TEST_ROOT_BASE as tests/test_gpu_arena_split.py's split48 layout
    (root rows past 2^31 units, a ~48 GiB arena whose gap is never built on the host): trees rooted at
    high rows take their root's row id from the request, the wildcard root in the same batch its
    batch-local row -- both branches of the root fix-up -- in the named and the ids form."""
    from keto_amd.capi import EXPAND_TREE
    ns = [(1, "n")]
    rows = [(1, "doc", "view", "alice"), (1, "doc", "view", None, 1, "team", "member"), (1, "team", "member", "bob"),
            (1, "doc2", "edit", "carol"), (1, "doc2", "edit", None, 1, "team", "member"),
            (1, "top", "all", None, 1, "doc", "view"), (1, "top", "all", None, 1, "doc2", "edit")]
    os.environ["KETO_TEST_ROOT_BASE"] = str(3 * (1 << 32) - (1 << 16))
    try:
        snap = _snapshot(ns, rows)
    finally:
        del os.environ["KETO_TEST_ROOT_BASE"]
    n_rows = snap.stats()["n_rows"]
    handles = snap.row_handles(np.arange(n_rows, dtype=np.uint32)).astype(np.int64)
    assert (handles >= (1 << 31)).any() and (handles < (1 << 31)).any()
    reqs = [(("set", "n", "top", "all"), 4), (("set", "n", "", "view"), 3), (("set", "n", "doc", "view"), 3),
            (("id", "nobody"), 1), (("set", "n", "none", "x"), 2), (("set", "n", "doc2", ""), 3),
            (("set", "n", "team", "member"), 2)]
    want = _same(snap, reqs, 5)
    assert want["json"][0][:3] == [EXPAND_TREE] * 3
    texts = _texts(want["json"])
    assert texts[0].endswith(b'"subject_set":{"namespace":"n","object":"top","relation":"all"}}')
    assert texts[1].endswith(b'"subject_set":{"namespace":"n","object":"","relation":"view"}}')
    roots = np.arange(n_rows, dtype=np.uint32) | SET
    depths = np.full(n_rows, 4, dtype=np.int32)
    want = _two_step_ids(snap, roots, depths, 5)
    for enc in ENCODINGS:
        assert _fused_ids(snap, roots, depths, 5, enc) == want[enc]
    snap.close()


# ---------------------------------------------------------------- 8. the ids form
def test_ids_form(shapes):
    """keto_expand_encode_batch_ids against keto_expand_batch_ids + the host encoders: every row as a
    subject-set root, subject-id roots between them; a row out of range is KETO_E_INVALID."""
    from keto_amd.capi import KetoError
    n_rows = shapes.stats()["n_rows"]
    roots = np.arange(n_rows, dtype=np.uint32) | SET
    roots = np.concatenate([roots, np.arange(0, 8, dtype=np.uint32), roots[::-1]])
    depths = (np.arange(len(roots)) % 6).astype(np.int32)
    want = _two_step_ids(shapes, roots, depths, 5)
    assert len(want["json"][2]) > 0
    for enc in ENCODINGS:
        assert _fused_ids(shapes, roots, depths, 5, enc) == want[enc]
    bad = np.array([int(roots[0]), n_rows | 0x80000000], dtype=np.uint32)
    for enc in ENCODINGS:
        with pytest.raises(KetoError) as err:
            shapes.expand_batch_ids_encoded(bad, np.zeros(2, dtype=np.int32), 5, enc)
        assert err.value.code == KETO_E_INVALID


# ---------------------------------------------------------------- 9. parts
def test_parts():
    """A 2-part shared-rows upload answers the roots this part owns and refuses the other part's with
    KETO_E_INVALID; a 2-part migrating upload refuses the call with KETO_E_INVALID."""
    from keto_amd.capi import PART_MIGRATE, KetoError
    from tools import synth
    g = synth.SynthGraph(synth.scaled(synth.POWERLAW_1B, 1 / 4096), threads=16)
    full = g.snapshot(device=0)
    rng = np.random.default_rng(52)
    rows = rng.integers(0, g.n_rows, size=2000).astype(np.uint32)
    own = full.row_owner(rows, 2)
    depths = rng.integers(-1, 7, size=len(rows)).astype(np.int32)
    part = g.snapshot_part(0, 2, device=0)
    mine = (own == 0) | (own < 0)
    assert mine.any() and (own == 1).any()
    roots = rows[mine] | SET
    want = _two_step_ids(part, roots, depths[mine], 5)
    assert len(want["proto"][2]) > 0
    for enc in ENCODINGS:
        assert _fused_ids(part, roots, depths[mine], 5, enc) == want[enc]
    other = rows[own == 1][:4] | SET
    for enc in ENCODINGS:
        with pytest.raises(KetoError) as err:
            part.expand_batch_ids_encoded(other, np.zeros(len(other), dtype=np.int32), 5, enc)
        assert err.value.code == KETO_E_INVALID
    del part
    mig = g.snapshot_part(0, 2, device=0, mode=PART_MIGRATE)
    for enc in ENCODINGS:
        with pytest.raises(KetoError) as err:
            mig.expand_batch_ids_encoded(np.array([0], dtype=np.uint32), np.zeros(1, dtype=np.int32), 5, enc)
        assert err.value.code == KETO_E_INVALID and "migrating" in str(err.value)


# ---------------------------------------------------------------- 10. interleaving and two threads
def test_interleaved_with_the_device_encoders_and_two_threads(shapes):
    """The fused JSON call, keto_tree_proto_all_device on an older arena, the fused protobuf call: the
    encoders share their device buffers.  Then two threads on the one snapshot, 20 calls each -- one
    the fused calls, the other keto_expand_batch + keto_tree_json_all_device: every result equals its
    serial value (the fused call keeps the expand's arena from the other thread's expand until its
    encoder has read it)."""
    from keto_amd import capi
    reqs_a = _mixed_batch(60, random.Random(11)) + [HUB]
    reqs_b = [HUB] + _mixed_batch(90, random.Random(12))
    want_a, want_b = _two_step(shapes, reqs_a, 5), _two_step(shapes, reqs_b, 5)
    keep = capi._Keep()
    old = C.c_void_p()
    capi._check(shapes.lib.keto_expand_batch(shapes.h, shapes._expand_reqs(keep, reqs_b), C.c_uint32(len(reqs_b)),
                                             C.c_int32(5), C.byref(old)))
    try:
        first = _fused(shapes, reqs_a, 5, "json")
        p_offs, p_raw, _ = shapes._proto_all(old, len(reqs_b), device=True)
        third = _fused(shapes, reqs_a, 5, "proto")
        j_offs, j_raw, _ = shapes._json_all_raw(old, len(reqs_b), device=True)
    finally:
        shapes.lib.keto_tree_arena_free(old)
    assert first == want_a["json"] and third == want_a["proto"]
    assert (p_offs.tolist(), p_raw) == want_b["proto"][1:] and (j_offs.tolist(), j_raw) == want_b["json"][1:]

    results, errors = {"fused": [], "pair": []}, []

    def fused():
        try:
            for k in range(20):
                enc = ENCODINGS[k % 2]
                results["fused"].append((enc, _fused(shapes, reqs_a, 5, enc)))
        except Exception as e:                                  # reported by the main thread
            errors.append(e)

    def pair():
        try:
            keep_b = capi._Keep()
            arr = shapes._expand_reqs(keep_b, reqs_b)
            for _ in range(20):
                a = C.c_void_p()
                capi._check(shapes.lib.keto_expand_batch(shapes.h, arr, C.c_uint32(len(reqs_b)), C.c_int32(5), C.byref(a)))
                try:
                    offs, raw, _ = shapes._json_all_raw(a, len(reqs_b), device=True)
                finally:
                    shapes.lib.keto_tree_arena_free(a)
                results["pair"].append((offs.tolist(), raw))
        except Exception as e:
            errors.append(e)

    ts = [threading.Thread(target=fused), threading.Thread(target=pair)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert len(results["fused"]) == len(results["pair"]) == 20
    for enc, got in results["fused"]:
        assert got == want_a[enc]
    for got in results["pair"]:
        assert got == want_b["json"][1:]
