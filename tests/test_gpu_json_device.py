"""keto_tree_json_all_device: every tree's Tree.MarshalJSON text encoded on the GPU.

The yardstick is the host encoder (keto_tree_json_all / keto_tree_json), which the rest of the suite
pins to the oracle's to_json(): raw bytes and offsets are compared, tree by tree, on one arena.
"""
import ctypes as C
import random

import numpy as np
import pytest

from tests.engine_util import rows_from_tuples, subj
from tests.randgraph import random_expands, random_store

pytestmark = pytest.mark.gpu


def _snapshot(namespaces, rows, page_size=100):
    import keto_amd
    return keto_amd.Snapshot.build(namespaces, rows, page_size=page_size, device=0)


class _Arena:
    """One keto_expand_batch arena, kept for several encoder calls."""

    def __init__(self, snap, reqs, g):
        from keto_amd import capi
        self.snap, self.n = snap, len(reqs)
        keep = capi._Keep()
        arr = snap._expand_reqs(keep, reqs)
        self.a = C.c_void_p()
        capi._check(snap.lib.keto_expand_batch(snap.h, arr, C.c_uint32(self.n), C.c_int32(g), C.byref(self.a)))
        self.status = [snap.lib.keto_tree_status(self.a, C.c_uint32(i)) for i in range(self.n)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.snap.lib.keto_tree_arena_free(self.a)

    def host(self):
        offs, raw, _ = self.snap._json_all_raw(self.a, self.n, device=False)
        return offs.tolist(), raw

    def device(self):
        offs, raw, _ = self.snap._json_all_raw(self.a, self.n, device=True)
        return offs.tolist(), raw

    def texts(self, enc):
        offs, raw = enc
        return [raw[offs[i]:offs[i + 1]] for i in range(self.n)]


def _same(ar, what=None):
    """Device offsets and bytes equal the host's; returns the per-tree texts."""
    h, d = ar.host(), ar.device()
    assert d[0] == h[0], what
    assert d[1] == h[1], what
    return ar.texts(d)


# ---------------------------------------------------------------- 1. random graphs
@pytest.mark.parametrize("seed", range(2300, 2340))
def test_random_expand_json_device_equals_host(seed):
    """Quirk-heavy random graphs (wildcard roots answered by batch-local rows, subject ids the snapshot
    does not know, empty fields, a namespace named "", collisions): the host encoder's text and
    offsets, tree by tree."""
    store, ns, tuples, raw, ps, alph = random_store(seed, wide=seed % 3 == 0)
    snap = _snapshot(ns, rows_from_tuples(ns, tuples, raw), ps)
    exps = random_expands(seed, alph, k=24)
    for g in sorted({e[2] for e in exps}):
        grp = [(subj(s), d) for s, d, gg in exps if gg == g]
        with _Arena(snap, grp, g) as ar:
            _same(ar, (seed, g))


# ---------------------------------------------------------------- 2. escaping
# name -> the text json_escape gives between the quotes (encoding/json with HTML escaping)
ESCAPES = [
    ('a"b\\c', b'a\\"b\\\\c'),
    ("<x>&y", b"\\u003cx\\u003e\\u0026y"),
    ("\n\r\t\x01\x08\x0c\x1f\x7f", b"\\n\\r\\t\\u0001\\u0008\\u000c\\u001f\x7f"),
    ("é€\U0001F600", "é€\U0001F600".encode()),
    ("\u2028\u2029", b"\\u2028\\u2029"),
    (b"\xff", b"\\ufffd"),
    (b"\xe2\x82", b"\\ufffd\\ufffd"),
    (b"\xc0\x80", b"\\ufffd\\ufffd"),
    (b"\xed\xa0\x80", b"\\ufffd\\ufffd\\ufffd"),
    (b"\xf4\x90\x80\x80", b"\\ufffd\\ufffd\\ufffd\\ufffd"),
    (b"ok\xe2", b"ok\\ufffd"),
]


def test_escaping_equals_host_and_hand_written_text():
    """Every class of json_escape (two-byte escapes, \\u00XX with lower-case hex, 0x7F raw, multi-byte
    UTF-8 copied, U+2028/9, and every kind of invalid sequence as \\ufffd per byte) in a namespace
    name, an object, a relation and a subject id: device == host == the text spelled out here, for
    leaf roots and for unions with these as children."""
    from keto_amd.capi import EXPAND_TREE
    names = [w for w, _ in ESCAPES]
    ns = [(i + 1, w) for i, w in enumerate(names)] + [(100, "plain")]
    rows = [(i + 1, w, w, w) for i, w in enumerate(names)]                        # (w:w#w) -> id w
    rows += [(100, "all", "m", None, i + 1, w, w) for i, w in enumerate(names)]   # plain:all#m -> every set
    rows += [(100, "all", "m", w) for w in names]                                 # ... and every id
    snap = _snapshot(ns, rows)

    def q(e):
        return b'"' + e + b'"'

    def leaf_id(e):
        return b'{"type":"leaf","subject_id":' + q(e) + b"}"

    def set_of(e):
        return b'"subject_set":{"namespace":' + q(e) + b',"object":' + q(e) + b',"relation":' + q(e) + b"}"

    reqs, want = [], []
    for w, e in ESCAPES:
        reqs.append((("id", w), 2))                       # a leaf root
        want.append(leaf_id(e))
        reqs.append((("set", w, w, w), 1))                # the set cut to a leaf
        want.append(b'{"type":"leaf",' + set_of(e) + b"}")
        reqs.append((("set", w, w, w), 2))                # a union with the id as its child
        want.append(b'{"type":"union","children":[' + leaf_id(e) + b"]," + set_of(e) + b"}")
    reqs.append((("set", "plain", "all", "m"), 2))        # a union with all of them as children
    with _Arena(snap, reqs, 5) as ar:
        assert all(s == EXPAND_TREE for s in ar.status)
        got = _same(ar)
    assert got[:-1] == want
    # the big union: every child spelled out, in whatever order the store gives them (two of the
    # names escape to the same text).  An escaped name holds no bare quote, so ',{"type":' only
    # occurs between children.
    pieces = [leaf_id(e) for _, e in ESCAPES] + [b'{"type":"leaf",' + set_of(e) + b"}" for _, e in ESCAPES]
    head, tail = b'{"type":"union","children":[', b'],"subject_set":{"namespace":"plain","object":"all","relation":"m"}}'
    text = got[-1]
    assert text.startswith(head) and text.endswith(tail)
    kids = text[len(head):len(text) - len(tail)].split(b',{"type":')
    kids = kids[:1] + [b'{"type":' + k for k in kids[1:]]
    assert sorted(kids) == sorted(pieces)


# ---------------------------------------------------------------- 3. deep chain
def test_deep_chain_json_device():
    """The 2,500-level chain of test_deep_chain_tree_json at max-depth 3000: the per-tree stack lives
    in scratch memory, and all 2,500 unions close behind the one leaf (one group of closes, innermost
    first)."""
    from keto_amd.capi import EXPAND_TREE
    from oracle.oracle_sql import RelationTuple, SubjectID, SubjectSet
    k = 2500
    ns = [(1, "n")]
    tuples = [RelationTuple("n", f"g{i}", "m", SubjectSet("n", f"g{i + 1}", "m")) for i in range(k - 1)]
    tuples.append(RelationTuple("n", f"g{k - 1}", "m", SubjectID("user")))
    snap = _snapshot(ns, rows_from_tuples(ns, tuples), 100)
    want = '{"type":"leaf","subject_id":"user"}'
    for i in reversed(range(k)):
        want = ('{"type":"union","children":[' + want +
                '],"subject_set":{"namespace":"n","object":"g%d","relation":"m"}}' % i)
    with _Arena(snap, [(("set", "n", "g0", "m"), 3000)], 3000) as ar:
        assert ar.status == [EXPAND_TREE]
        offs, raw = ar.device()
    assert offs == [0, len(want)]
    assert raw == want.encode()


# ---------------------------------------------------------------- 4. hub and shapes
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
NIL = (("set", "n", "nothing", "m"), 3)                  # no tuples: a nil tree ("null")
NOT_FOUND = (("set", "nope", "x", "y"), 3)               # unknown namespace: an empty range


def test_hub_spans_blocks(shapes):
    """A union with 3,000 leaf children (more than one 256-thread block, one leaf run)."""
    from keto_amd.capi import EXPAND_TREE
    with _Arena(shapes, [(("set", "n", "hub", "m"), 2)], 5) as ar:
        assert ar.status == [EXPAND_TREE]
        txt, = _same(ar)
    assert txt.count(b'{"type":"leaf"') == 3000 and txt.startswith(b'{"type":"union","children":[{"type":"leaf"')


def test_mixed_children_and_leaf_root(shapes):
    """leaf, union{2 leaves}, leaf, <deep>, leaf: a run of leaves crosses g2's end.  <deep> is a union
    whose only child is the set the depth cut turns into a leaf (max-depth 3), or itself that leaf
    (max-depth 2, where g2 is cut too).  The engine, like the reference, never emits a union without
    children: the depth cut gives a leaf, and the kernels treat both as "closes at once".  A subject-id
    root is a single leaf."""
    from keto_amd.capi import EXPAND_TREE
    with _Arena(shapes, TREE_ROOTS, 5) as ar:
        assert all(s == EXPAND_TREE for s in ar.status)
        got = _same(ar)
    leaf = lambda s: b'{"type":"leaf","subject_id":"' + s + b'"}'
    sset = lambda o: b'"subject_set":{"namespace":"n","object":"' + o + b'","relation":"m"}'
    assert got[2] == leaf(b"someone")
    assert got[1] == b'{"type":"union","children":[' + leaf(b"u1") + b"," + leaf(b"u2") + b"]," + sset(b"g2") + b"}"
    kids = {leaf(b"a"), leaf(b"b"), leaf(b"c"), got[1],
            b'{"type":"union","children":[{"type":"leaf",' + sset(b"deeper") + b"}]," + sset(b"deep") + b"}"}
    top = got[0]
    assert all(top.count(k) >= 1 for k in kids)
    order = sorted(kids, key=top.find)
    assert top == b'{"type":"union","children":[' + b",".join(order) + b"]," + sset(b"top") + b"}"


def _mixed_batch(n, rng):
    """n roots: trees (repeated), nil trees and not-found roots; runs of node-less roots at the
    start, in the middle (with 3+ nil trees in a row) and at the end."""
    reqs = [NIL, NOT_FOUND, NIL, NIL, NIL, NOT_FOUND]
    while len(reqs) < n // 2:
        reqs.append(rng.choice(TREE_ROOTS + TREE_ROOTS + [NIL, NOT_FOUND]))
    reqs += [NOT_FOUND, NIL, NIL, NIL, NIL, NOT_FOUND, NOT_FOUND, NIL]
    while len(reqs) < n - 6:
        reqs.append(rng.choice(TREE_ROOTS + TREE_ROOTS + [NIL, NOT_FOUND]))
    reqs += [NIL, NIL, NOT_FOUND, NIL, NIL, NOT_FOUND]
    return reqs[:n]


def test_batch_with_nil_and_error_runs(shapes):
    """600 roots mixing trees, nil trees, not-found roots and repeats: node-less trees have no node to
    hang "null" on and share a node index with their neighbours."""
    from keto_amd.capi import EXPAND_NIL, EXPAND_NOT_FOUND, EXPAND_TREE
    reqs = _mixed_batch(600, random.Random(7))
    with _Arena(shapes, reqs, 5) as ar:
        assert {EXPAND_NIL, EXPAND_NOT_FOUND, EXPAND_TREE} == set(ar.status)
        assert ar.status[:6] == [EXPAND_NIL, EXPAND_NOT_FOUND] + [EXPAND_NIL] * 3 + [EXPAND_NOT_FOUND]
        assert ar.status[-2:] == [EXPAND_NIL, EXPAND_NOT_FOUND]
        got = _same(ar)
    for st, txt in zip(ar.status, got):
        assert (txt == b"null") if st == EXPAND_NIL else (txt == b"") if st == EXPAND_NOT_FOUND else txt.startswith(b"{")


@pytest.mark.parametrize("reqs", [[NIL, NOT_FOUND, NIL, NIL, NIL, NOT_FOUND, NOT_FOUND], [NOT_FOUND, NOT_FOUND], [NIL], []],
                         ids=["nil_and_errors", "errors", "one_nil", "empty"])
def test_batches_without_nodes(shapes, reqs):
    """A batch that is all nil / error, and n = 0."""
    with _Arena(shapes, reqs, 5) as ar:
        got = _same(ar)
    assert got == [b"null" if r is NIL else b"" for r in reqs]


# ---------------------------------------------------------------- 5. buffers
def _call(snap, ar, buf_ptr, cap):
    offs = np.full(ar.n + 1, 0xDEADBEEF, dtype=np.uint64)
    rc = snap.lib.keto_tree_json_all_device(snap.h, ar.a, buf_ptr, C.c_uint64(cap), offs.ctypes.data_as(C.c_void_p))
    return rc, offs.tolist()


@pytest.mark.parametrize("pin_chunk", [None, 4096], ids=["default_chunks", "chunks_4k"])
def test_buffer_rules(shapes, monkeypatch, pin_chunk):
    """buf = NULL sizes; cap = total - 1 leaves buf untouched (offsets still written); a pinned
    keto_host_alloc buffer and a pageable one both get the text; KETO_PROTO_PIN_CHUNK=4096 sends the
    pageable one through many bounce chunks."""
    from keto_amd.capi import HostBuffer
    if pin_chunk:
        monkeypatch.setenv("KETO_PROTO_PIN_CHUNK", str(pin_chunk))
    reqs = [(("set", "n", "hub", "m"), 2), NIL] + TREE_ROOTS + [NOT_FOUND, NIL]
    with _Arena(shapes, reqs, 5) as ar:
        h_offs, h_raw = ar.host()
        total = len(h_raw)
        assert total > 5 * 4096
        rc, offs = _call(shapes, ar, None, 0)
        assert rc == total and offs == h_offs
        page = np.full(total, 0xA5, dtype=np.uint8)
        rc, offs = _call(shapes, ar, page.ctypes.data_as(C.c_void_p), total - 1)
        assert rc == total and offs == h_offs and (page == 0xA5).all()
        rc, offs = _call(shapes, ar, page.ctypes.data_as(C.c_void_p), total)
        assert rc == total and offs == h_offs and page.tobytes() == h_raw
        pinned = HostBuffer(total + 16, np.uint8)
        pinned.array[:] = 0xA5
        rc, offs = _call(shapes, ar, C.c_void_p(pinned.p.value), total - 1)
        assert rc == total and offs == h_offs and (pinned.array == 0xA5).all()
        rc, offs = _call(shapes, ar, C.c_void_p(pinned.p.value), total + 16)
        assert rc == total and offs == h_offs
        assert pinned.array[:total].tobytes() == h_raw and (pinned.array[total:] == 0xA5).all()   # no NUL, no overrun


# ---------------------------------------------------------------- 6. after a write
def test_after_apply_uses_new_tables():
    """keto_snapshot_apply adds tuples with new strings and a new row: the device tables are uploaded
    again for the new snapshot version."""
    from keto_amd.capi import EXPAND_TREE
    ns = [(1, "n")]
    snap = _snapshot(ns, [(1, "doc", "view", "alice"), (1, "doc", "view", None, 1, "team", "member"),
                          (1, "team", "member", "bob")])
    reqs = [(("set", "n", "doc", "view"), 4), (("set", "n", "fresh<row>", "rel&new"), 4), (("id", "carol\n"), 1)]
    with _Arena(snap, reqs, 5) as ar:
        before = _same(ar)
    assert before[1] == b"null"
    snap.apply(inserts=[(1, "fresh<row>", "rel&new", "carol\n"), (1, "team", "member", None, 1, "fresh<row>", "rel&new"),
                        (1, "doc", "view", "dave \"d\"")])
    with _Arena(snap, reqs, 5) as ar:
        assert ar.status == [EXPAND_TREE] * 3
        after = _same(ar)
    assert after[1] == (b'{"type":"union","children":[{"type":"leaf","subject_id":"carol\\n"}],"subject_set":'
                        b'{"namespace":"n","object":"fresh\\u003crow\\u003e","relation":"rel\\u0026new"}}')
    assert after[1] in after[0] and b'"dave \\"d\\""' in after[0] and after[0] != before[0]


# ---------------------------------------------------------------- 7. interleaving
def test_interleaved_with_device_proto(shapes):
    """Device JSON, device protobuf, device JSON on one arena: the encoders share their device
    buffers."""
    reqs = _mixed_batch(60, random.Random(11)) + [(("set", "n", "hub", "m"), 2)]
    with _Arena(shapes, reqs, 5) as ar:
        first = ar.device()
        p_offs, p_raw, _ = shapes._proto_all(ar.a, ar.n, device=True)
        third = ar.device()
        hp_offs, hp_raw, _ = shapes._proto_all(ar.a, ar.n, device=False)
        host = ar.host()
    assert first == third == host
    assert p_offs.tolist() == hp_offs.tolist() and p_raw == hp_raw


def test_host_only_snapshot_with_a_real_arena(shapes):
    """An arena and a host-only snapshot (device = -1): the code keto_tree_proto_all_device gives."""
    import keto_amd
    host_only = keto_amd.Snapshot.build([(1, "n")], [(1, "a", "r", "u")], device=-1)
    with _Arena(shapes, [TREE_ROOTS[1]], 5) as ar:
        offs = np.zeros(ar.n + 1, dtype=np.uint64)
        want = shapes.lib.keto_tree_proto_all_device(host_only.h, ar.a, None, C.c_uint64(0),
                                                     offs.ctypes.data_as(C.c_void_p))
        got = shapes.lib.keto_tree_json_all_device(host_only.h, ar.a, None, C.c_uint64(0),
                                                   offs.ctypes.data_as(C.c_void_p))
    assert got == want and want < 0
    assert shapes.lib.keto_last_error()
