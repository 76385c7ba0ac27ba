"""The three acl.SubjectTree encoders (keto_tree_proto, keto_tree_proto_all, keto_tree_proto_all_device)
against the protobuf runtime where a length varint changes width: the families of tests/proto_util.py,
which tests/test_proto_edges_cpu.py holds on the edges.  The yardstick is always
tree_json_to_proto(hand-written expected tree), byte for byte; nothing here computes a size.
"""
import ctypes as C
import itertools
import json
import random
import time

import numpy as np
import pytest

from tests.proto_util import (EDGE_GLOBAL_DEPTH, batch_shapes, family_a, family_b, family_c, leaf, tree_json_to_proto,
                              union)

pytestmark = pytest.mark.gpu


def _snapshot(namespaces, rows, page_size=100):
    import keto_amd
    return keto_amd.Snapshot.build(namespaces, rows, page_size=page_size, device=0)


def _same_bytes(got, want, what):
    """got == want, without a megabyte diff when they differ."""
    if got == want:
        return
    at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    raise AssertionError(f"{what}: {len(got)} bytes for {len(want)}, first difference at {at}: "
                         f"{got[at:at + 16].hex()} for {want[at:at + 16].hex()}")


class _Arena:
    """One keto_expand_batch arena, kept for several encoder calls, with the runtime's bytes of the
    expected trees (b"" for a root without a tree)."""

    def __init__(self, snap, reqs, want, g=EDGE_GLOBAL_DEPTH):
        from keto_amd import capi
        self.snap, self.n, self.want = snap, len(reqs), want
        self.pb = [b"" if t is None else tree_json_to_proto(t) for t in want]
        self.offs = [0] + list(itertools.accumulate(len(p) for p in self.pb))
        keep = capi._Keep()
        arr = snap._expand_reqs(keep, reqs)
        self.a = C.c_void_p()
        capi._check(snap.lib.keto_expand_batch(snap.h, arr, C.c_uint32(self.n), C.c_int32(g), C.byref(self.a)))
        self.status = [snap.lib.keto_tree_status(self.a, C.c_uint32(i)) for i in range(self.n)]

    def free(self):
        self.snap.lib.keto_tree_arena_free(self.a)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def proto_one(self, i):
        """keto_tree_proto of tree i: its bytes, or the negative code."""
        lib, snap = self.snap.lib, self.snap
        n = lib.keto_tree_proto(snap.h, self.a, C.c_uint32(i), None, C.c_uint64(0))
        if n <= 0:
            return n if n < 0 else b""
        buf = np.empty(n, dtype=np.uint8)
        assert lib.keto_tree_proto(snap.h, self.a, C.c_uint32(i), buf.ctypes.data_as(C.c_void_p), C.c_uint64(n)) == n
        return buf.tobytes()

    def proto_all(self, device):
        offs, raw, _ = self.snap._proto_all(self.a, self.n, device=device)
        return offs.tolist(), raw

    def json_all(self, device):
        offs, raw, _ = self.snap._json_all_raw(self.a, self.n, device=device)
        return offs.tolist(), raw

    def check_batch(self, device, what):
        """A batch encoder's offsets are the prefix sums of the runtime's lengths, its bytes the
        runtime's, tree by tree."""
        offs, raw = self.proto_all(device)
        assert offs == self.offs, what
        assert len(raw) == self.offs[-1], what
        for i, p in enumerate(self.pb):
            _same_bytes(raw[offs[i]:offs[i + 1]], p, (what, i))

    def check_each(self, what):
        for i, p in enumerate(self.pb):
            got = self.proto_one(i)
            assert isinstance(got, bytes), (what, i, got)
            _same_bytes(got, p, (what, i))

    def check_json(self, what):
        """E: the device JSON encoder gives the host's bytes and offsets, and each text is the
        expected tree."""
        host, dev = self.json_all(False), self.json_all(True)
        assert dev[0] == host[0], what
        _same_bytes(dev[1], host[1], what)
        offs, raw = dev
        for i, t in enumerate(self.want):
            assert json.loads(raw[offs[i]:offs[i + 1]]) == t, (what, i)


def _family(build):
    from keto_amd.capi import EXPAND_TREE
    ns, rows, reqs, want = build()
    t0 = time.perf_counter()
    ar = _Arena(_snapshot(ns, rows), reqs, want)
    print(f"\n{build.__name__}: {len(reqs)} trees, {ar.offs[-1]} bytes; snapshot + expand + runtime "
          f"{time.perf_counter() - t0:.2f} s")
    assert ar.status == [EXPAND_TREE] * len(reqs)
    return ar


@pytest.fixture(scope="module")
def arena_a():
    ar = _family(family_a)
    yield ar
    ar.free()


@pytest.fixture(scope="module")
def arena_b():
    ar = _family(family_b)
    yield ar
    ar.free()


@pytest.fixture(scope="module")
def arena_c():
    ar = _family(family_c)
    yield ar
    ar.free()


FAMILIES = ["arena_a", "arena_b", "arena_c"]


# ---------------------------------------------------------------- A-C: the three encoders, and E
@pytest.mark.parametrize("fam", FAMILIES)
def test_proto_edges_per_tree(fam, request):
    """keto_tree_proto of every tree: A subtree lengths, B string / Subject / SubjectSet lengths, C
    leaf runs split between unions, each at 2^7, 2^14 (and A at 2^21) - 1, + 0, + 1."""
    request.getfixturevalue(fam).check_each(fam)


@pytest.mark.parametrize("fam", FAMILIES)
def test_proto_edges_host_batch(fam, request):
    """keto_tree_proto_all: slices and offsets."""
    request.getfixturevalue(fam).check_batch(False, fam)


@pytest.mark.parametrize("fam", FAMILIES)
def test_proto_edges_device_batch(fam, request):
    """keto_tree_proto_all_device: slices and offsets.  Family A holds six 2 MiB ids, each copied by
    one lane (its wall time is printed)."""
    ar = request.getfixturevalue(fam)
    t0 = time.perf_counter()
    ar.check_batch(True, fam)
    print(f"\n{fam}: device protobuf (sizing + filling call, compared) {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("fam", FAMILIES)
def test_proto_edges_json_on_the_same_arena(fam, request):
    """keto_tree_json_all_device == keto_tree_json_all on the same arenas, and each text parses to
    the expected tree."""
    t0 = time.perf_counter()
    request.getfixturevalue(fam).check_json(fam)
    print(f"\n{fam}: host + device JSON, parsed {time.perf_counter() - t0:.2f} s")


def test_proto_edges_interleaved_with_device_json(arena_a):
    """Device protobuf, device JSON, device protobuf on family A's arena: the encoders share work
    buffers that the 2 MiB ids have just grown to megabytes."""
    arena_a.check_batch(True, "first")
    j_offs, j_raw = arena_a.json_all(True)
    arena_a.check_batch(True, "third")
    h_offs, h_raw = arena_a.json_all(False)
    assert j_offs == h_offs
    _same_bytes(j_raw, h_raw, "json between")


# ---------------------------------------------------------------- D: batches
@pytest.fixture(scope="module")
def shapes():
    """(snapshot, {request: expected tree}, tree requests, nil request, not-found request)."""
    ns, rows, reqs, want, nil, not_found = batch_shapes()
    table = dict(zip(reqs, want))
    table[nil] = table[not_found] = None
    return _snapshot(ns, rows), table, reqs, nil, not_found


def _mixed_batch(n, rng, trees, nil, nf):
    """n roots: trees (repeated), nil trees and not-found roots; runs of node-less roots at the
    start, in the middle (with 3+ nil trees in a row) and at the end."""
    reqs = [nil, nf, nil, nil, nil, nf]
    while len(reqs) < n // 2:
        reqs.append(rng.choice(trees + trees + [nil, nf]))
    reqs += [nf, nil, nil, nil, nil, nf, nf, nil]
    while len(reqs) < n - 6:
        reqs.append(rng.choice(trees + trees + [nil, nf]))
    reqs += [nil, nil, nf, nil, nil, nf]
    return reqs[:n]


def _check_mixed(ar, reqs, nil, nf):
    from keto_amd.capi import EXPAND_NIL, EXPAND_NOT_FOUND, EXPAND_TREE
    assert ar.status == [EXPAND_NIL if r is nil else EXPAND_NOT_FOUND if r is nf else EXPAND_TREE for r in reqs]
    ar.check_batch(True, "device")
    ar.check_batch(False, "host")
    assert all(a <= b for a, b in zip(ar.offs, ar.offs[1:]))
    for i, r in enumerate(reqs):                     # per tree: nil = no message, not found = an error
        got = ar.proto_one(i)
        if r is nf:
            assert isinstance(got, int) and got < 0
        else:
            assert got == ar.pb[i], i


def test_proto_edges_batch_with_nil_and_error_runs(shapes):
    """600 roots mixing trees, nil trees, not-found roots and repeats: node-less roots are zero-length
    slices; the lengths are the runtime's."""
    snap, table, trees, nil, nf = shapes
    reqs = _mixed_batch(600, random.Random(7), trees, nil, nf)
    assert reqs[0] is nil and reqs[1] is nf and reqs[-1] is nf and reqs[-2] is nil
    with _Arena(snap, reqs, [table[r] for r in reqs]) as ar:
        _check_mixed(ar, reqs, nil, nf)
        assert ar.offs[-1] > 0 and ar.offs[6] == 0 and ar.offs[-7] == ar.offs[-1]


@pytest.mark.parametrize("kinds", ["nfnnnff", "ff", "n", ""], ids=["nil_and_errors", "errors", "one_nil", "empty"])
def test_proto_edges_batches_without_nodes(shapes, kinds):
    """A batch that is all nil / error, and n = 0: every slice is empty."""
    snap, table, trees, nil, nf = shapes
    reqs = [nil if k == "n" else nf for k in kinds]
    with _Arena(snap, reqs, [None] * len(reqs)) as ar:
        _check_mixed(ar, reqs, nil, nf)
        assert ar.offs == [0] * (len(reqs) + 1)


def _call(ar, buf_ptr, cap):
    snap = ar.snap
    offs = np.full(ar.n + 1, 0xDEADBEEF, dtype=np.uint64)
    rc = snap.lib.keto_tree_proto_all_device(snap.h, ar.a, buf_ptr, C.c_uint64(cap), offs.ctypes.data_as(C.c_void_p))
    return rc, offs.tolist()


@pytest.mark.parametrize("pin_chunk", [None, 4096], ids=["default_chunks", "chunks_4k"])
def test_proto_edges_buffer_rules(arena_c, monkeypatch, pin_chunk):
    """buf = NULL sizes; cap = total - 1 returns the total, writes the offsets and leaves buf
    untouched; a pinned keto_host_alloc buffer with 16 spare bytes keeps its tail; a pageable one
    gets the bytes; KETO_PROTO_PIN_CHUNK=4096 sends the pageable one through more than 5 bounce
    chunks."""
    from keto_amd.capi import HostBuffer
    if pin_chunk:
        monkeypatch.setenv("KETO_PROTO_PIN_CHUNK", str(pin_chunk))
    ar = arena_c
    want, total = b"".join(ar.pb), ar.offs[-1]
    assert total > 5 * 4096
    rc, offs = _call(ar, None, 0)
    assert rc == total and offs == ar.offs
    page = np.full(total, 0xA5, dtype=np.uint8)
    rc, offs = _call(ar, page.ctypes.data_as(C.c_void_p), total - 1)
    assert rc == total and offs == ar.offs and (page == 0xA5).all()
    rc, offs = _call(ar, page.ctypes.data_as(C.c_void_p), total)
    assert rc == total and offs == ar.offs
    _same_bytes(page.tobytes(), want, "pageable")
    pinned = HostBuffer(total + 16, np.uint8)
    pinned.array[:] = 0xA5
    rc, offs = _call(ar, C.c_void_p(pinned.p.value), total - 1)
    assert rc == total and offs == ar.offs and (pinned.array == 0xA5).all()
    rc, offs = _call(ar, C.c_void_p(pinned.p.value), total + 16)
    assert rc == total and offs == ar.offs
    _same_bytes(pinned.array[:total].tobytes(), want, "pinned")
    assert (pinned.array[total:] == 0xA5).all()


def test_proto_edges_after_apply():
    """keto_snapshot_apply adds a tuple whose new id is 130 bytes, and a new row: the next device call
    encodes the new strings (compared with the runtime, not with an earlier call)."""
    from keto_amd.capi import EXPAND_NIL, EXPAND_TREE
    new = "N" * 130
    snap = _snapshot([(1, "n")], [(1, "doc", "view", "alice"), (1, "doc", "view", None, 1, "team", "member"),
                                  (1, "team", "member", "bob")])
    reqs = [(("set", "n", "doc", "view"), 4), (("set", "n", "fresh", "rel"), 4), (("id", new), 1)]
    team = union("n", "team", "member", [leaf("bob")])
    before = [union("n", "doc", "view", [team, leaf("alice")]), None, leaf(new)]
    with _Arena(snap, reqs, before) as ar:
        assert ar.status == [EXPAND_TREE, EXPAND_NIL, EXPAND_TREE]
        ar.check_batch(True, "before")
    snap.apply(inserts=[(1, "fresh", "rel", new), (1, "team", "member", None, 1, "fresh", "rel"),
                        (1, "doc", "view", "dave")])
    fresh = union("n", "fresh", "rel", [leaf(new)])
    team = union("n", "team", "member", [fresh, leaf("bob")])
    after = [union("n", "doc", "view", [team, leaf("alice"), leaf("dave")]), fresh, leaf(new)]
    with _Arena(snap, reqs, after) as ar:
        assert ar.status == [EXPAND_TREE] * 3
        ar.check_batch(True, "after")
        ar.check_batch(False, "after, host")
        ar.check_each("after, per tree")
