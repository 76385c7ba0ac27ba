"""The edge-case families of tests/proto_util.py against the protobuf runtime and the SQL oracle
alone: the inputs of tests/test_gpu_proto_edges.py really sit where a length varint changes width,
and their hand-written expected trees are the reference's trees.  No engine, no device."""
import sys

import pytest

from oracle.oracle_sql import ExpandEngine, SQLStore, SubjectID, SubjectSet
from tests.proto_util import (A_LENGTHS, BOUNDS, C_INNER, C_MID, C_MID_14, EDGE_GLOBAL_DEPTH, EDGE_LENGTHS,
                              SubjectTree, batch_shapes, chain_tree, family_a, family_b, family_c, nested_sizes,
                              tree_json_to_proto)


@pytest.fixture(scope="module")
def fam_a():
    return family_a()


@pytest.fixture(scope="module")
def fam_b():
    return family_b()


@pytest.fixture(scope="module")
def fam_c():
    return family_c()


def _oracle_trees(ns, rows, reqs):
    store = SQLStore(ns, raw_rows=[tuple(r) + (None, None, None) if len(r) == 4 else r for r in rows])
    eng = ExpandEngine(store, EDGE_GLOBAL_DEPTH)
    out = []
    for sub, depth in reqs:
        t = eng.build_tree(SubjectID(sub[1]) if sub[0] == "id" else SubjectSet(*sub[1:]), depth)
        out.append(None if t is None else t.to_json())
    return out


@pytest.mark.parametrize("fam", ["fam_a", "fam_b", "fam_c"])
def test_expected_trees_are_the_oracles(fam, request):
    """The trees written out by hand equal ExpandEngine.build_tree on a store of the same rows."""
    ns, rows, reqs, want = request.getfixturevalue(fam)
    assert len(reqs) == len(want)
    got = _oracle_trees(ns, rows, reqs)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, reqs[i][0][0], reqs[i][1])


def test_batch_shapes_are_the_oracles():
    ns, rows, reqs, want, nil, _ = batch_shapes()
    assert _oracle_trees(ns, rows, reqs + [nil]) == want + [None]


def _a_sizes(want):
    """(sizes of the mid messages, sizes of the leaf messages below them, all nested sizes)."""
    mids, leaves, every = set(), set(), set()
    for t in want:
        z = nested_sizes(t)
        every.update(z)
        if t["type"] == "union":
            assert len(z) == 2                                   # pre-order: mid, its leaf
            mids.add(z[0])
            leaves.add(z[1])
    return mids, leaves, every


def test_family_a_straddles_every_bound(fam_a):
    """Some non-root message of family A has B - 1, B and B + 1 bytes for B = 2^7, 2^14, 2^21; more
    than that, the mid messages do (their children hold a leaf just below) and the leaves do (their
    string length is the only thing near)."""
    mids, leaves, every = _a_sizes(fam_a[3])
    for b in BOUNDS:
        assert {b - 1, b, b + 1} <= every, b
        assert {b - 1, b, b + 1} <= mids, b
        assert {b - 1, b, b + 1} <= leaves, b


def test_family_a_needs_every_length():
    """Without any one of its lengths family A misses a size: none of them is spare."""
    small = [n for n in A_LENGTHS if n < 1 << 20]                # the 2 MiB ones work the same way
    need = {b + d for b in BOUNDS[:2] for d in (-1, 0, 1)}
    for drop in small:
        mids, leaves, _ = _a_sizes(family_a([n for n in small if n != drop], ())[3])
        assert not (need <= mids and need <= leaves), drop


def _subjects(m):
    """Every Subject message of a parsed tree."""
    out, todo = [], [m]
    while todo:
        x = todo.pop()
        out.append(x.subject)
        todo.extend(x.children)
    return out


def test_family_b_field_lengths(fam_b):
    """Ids, objects, relations and namespace names of every edge length; the empty id and the set
    without fields; a SubjectSet whose inner length is 128 or more from fields below 128."""
    ids, nss, objs, rels, small_fields_long_set = set(), set(), set(), set(), False
    for t in fam_b[3]:
        for s in _subjects(SubjectTree.FromString(tree_json_to_proto(t))):
            if s.WhichOneof("ref") == "id":
                ids.add(len(s.id.encode()))
                continue
            assert s.WhichOneof("ref") == "set"
            f = [len(x.encode()) for x in (s.set.namespace, s.set.object, s.set.relation)]
            nss.add(f[0])
            objs.add(f[1])
            rels.add(f[2])
            small_fields_long_set |= max(f) < 128 <= s.set.ByteSize()
    for have in (ids, nss, objs, rels):
        assert set(EDGE_LENGTHS) <= have
    assert small_fields_long_set
    # multi-byte names: 128+ bytes in fewer than 128 characters
    assert any(len(r[3]) < 128 <= len(r[3].encode()) for r in fam_b[1] if r[3] is not None)
    assert any(len(n) < 128 <= len(n.encode()) for _, n in fam_b[0])
    assert any(n == "" for _, n in fam_b[0])


def test_family_b_fixed_bytes(fam_b):
    """The oneof is present even when empty, and a set without fields is 12 00."""
    ns, rows, reqs, want = fam_b
    assert tree_json_to_proto(want[reqs.index((("id", ""), 2))]) == bytes.fromhex("080412020A00")
    assert tree_json_to_proto(want[reqs.index((("set", "", "", ""), 1))]) == bytes.fromhex("080412021200")


def test_family_c_sits_on_the_edges(fam_c):
    """inner at 127, 128, 129; mid at 2^7 and 2^14 - 1, + 0, + 1; the hub (a non-root child with a
    leaf before it and two behind) at 2^14 - 1, + 0, + 1; and family C as a whole straddles 2^7 and
    2^14 like family A."""
    want = fam_c[3]
    n1, n2, n3 = len(C_INNER), len(C_MID), len(C_MID_14)
    edge = lambda b: [b - 1, b, b + 1]
    assert [nested_sizes(t)[1] for t in want[:n1]] == edge(BOUNDS[0])
    assert [nested_sizes(t)[0] for t in want[n1:n1 + n2]] == edge(BOUNDS[0])
    assert [nested_sizes(t)[0] for t in want[n1 + n2:n1 + n2 + n3]] == edge(BOUNDS[1])
    hubs = want[n1 + n2 + n3:]
    assert [nested_sizes(t)[1] for t in hubs] == edge(BOUNDS[1])
    for t in hubs:
        kids = t["children"]
        assert [k["type"] for k in kids] == ["leaf", "union", "leaf", "leaf"]
        assert len(kids[1]["children"]) > 4 * 256 and all(k["type"] == "leaf" for k in kids[1]["children"])
    sizes = set()
    for t in want:
        sizes.update(nested_sizes(t))
    for b in BOUNDS[:2]:
        assert set(edge(b)) <= sizes, b


def test_deep_chain_serializes():
    """The runtime serializes the 2,500-level chain (it only refuses to parse past 100 levels), so
    test_deep_chain_tree_json can compare bytes with it."""
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * 2500 + 1000))
    try:
        pb = tree_json_to_proto(chain_tree(2500))
    finally:
        sys.setrecursionlimit(old)
    assert pb.startswith(b"\x08\x01\x12") and pb.endswith(b"\x08\x04\x12\x06\x0a\x04user")
    assert pb.count(b"\x1a\x01m") == 2500
