"""acl.SubjectTree / Subject message classes built at run time from a descriptor that restates
proto/ory/keto/acl/v1alpha1/acl.proto and expand_service.proto (field numbers and types only), so
the tests can serialize the oracle's trees with the protobuf runtime and compare bytes with the
engine's encoder (keto_tree_proto).  Test infrastructure only."""
from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

_F = descriptor_pb2.FieldDescriptorProto


def _classes():
    fd = descriptor_pb2.FileDescriptorProto(name="keto_acl_restated.proto", package="ory.keto.acl.v1alpha1",
                                            syntax="proto3")
    ss = fd.message_type.add(name="SubjectSet")
    for i, n in enumerate(("namespace", "object", "relation"), 1):
        ss.field.add(name=n, number=i, type=_F.TYPE_STRING, label=_F.LABEL_OPTIONAL)
    sub = fd.message_type.add(name="Subject")
    sub.oneof_decl.add(name="ref")
    sub.field.add(name="id", number=1, type=_F.TYPE_STRING, label=_F.LABEL_OPTIONAL, oneof_index=0)
    sub.field.add(name="set", number=2, type=_F.TYPE_MESSAGE, label=_F.LABEL_OPTIONAL, oneof_index=0,
                  type_name=".ory.keto.acl.v1alpha1.SubjectSet")
    en = fd.enum_type.add(name="NodeType")
    for n, v in (("NODE_TYPE_UNSPECIFIED", 0), ("NODE_TYPE_UNION", 1), ("NODE_TYPE_EXCLUSION", 2),
                 ("NODE_TYPE_INTERSECTION", 3), ("NODE_TYPE_LEAF", 4)):
        en.value.add(name=n, number=v)
    st = fd.message_type.add(name="SubjectTree")
    st.field.add(name="node_type", number=1, type=_F.TYPE_ENUM, label=_F.LABEL_OPTIONAL,
                 type_name=".ory.keto.acl.v1alpha1.NodeType")
    st.field.add(name="subject", number=2, type=_F.TYPE_MESSAGE, label=_F.LABEL_OPTIONAL,
                 type_name=".ory.keto.acl.v1alpha1.Subject")
    st.field.add(name="children", number=3, type=_F.TYPE_MESSAGE, label=_F.LABEL_REPEATED,
                 type_name=".ory.keto.acl.v1alpha1.SubjectTree")
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    get = getattr(message_factory, "GetMessageClass", None)
    if get is None:
        f = message_factory.MessageFactory(pool)
        get = lambda d: f.GetPrototype(d)
    return get(pool.FindMessageTypeByName("ory.keto.acl.v1alpha1.SubjectTree"))


SubjectTree = _classes()


def tree_json_to_proto(js) -> bytes:
    """Tree.ToProto() (internal/expand/tree.go:165-188) of a reference JSON tree, serialized."""
    def fill(m, t):
        m.node_type = 4 if t["type"] == "leaf" else 1
        if "subject_id" in t:
            m.subject.id = t["subject_id"]
        else:
            s = t["subject_set"]
            m.subject.set.SetInParent()
            m.subject.set.namespace = s["namespace"]
            m.subject.set.object = s["object"]
            m.subject.set.relation = s["relation"]
        if t["type"] != "leaf":
            for c in t.get("children", []) or []:
                fill(m.children.add(), c)
    m = SubjectTree()
    fill(m, js)
    return m.SerializeToString(deterministic=True)


# ---------------------------------------------------------------------------------------------
# Edge cases of the length varints (tests/test_proto_edges_cpu.py, tests/test_gpu_proto_edges.py).
# Every family is (namespaces, rows, requests, expected JSON trees): rows as Snapshot.build takes
# them, requests as (subject, max-depth) for one batch at EDGE_GLOBAL_DEPTH, and request i's
# reference tree (None: a nil tree) written out from the rows -- children in the store's order
# (internal/persistence/sql/relationtuples.go:250: subject sets first, by namespace id, object and
# relation; then subject ids by their bytes), a set at the depth cut or without tuples as a leaf.
# The expected bytes are always tree_json_to_proto(expected tree): no arithmetic here.
EDGE_GLOBAL_DEPTH = 5
BOUNDS = (1 << 7, 1 << 14, 1 << 21)            # where a length varint gains a byte
EDGE_LENGTHS = (0, 1, 127, 128, 129, 16383, 16384)


def nested_sizes(js):
    """ByteSize() of every non-root SubjectTree message of a reference JSON tree, in pre-order, from
    the runtime (the values the encoders write behind every children tag).  Shallow trees only: the
    runtime parses at most 100 levels."""
    out, todo = [], list(reversed(SubjectTree.FromString(tree_json_to_proto(js)).children))
    while todo:
        m = todo.pop()
        out.append(m.ByteSize())
        todo.extend(reversed(m.children))
    return out


def leaf(sid):
    return {"type": "leaf", "subject_id": sid}


def leaf_set(ns, obj, rel):
    return {"type": "leaf", "subject_set": {"namespace": ns, "object": obj, "relation": rel}}


def union(ns, obj, rel, children):
    return {"type": "union", "children": children, "subject_set": {"namespace": ns, "object": obj, "relation": rel}}


# Family A.  n:tII#m -> n:mII#m -> one id of L bytes: with these 3-byte object names the leaf's
# message, or mII's, sits at B - 1, B, B + 1 for every B of BOUNDS (test_proto_edges_cpu.py holds
# them there).  The last six are the 2 MiB ids.
A_LENGTHS = (102, 103, 104, 121, 122, 123,
             16355, 16356, 16357, 16375, 16376, 16377,
             2097120, 2097121, 2097122, 2097141, 2097142, 2097143)
A_UNKNOWN = (103, 122, 16356, 16376, 2097121, 2097142)      # ids of these lengths no tuple holds


def family_a(lengths=A_LENGTHS, unknown=A_UNKNOWN):
    """Subtree-length edges: per L a tree top{mid{leaf}} and the id as a leaf root; then leaf roots
    the snapshot does not know (the arena's extra strings)."""
    ns, rows, reqs, want = [(1, "n")], [], [], []
    for i, n in enumerate(lengths):
        top, mid, x = f"t{i:02d}", f"m{i:02d}", "x" * n
        rows += [(1, top, "m", None, 1, mid, "m"), (1, mid, "m", x)]
        reqs += [(("set", "n", top, "m"), 3), (("id", x), 3)]
        want += [union("n", top, "m", [union("n", mid, "m", [leaf(x)])]), leaf(x)]
    for n in unknown:
        reqs.append((("id", "y" * n), 1))
        want.append(leaf("y" * n))
    return ns, rows, reqs, want


def family_b():
    """String, Subject and SubjectSet length edges: ids, objects, relations and namespace names of
    every EDGE_LENGTHS length (one field at a time and all three), a set whose inner length passes
    128 from fields of 42 + 43 + 43 bytes, multi-byte UTF-8 names, the empty id, a namespace named
    "", and wildcard roots (answered from batch-local rows; empty fields are left out of the
    message)."""
    e64, eur43 = "é" * 64, "€" * 43                     # 128 and 129 bytes
    ns = [(1, "n"), (2, "w")] + [(10 + i, "N" * n) for i, n in enumerate(EDGE_LENGTHS)]
    ns += [(30, "k" * 42), (31, e64), (32, eur43)]
    rows, reqs, want = [], [], []

    def ask(subject, depth, tree):
        reqs.append((subject, depth))
        want.append(tree)

    # subject ids: leaf roots (known and unknown to the snapshot) and children of n:ids#m
    for n in EDGE_LENGTHS:
        rows.append((1, "ids", "m", "i" * n))
        ask(("id", "i" * n), 2, leaf("i" * n))
        if n:
            ask(("id", "j" * n), 0, leaf("j" * n))
    ask(("set", "n", "ids", "m"), 2, union("n", "ids", "m", [leaf("i" * n) for n in EDGE_LENGTHS]))
    # subject sets: one long field at a time, then all three
    full = []
    for i, n in enumerate(EDGE_LENGTHS):
        if not n:
            continue
        nsid, name, obj, rel = 10 + i, "N" * n, "o" * n, "r" * n
        rows += [(1, obj, "m", "u"), (1, "obj", rel, "u"), (nsid, "obj", "m", "u"), (nsid, obj, rel, "u")]
        for s in (("n", obj, "m"), ("n", "obj", rel), (name, "obj", "m"), (name, obj, rel)):
            ask(("set",) + s, 1, leaf_set(*s))
            ask(("set",) + s, 2, union(*s, [leaf("u")]))
        rows.append((1, "sets", "m", None, nsid, obj, rel))
        full.append((name, obj, rel))
    # the namespace named "" (id 10): a subject set naming it reads as a wildcard namespace
    rows += [(10, "obj0", "m", "u"), (1, "sets", "m", None, 10, "obj0", "m")]
    full.insert(0, ("", "obj0", "m"))
    ask(("set", "", "obj0", "m"), 1, leaf_set("", "obj0", "m"))
    ask(("set", "", "obj0", "m"), 2, union("", "obj0", "m", [leaf("u")]))
    ask(("set", "n", "sets", "m"), 2, union("n", "sets", "m", [leaf_set(*s) for s in full]))
    ask(("set", "n", "sets", "m"), 3, union("n", "sets", "m", [union(*s, [leaf("u")]) for s in full]))
    # inner length 134 from fields of 42, 43 and 43 bytes
    s = ("k" * 42, "p" * 43, "q" * 43)
    rows.append((30, s[1], s[2], "u"))
    ask(("set",) + s, 1, leaf_set(*s))
    ask(("set",) + s, 2, union(*s, [leaf("u")]))
    # multi-byte UTF-8: 128+ bytes in fewer than 128 characters
    for nsid, a, b in ((31, e64, eur43), (32, eur43, e64)):
        rows.append((nsid, a, b, a))
        ask(("set", a, a, b), 1, leaf_set(a, a, b))
        ask(("set", a, a, b), 2, union(a, a, b, [leaf(a)]))
        ask(("id", a), 1, leaf(a))
    ask(("id", "ü" * 64), 1, leaf("ü" * 64))
    # wildcard roots over namespace w, and the root with no field at all
    rows += [(2, "a", "r1", "u1"), (2, "a", "r2", None, 2, "b", "r2"), (2, "b", "r2", "u2")]
    ask(("set", "w", "", ""), 3, union("w", "", "", [leaf("u1"), union("w", "b", "r2", [leaf("u2")]), leaf("u2")]))
    ask(("set", "w", "", "r2"), 2, union("w", "", "r2", [leaf_set("w", "b", "r2"), leaf("u2")]))
    ask(("set", "w", "a", ""), 2, union("w", "a", "", [leaf("u1"), leaf_set("w", "b", "r2")]))
    ask(("set", "", "", ""), 1, leaf_set("", "", ""))
    return ns, rows, reqs, want


# Family C.  (a, b, c): byte lengths of l1, l2, l3 in top{ mid{ inner{l1, l2}, l3 }, l4, l5 }; the
# five leaves are one pre-order run, taken 2 / 1 / 2 by the three unions.  C_INNER puts inner at
# 127, 128, 129; C_MID and C_MID_14 put mid at 2^7 and 2^14 - 1, + 0, + 1.
C_INNER = ((47, 47, 3), (47, 48, 3), (48, 48, 3))
C_MID = ((10, 10, 47), (10, 10, 48), (10, 10, 49))
C_MID_14 = ((10, 10, 16300), (10, 10, 16301), (10, 10, 16302))
C_HUB_MEMBERS = 1200
C_HUB_TUNED = (768, 769, 770)                  # the last member's id: the hub at 2^14 - 1, + 0, + 1


def family_c():
    """Leaf runs split between unions at width edges.  Requests 0-8: the variants of C_INNER, C_MID
    and C_MID_14 (nested_sizes()[0] is mid, [1] is inner).  Requests 9-11: pNN{ leaf set, hNN{1,200
    ids}, z1, z2 } -- the hub is a non-root child (nested_sizes()[1]), its members and z1, z2 one run
    over more than four 256-thread blocks."""
    ns, rows, reqs, want = [(1, "n")], [], [], []
    for v, (a, b, c) in enumerate(C_INNER + C_MID + C_MID_14):
        top, mid, inner = f"t{v:02d}", f"m{v:02d}", f"i{v:02d}"
        l1, l2, l3, l4, l5 = "a" * a, "b" * b, "c" * c, "d", "e"
        rows += [(1, top, "m", None, 1, mid, "m"), (1, top, "m", l4), (1, top, "m", l5),
                 (1, mid, "m", None, 1, inner, "m"), (1, mid, "m", l3), (1, inner, "m", l1), (1, inner, "m", l2)]
        reqs.append((("set", "n", top, "m"), 4))
        want.append(union("n", top, "m", [union("n", mid, "m", [union("n", inner, "m", [leaf(l1), leaf(l2)]), leaf(l3)]),
                                          leaf(l4), leaf(l5)]))
    for v, n in enumerate(C_HUB_TUNED):
        par, hub = f"p{v:02d}", f"h{v:02d}"
        members = [f"u{i:04d}" for i in range(C_HUB_MEMBERS - 1)] + ["v" * n]
        rows += [(1, par, "m", None, 1, "aaa", "m"), (1, par, "m", None, 1, hub, "m"), (1, par, "m", "z1"),
                 (1, par, "m", "z2")]
        rows += [(1, hub, "m", u) for u in members]
        reqs.append((("set", "n", par, "m"), 3))
        want.append(union("n", par, "m", [leaf_set("n", "aaa", "m"), union("n", hub, "m", [leaf(u) for u in members]),
                                          leaf("z1"), leaf("z2")]))
    return ns, rows, reqs, want


def chain_tree(k=2500):
    """The k-level chain of test_deep_chain_tree_json: n:g0#m -> ... -> n:g(k-1)#m -> user."""
    t = leaf("user")
    for i in reversed(range(k)):
        t = union("n", f"g{i}", "m", [t])
    return t


# Family D's snapshot: `top` = deep{deeper}, g2{u1, u2}, a, b, c; roots that give trees, a nil tree
# and an unknown namespace.
def batch_shapes():
    """(namespaces, rows, tree requests, their expected trees, a nil request, a not-found request)."""
    ns = [(1, "n")]
    rows = [(1, "top", "m", "a"), (1, "top", "m", None, 1, "g2", "m"), (1, "top", "m", "b"),
            (1, "top", "m", None, 1, "deep", "m"), (1, "top", "m", "c"), (1, "g2", "m", "u1"), (1, "g2", "m", "u2"),
            (1, "deep", "m", None, 1, "deeper", "m"), (1, "deeper", "m", "z")]
    g2 = union("n", "g2", "m", [leaf("u1"), leaf("u2")])
    ids = [leaf("a"), leaf("b"), leaf("c")]
    reqs = [(("set", "n", "top", "m"), 3), (("set", "n", "g2", "m"), 2), (("id", "someone"), 2),
            (("set", "n", "top", "m"), 2), (("set", "n", "deep", "m"), 4)]
    want = [union("n", "top", "m", [union("n", "deep", "m", [leaf_set("n", "deeper", "m")]), g2] + ids), g2,
            leaf("someone"), union("n", "top", "m", [leaf_set("n", "deep", "m"), leaf_set("n", "g2", "m")] + ids),
            union("n", "deep", "m", [union("n", "deeper", "m", [leaf("z")])])]
    return ns, rows, reqs, want, (("set", "n", "nothing", "m"), 3), (("set", "nope", "x", "y"), 3)
