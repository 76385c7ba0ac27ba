"""The expectations keto_subjects_batch is compared with.  Neither is the code under test.

(A) the oracle: oracle.oracle_sql.ExpandEngine(store, global max-depth).build_tree(SubjectSet(...), depth)
    (internal/expand/engine.go), flattened here: the SubjectID leaves of the tree, their ids mapped to the
    snapshot's string ids by keto_list_plan (host only), made distinct, sorted by string id and paged by the
    list rule (internal/persistence/sql/relationtuples.go:262-265).
(B) the two-step path: keto_expand_batch[_ids] nodes flattened with numpy -- unique of the id-leaf words per
    tree.  Works on any graph, synthetic ones included.

An answer is (status, [string ids], token, total, leaves, set_leaves): leaves = SubjectID leaf nodes before
deduplication, set_leaves = leaf nodes whose subject is a subject set.
"""
import ctypes as C

import numpy as np

from oracle.oracle_sql import ExpandEngine, NotFoundError, SubjectID, SubjectSet

SUBJECTS_OK, SUBJECTS_NOT_FOUND, SUBJECTS_UNDECIDED = 0, 1, 2
SET = 0x80000000


def page_of(words, size, page):
    """The list rule over the sorted distinct words -> (the page, next token, total)."""
    first = (max(page, 1) - 1) * size
    total_pages = -(-len(words) // size)
    return list(words[first:first + size]), "" if max(page, 1) >= total_pages else str(max(page, 1) + 1), len(words)


def last_page(total, size):
    return -(-total // size)


# ------------------------------------------------------------------------------------------------ (A)
def flatten_tree(tree):
    """An oracle Tree (or None) -> ([ids of the SubjectID leaves, duplicates kept], subject-set leaves)."""
    ids, sets = [], 0
    stack = [tree] if tree is not None else []
    while stack:
        t = stack.pop()
        if t.type == "leaf":
            if isinstance(t.subject, SubjectID):
                ids.append(t.subject.id)
            else:
                sets += 1
        stack.extend(t.children)
    return ids, sets


def oracle_leaves(store, namespace, obj, relation, depth, global_max_depth):
    """(ids with duplicates, set leaves) of the reference's tree, or None for herodot.ErrNotFound."""
    try:
        return flatten_tree(ExpandEngine(store, global_max_depth).build_tree(SubjectSet(namespace, obj, relation), depth))
    except NotFoundError:
        return None


def words_of(snap, ids, memo=None):
    """Subject-id strings -> the snapshot's string ids, by keto_list_plan (a host-only snapshot will do)."""
    memo = {} if memo is None else memo
    new = sorted({x for x in ids if x not in memo})
    if new:
        for x, p in zip(new, snap.list_plan([("", "", "", ("id", x), 0, 0) for x in new])):
            assert p["subject"] is not None and not p["subject"] & SET, (x, p)
            memo[x] = p["subject"]
    return [memo[x] for x in ids]


def expected_oracle(store, snap, query, global_max_depth=5, cache=None, memo=None):
    """query = (namespace, object, relation, depth, size, page) -> the answer, by yardstick (A).  cache: a dict
    shared by the queries of one store, snapshot version and global max-depth; memo: words_of's."""
    ns, obj, rel, depth, size, page = query
    key = (ns, obj, rel, depth, global_max_depth)
    cache = {} if cache is None else cache
    if key not in cache:
        got = oracle_leaves(store, ns, obj, rel, depth, global_max_depth)
        if got is not None:
            ids, sets = got
            got = (sorted(set(words_of(snap, ids, memo))), len(ids), sets)
        cache[key] = got
    got = cache[key]
    if got is None:
        return (SUBJECTS_NOT_FOUND, [], "", 0, 0, 0)
    words, leaves, sets = got
    ids, token, total = page_of(words, size if size else store.page_size, page)
    return (SUBJECTS_OK, ids, token, total, leaves, sets)


# ------------------------------------------------------------------------------------------------ (B)
def expand_nodes(snap, reqs, global_max_depth):
    """keto_expand_batch for reqs = [(subject, depth)] -> [(status, nodes as an (m, 2) uint32 array)]."""
    from keto_amd import capi
    keep = capi._Keep()
    n = len(reqs)
    a = C.c_void_p()
    capi._check(snap.lib.keto_expand_batch(snap.h, snap._expand_reqs(keep, reqs), C.c_uint32(n),
                                           C.c_int32(global_max_depth), C.byref(a)))
    out = []
    try:
        for i in range(n):
            st = snap.lib.keto_tree_status(a, C.c_uint32(i))
            nn = C.c_uint64()
            ptr = snap.lib.keto_tree_nodes(a, C.c_uint32(i), C.byref(nn))
            if nn.value:
                buf = (C.c_uint32 * (2 * nn.value)).from_address(C.cast(ptr, C.c_void_p).value)
                out.append((st, np.frombuffer(buf, dtype=np.uint32).copy().reshape(-1, 2)))
            else:
                out.append((st, np.zeros((0, 2), dtype=np.uint32)))
    finally:
        snap.lib.keto_tree_arena_free(a)
    return out


def flatten_nodes(nodes):
    """(m, 2) nodes of one tree -> (sorted distinct id-leaf words, id leaves, set leaves)."""
    leaf = (nodes[:, 1] & np.uint32(SET)) != 0
    is_set = (nodes[:, 0] & np.uint32(SET)) != 0
    words = nodes[leaf & ~is_set, 0]
    return np.unique(words), int(len(words)), int((leaf & is_set).sum())


def status_of_expand(st):
    from keto_amd.capi import EXPAND_NOT_FOUND, EXPAND_UNDECIDED
    return SUBJECTS_NOT_FOUND if st == EXPAND_NOT_FOUND else SUBJECTS_UNDECIDED if st == EXPAND_UNDECIDED else SUBJECTS_OK


def answers_from_trees(trees, queries, page_size):
    """trees: {(ns, obj, rel, depth): (status, nodes)}; queries as in expected_oracle -> their answers."""
    flat = {k: (status_of_expand(st),) + flatten_nodes(nodes) for k, (st, nodes) in trees.items()}
    out = []
    for ns, obj, rel, depth, size, page in queries:
        st, words, leaves, sets = flat[(ns, obj, rel, depth)]
        ids, token, total = page_of(words.tolist(), size if size else page_size, page)
        out.append((st, ids, token, total, leaves, sets))
    return out


def expected_two_step(snap, queries, global_max_depth, page_size):
    """The answers by yardstick (B): each distinct (namespace, object, relation, depth) expanded once."""
    heads = sorted({q[:4] for q in queries})
    got = expand_nodes(snap, [(("set", ns, obj, rel), d) for ns, obj, rel, d in heads], global_max_depth)
    return answers_from_trees(dict(zip(heads, got)), queries, page_size)


# ------------------------------------------------------------------------------------------------ the call
def answers(r):
    """Snapshot.subjects_raw's dict -> [(status, [string ids], token, total, leaves, set_leaves)]."""
    offs, ids = r["offsets"].tolist(), r["ids"].tolist()
    return [(int(r["status"][i]), ids[offs[i]:offs[i + 1]], str(int(r["next_page"][i])) if r["next_page"][i] else "",
             int(r["totals"][i]), int(r["leaves"][i]), int(r["set_leaves"][i])) for i in range(len(offs) - 1)]
