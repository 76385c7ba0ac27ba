"""The expectation keto_allowed_subjects_batch is compared with: "which subject ids does a check allow on
namespace N, object O, relation R", answered the only way the reference can -- one
check.(*Engine).SubjectIsAllowed per subject id the store knows, on the oracle store's own SQLite connection.

  * candidates   SELECT DISTINCT subject_id of the whole store: a check says yes only when a tuple it reads
                 holds the requested subject (internal/check/engine.go:54), so an id no tuple holds can never
                 be allowed
  * the check    oracle.oracle_sql.CheckEngine(store, global max-depth).subject_is_allowed, which clamps the
                 request depth as internal/check/engine.go:118-120 does
  * the order    ids by their UTF-8 bytes: on a freshly built snapshot string-id order is byte order (a
                 subject first written by a later keto_snapshot_apply sorts last instead; the tests that
                 write say so themselves)
  * the page     ids [(page-1) * size, page * size), size 0 -> the store's page size, page 0 -> 1; the token
                 and the total by the list rule (internal/persistence/sql/relationtuples.go:262-265): "" when
                 page >= ceil(total / size)

The number of ids the device checked (`candidates`) is no part of the expectation: it depends on how far
the hop-bounded search got, which the reference has no notion of.  The tests that pin it work it out by hand.
"""
from oracle.oracle_sql import _NID, CheckEngine, NotFoundError, RelationTuple, SubjectID

ALLOWED_OK, ALLOWED_UNKNOWN_NAMESPACE, ALLOWED_UNDECIDED, ALLOWED_UNSUPPORTED = 0, 1, 2, 3


def subject_ids(store):
    """Every distinct subject id of the store, sorted by UTF-8 bytes."""
    rows = store.conn.execute("SELECT DISTINCT subject_id FROM keto_relation_tuples WHERE nid = ? AND "
                              "subject_id IS NOT NULL", (_NID,)).fetchall()
    return sorted((r[0] for r in rows), key=lambda s: s.encode())


def allowed_ids(store, namespace, obj, relation, depth, global_max_depth):
    """The subject ids the reference's check allows on namespace:obj#relation, in byte order; raises
    NotFoundError for an unknown namespace name."""
    store.nm.by_name(namespace)
    eng = CheckEngine(store, global_max_depth)
    return [s for s in subject_ids(store)
            if eng.subject_is_allowed(RelationTuple(namespace, obj, relation, SubjectID(s)), depth)]


def page_of(allowed, size, page):
    """The list rule over the allowed ids -> (the page, next token, total)."""
    first = (max(page, 1) - 1) * size
    total_pages = -(-len(allowed) // size)
    return allowed[first:first + size], "" if max(page, 1) >= total_pages else str(max(page, 1) + 1), len(allowed)


def expected(store, query, global_max_depth=5, cache=None):
    """query = (namespace, object, relation, depth, size, page) -> (status, [ids], token, total) as the first
    four fields of Snapshot.allowed_subjects report it.  cache: a dict shared by the queries of one store
    and global max-depth (the allowed set of a (namespace, object, relation, depth) is computed once for
    all its pages)."""
    ns, obj, rel, depth, size, page = query
    if ns == "" or obj == "" or rel == "":
        return (ALLOWED_UNSUPPORTED, [], "", 0)
    key = (ns, obj, rel, depth, global_max_depth)
    if cache is None or key not in cache:
        try:
            got = allowed_ids(store, ns, obj, rel, depth, global_max_depth)
        except NotFoundError:
            got = None
        if cache is not None:
            cache[key] = got
    else:
        got = cache[key]
    if got is None:
        return (ALLOWED_UNKNOWN_NAMESPACE, [], "", 0)
    ids, token, total = page_of(got, size if size else store.page_size, page)
    return (ALLOWED_OK, ids, token, total)


def last_page(n_allowed, size):
    return -(-n_allowed // size)
