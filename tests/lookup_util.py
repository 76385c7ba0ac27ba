"""The expectation keto_lookup_objects_batch is compared with: "which objects of namespace N does subject S
have relation R on", answered the only way the reference can -- one check.(*Engine).SubjectIsAllowed per
candidate object, on the oracle store's own SQLite connection.

  * candidates   SELECT DISTINCT object ... WHERE namespace_id = ? AND relation = ? (whereQuery,
                 internal/persistence/sql/relationtuples.go:178-198, with the object left out): an object
                 without a tuple at that relation can never be allowed, the check reads the top-level row's
                 tuples (internal/check/engine.go:82-114)
  * the check    oracle.oracle_sql.CheckEngine(store, global max-depth).subject_is_allowed, which clamps the
                 request depth as internal/check/engine.go:118-120 does
  * the order    objects by their UTF-8 bytes (the snapshot's key order inside one namespace and relation)
  * the page     rows [(page-1) * size, page * size), size 0 -> the store's page size, page 0 -> 1; the token
                 and the total by the list rule (internal/persistence/sql/relationtuples.go:262-265): "" when
                 page >= ceil(total / size)
"""
from oracle.oracle_sql import _NID, CheckEngine, NotFoundError, RelationTuple, SubjectID, SubjectSet

LOOKUP_OK, LOOKUP_UNKNOWN_NAMESPACE, LOOKUP_UNDECIDED, LOOKUP_UNSUPPORTED = 0, 1, 2, 3


def candidates(store, namespace, relation):
    """The distinct objects with a tuple at (namespace, relation), sorted by UTF-8 bytes; raises
    NotFoundError for an unknown namespace name."""
    ns_id, _ = store.nm.by_name(namespace)
    rows = store.conn.execute("SELECT DISTINCT object FROM keto_relation_tuples WHERE nid = ? AND namespace_id = ? "
                              "AND relation = ?", (_NID, ns_id, relation)).fetchall()
    return sorted((r[0] for r in rows), key=lambda o: o.encode())


def allowed_objects(store, namespace, relation, subject, depth, global_max_depth):
    """(every candidate object, those the reference's check allows), both in byte order."""
    cand = candidates(store, namespace, relation)
    eng = CheckEngine(store, global_max_depth)
    return cand, [o for o in cand if eng.subject_is_allowed(RelationTuple(namespace, o, relation, subject), depth)]


def page_of(allowed, size, page):
    """The list rule over the allowed objects -> (the page, next token, total)."""
    first = (max(page, 1) - 1) * size
    total_pages = -(-len(allowed) // size)
    return allowed[first:first + size], "" if max(page, 1) >= total_pages else str(max(page, 1) + 1), len(allowed)


def expected(store, query, global_max_depth=5, cache=None):
    """query = (namespace, relation, subject, depth, size, page) with subject a SubjectID / SubjectSet ->
    (status, [objects], token, total, candidates, undecided) as Snapshot.lookup_objects reports it.
    cache: a dict shared by the queries of one store and global max-depth (the allowed set of a
    (namespace, relation, subject, depth) is computed once for all its pages)."""
    ns, rel, sub, depth, size, page = query
    key = (ns, rel, sub, depth, global_max_depth)
    if cache is None or key not in cache:
        try:
            got = allowed_objects(store, ns, rel, sub, depth, global_max_depth)
        except NotFoundError:
            got = None
        if cache is not None:
            cache[key] = got
    else:
        got = cache[key]
    if got is None:
        return (LOOKUP_UNKNOWN_NAMESPACE, [], "", 0, 0, 0)
    cand, allowed = got
    objs, token, total = page_of(allowed, size if size else store.page_size, page)
    return (LOOKUP_OK, objs, token, total, len(cand), 0)


def subject_key(s):
    return ("id", s.id) if isinstance(s, SubjectID) else ("set", s.namespace, s.object, s.relation)


def to_request(query):
    """A lookup_util query -> the tuple Snapshot.lookup_objects takes."""
    ns, rel, sub, depth, size, page = query
    return (ns, rel, subject_key(sub), depth, size, page)


def last_page(n_allowed, size):
    return -(-n_allowed // size)
