"""Persister.GetRelationTuples as a *list*, restated on the oracle store's own SQLite connection -- the
expectation keto_list_batch is compared with.

Followed reference lines (relative to the reference tree):
  * whereQuery    internal/persistence/sql/relationtuples.go:178-198
  * whereSubject  internal/persistence/sql/relationtuples.go:151-176 (exact equality on every field)
  * the query     internal/persistence/sql/relationtuples.go:238-277 (ORDER BY :250, Paginate :251,
                  token :262-265: "" when Page >= TotalPages, toInternal over the page :267-274)
  * pagination    internal/persistence/sql/persister.go:46,106-134 (size 0 -> the default page size,
                  which the oracle store carries as ``page_size``; token "" -> page 1)
pop's handling of page < 1 or per-page < 1 is not restated: callers pass page >= 1, size >= 0.
"""
from oracle.oracle_sql import _NID, _ORDER, NotFoundError, SubjectID, SubjectSet

LIST_OK, LIST_NOT_FOUND, LIST_UNDECIDED = 0, 1, 2

_COLS = ("namespace_id, object, relation, subject_id, subject_set_namespace_id, subject_set_object, "
         "subject_set_relation")


def where_clause(store, namespace, obj, relation, subject=None, key_only=False):
    """(sql, args) of whereQuery (+ whereSubject); raises NotFoundError for an unknown namespace name.
    key_only: the namespace / object / relation part alone (the names are still resolved)."""
    where, args = ["nid = ?"], [_NID]
    if namespace != "":
        ns_id, _ = store.nm.by_name(namespace)
        where.append("namespace_id = ?")
        args.append(ns_id)
    if obj != "":
        where.append("object = ?")
        args.append(obj)
    if relation != "":
        where.append("relation = ?")
        args.append(relation)
    if isinstance(subject, SubjectID):
        if not key_only:
            where += ["subject_id = ?", "subject_set_namespace_id IS NULL", "subject_set_object IS NULL",
                      "subject_set_relation IS NULL"]
            args.append(subject.id)
    elif isinstance(subject, SubjectSet):
        sns, _ = store.nm.by_name(subject.namespace)
        if not key_only:
            where += ["subject_set_namespace_id = ?", "subject_set_object = ?", "subject_set_relation = ?",
                      "subject_id IS NULL"]
            args += [sns, subject.object, subject.relation]
    return " AND ".join(where), args


def count_key_part(store, namespace, obj, relation):
    """COUNT(*) of the namespace / object / relation part of a query."""
    w, args = where_clause(store, namespace, obj, relation)
    return store.conn.execute(f"SELECT COUNT(*) FROM keto_relation_tuples WHERE {w}", args).fetchone()[0]


def get_relation_tuples(store, namespace, obj, relation, subject=None, size=0, page=1):
    """-> ([RelationTuple], next page token, total matches); raises NotFoundError like the reference."""
    per_page = size if size else store.page_size
    w, args = where_clause(store, namespace, obj, relation, subject)
    total = store.conn.execute(f"SELECT COUNT(*) FROM keto_relation_tuples WHERE {w}", args).fetchone()[0]
    rows = store.conn.execute(f"SELECT {_COLS} FROM keto_relation_tuples WHERE {w} ORDER BY {_ORDER} LIMIT ? OFFSET ?",
                              args + [per_page, (page - 1) * per_page]).fetchall()
    total_pages = -(-total // per_page)
    token = "" if page >= total_pages else str(page + 1)
    return [store._to_internal(r) for r in rows], token, total


def last_page(store, namespace, obj, relation, subject=None, size=0):
    """Number of pages of a query (0 for an empty one); raises NotFoundError for unknown namespaces."""
    per_page = size if size else store.page_size
    w, args = where_clause(store, namespace, obj, relation, subject)
    total = store.conn.execute(f"SELECT COUNT(*) FROM keto_relation_tuples WHERE {w}", args).fetchone()[0]
    return -(-total // per_page)


def subject_key(s):
    return ("id", s.id) if isinstance(s, SubjectID) else ("set", s.namespace, s.object, s.relation)


def tuple_key(t):
    """A RelationTuple as the comparable tuple of strings Snapshot.list_batch returns."""
    return (t.namespace, t.object, t.relation, subject_key(t.subject))


def expected(store, query):
    """query = (namespace, object, relation, subject or None, size, page) with page >= 0 (0 = "") ->
    (status, [tuple_key], token, total) as Snapshot.list_batch reports an answered query."""
    ns, obj, rel, sub, size, page = query
    try:
        tuples, token, total = get_relation_tuples(store, ns, obj, rel, sub, size, max(page, 1))
    except NotFoundError:
        return (LIST_NOT_FOUND, [], "", 0)
    return (LIST_OK, [tuple_key(t) for t in tuples], token, total)


def to_request(query):
    """A list_util query -> the tuple Snapshot.list_batch / list_plan take."""
    ns, obj, rel, sub, size, page = query
    return (ns, obj, rel, None if sub is None else subject_key(sub), size, page)
