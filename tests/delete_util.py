"""Persister.DeleteAllRelationTuples restated on the oracle store's own SQLite connection -- the
expectation keto_snapshot_delete_query is compared with -- and the query sequences of its tests.

Followed reference lines (relative to the reference tree):
  * DeleteAllRelationTuples  internal/persistence/sql/relationtuples.go:225-236 (a DELETE by whereQuery)
  * whereQuery / whereSubject  :178-198, :151-176 (tests.list_util.where_clause)
"""
import random

from oracle.oracle_sql import SubjectID, SubjectSet
from tests import list_util

PATH_HOST, PATH_DEVICE = 0, 1
E_INVALID, E_REBUILD = -1, -6


def sql_delete(store, namespace, obj, relation, subject=None):
    """Runs the delete on the store -> (rows affected, distinct (namespace, object, relation) rows that
    held a match before it); raises NotFoundError for an unknown namespace, like the reference."""
    w, args = list_util.where_clause(store, namespace, obj, relation, subject)
    touched = store.conn.execute(
        f"SELECT COUNT(*) FROM (SELECT DISTINCT namespace_id, object, relation FROM keto_relation_tuples WHERE {w})",
        args).fetchone()[0]
    cur = store.conn.execute(f"DELETE FROM keto_relation_tuples WHERE {w}", args)
    store.conn.commit()
    return cur.rowcount, touched


def n_tuples(store):
    return store.conn.execute("SELECT COUNT(*) FROM keto_relation_tuples").fetchone()[0]


def request(q):
    """(namespace, object, relation, subject or None) -> Snapshot.delete_query's arguments."""
    ns, obj, rel, sub = q
    return ns, obj, rel, None if sub is None else list_util.subject_key(sub)


def query_sequence(seed, alph, tuples):
    """Deletes over every filter shape -- all three, namespace + object, object only, relation only,
    namespace, none -- each with a subject id, a stored subject set, a subject the store never saw, a
    string it never saw, and no subject; the narrow ones first so that later ones still find tuples,
    the empty query (everything that is left) last."""
    rng = random.Random(seed * 613 + 5)
    names, objs, rels, users = alph
    known = [n for n in names]
    stored = [t.subject for t in tuples if isinstance(t.subject, SubjectSet)]

    def shapes():
        n, o, r = rng.choice(known), rng.choice(objs), rng.choice(rels)
        return [(n, o, r), (n, o, ""), ("", o, ""), ("", "", r), (n, "", "")]

    out = []
    for (n, o, r) in shapes():
        out.append((n, o, r, SubjectSet(rng.choice(known), "zz-unknown", rng.choice(rels))))     # unknown subject
        out.append((n, o, r, SubjectID("zz-unknown")))
    out.append((rng.choice(known), "zz-unknown", "", None))                                       # unknown strings
    out.append(("", "", "zz-unknown", SubjectID(rng.choice(users))))
    for (n, o, r) in shapes():
        out.append((n, o, r, SubjectID(rng.choice(users))))
        if stored:
            out.append((n, o, r, rng.choice(stored)))
    for (n, o, r) in shapes():
        out.append((n, o, r, None))
    out.append(("", "", "", SubjectID(rng.choice(users))))
    if stored:
        out.append(("", "", "", rng.choice(stored)))
    for (n, o, r) in shapes():
        out.append((n, o, r, None))
    out.append(("", "", "", None))
    out.append(("", "", "", None))                                                                # nothing is left
    return out


def plan_keys(alph):
    """The narrowing keys whose list_plan range is exactly their tuples: namespace, namespace + object,
    all three."""
    names, objs, rels, _ = alph
    keys = [(n, "", "") for n in names if n != ""]
    keys += [(n, o, "") for n in names if n != "" for o in objs]
    keys += [(n, o, r) for n in names if n != "" for o in objs for r in rels]
    return keys


def check_plans(snap, store, keys):
    plans = snap.list_plan([(n, o, r, None, 0, 0) for n, o, r in keys])
    for k, p in zip(keys, plans):
        assert p["hi"] - p["lo"] == list_util.count_key_part(store, *k), (k, p)
