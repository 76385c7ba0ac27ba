"""Shared by the list-index patch tests (tests/test_list_patch_cpu.py, tests/test_gpu_list_patch.py):
random transactions over a random store's alphabet, applied to the snapshot and to SQLite alike, and
the host half of the patched index compared with SQLite and with a snapshot built afresh."""
import random

import keto_amd
from oracle.oracle_sql import RelationTuple, SubjectID, SubjectSet
from tests import delete_util
from tests.engine_util import rows_from_tuples

# strings the build never saw: "0" sorts before every string of the random alphabets, "zz" after them
NEW_OBJS = ["0", "zz"]
NEW_RELS = ["0r"]
NEW_USERS = ["0u", "zed"]


def wider(alph):
    """The random store's alphabet with the strings only writes bring."""
    names, objs, rels, users = alph
    return names, objs + NEW_OBJS, rels + NEW_RELS, users + NEW_USERS


def stored(store):
    """The store's tuples in commit order, as RelationTuples."""
    rows = store.conn.execute(
        "SELECT namespace_id, object, relation, subject_id, subject_set_namespace_id, subject_set_object, "
        "subject_set_relation FROM keto_relation_tuples ORDER BY commit_time").fetchall()
    return [store._to_internal(r) for r in rows]


def random_transaction(rng, alph, store, wildcards=True):
    """(inserts, deletes): new tuples, duplicates of stored ones, deletes of every equal stored tuple and
    deletes of tuples the store does not hold."""
    names, objs, rels, users = wider(alph)
    have = stored(store)

    def fresh():
        if rng.random() < 0.6:
            sub = SubjectID(rng.choice(users))
        else:
            so, sr = rng.choice(objs), rng.choice(rels)
            if wildcards and rng.random() < 0.1:
                so = ""
            if wildcards and rng.random() < 0.1:
                sr = ""
            sub = SubjectSet(rng.choice(names), so, sr)
        return RelationTuple(rng.choice(names), rng.choice(objs), rng.choice(rels), sub)

    ins = [fresh() for _ in range(rng.randint(0, 4))]
    if have:
        ins += [rng.choice(have) for _ in range(rng.randint(0, 2))]            # duplicates
    dels = [rng.choice(have) for _ in range(rng.randint(0, 3))] if have else []
    dels += [fresh() for _ in range(rng.randint(0, 2))]                         # mostly absent
    if rng.random() < 0.15 and have:                                            # empties whole rows
        t = rng.choice(have)
        dels += [u for u in have if (u.namespace, u.object, u.relation) == (t.namespace, t.object, t.relation)]
    return ins, dels


def apply(snap, store, ns, ins, dels):
    """One transaction on both sides (inserts, then deletes); returns the snapshot's new version.  A
    refused write raises: no case is left out silently."""
    version = snap.apply(rows_from_tuples(ns, ins), rows_from_tuples(ns, dels))
    for t in ins:
        store.insert(t)
    for t in dels:
        store.delete(t)
    store.conn.commit()
    return version


def check_host(snap, store, ns, ps, keys):
    """The host half after a write: every plan range holds exactly the key's tuples (SQLite), and it is
    the range of a snapshot built afresh from the store (positions in the global ORDER BY)."""
    delete_util.check_plans(snap, store, keys)
    queries = [("", "", "", None, 0, 0)] + [(n, o, r, None, 0, 0) for n, o, r in keys]
    fresh = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, stored(store)), page_size=ps, device=-1)
    want = [(p["lo"], p["hi"], p["status"]) for p in fresh.list_plan(queries)]
    got = [(p["lo"], p["hi"], p["status"]) for p in snap.list_plan(queries)]
    assert got == want, [(q, g, w) for q, g, w in zip(queries, got, want) if g != w]
    assert got[0][1] == delete_util.n_tuples(store)
    fresh.close()


def seeded(seed):
    return random.Random(seed * 7919 + 11)
