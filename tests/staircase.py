"""Staircase graphs: checks whose answer hinges on one entry of the visited map.

One staircase (k1, k2, gmd, first_visit), in namespace "n", relation "r", every object prefixed by
the case's tag:

    top -> A                          the top-level tuple: one fresh visited map
    A -> a000 .. a{k1-1}              filler sets with no tuples
    A -> b0 -> c0 -> .. -> c{gmd-4}   a chain whose last set is opened at remaining depth 1
    c_last -> X                       only with first_visit: X enters the map, no depth left to open it
    A -> f000 .. f{k2-1}              more fillers
    A -> z -> X
    X -> user                         a subject id

The request n:<tag>top#r@user at request depth 0 and global max-depth gmd answers false with
first_visit (the second arrival at X, which has depth left, is cut by the visited map,
internal/check/engine.go:36-80 with internal/x/graph/graph_utils.go:13-35) and true without.  Between
X's entry and the arrival that decides, k2 + 1 further ids enter the map, and k1 + gmd - 1 entered
before it: the sweep moves X through every store of a tier-0 lane's map (LaneVisited in
keto_amd/csrc/engine.hip) and the map's size past every hand-over.

How a lane of geometry (RV, LV) keeps its map: the newest RV ids sit in registers, by age; an id
pushed out of the registers goes to the lane's LDS column while the map holds at most RV + LV ids
(the i-th id ever inserted, i < LV, lands in LDS slot i and stays there), later ones go to the
lane's HBM table; a table more than half full (128 of 256 entries) hands the request up to tier 1.
`home` says where an id with a given history sits.

Nothing here assumes where a*, b0, f* and z fall in A's row: `trace` walks the store by its own
ORDER BY (SQLStore.get_relation_tuples), page by page, the way the reference engine does.
"""
import random
from collections import namedtuple

from oracle.oracle_sql import NotFoundError, RelationTuple, SubjectID, SubjectSet

NS = [(1, "n")]
# k1 = 0, 3, 9 put the ids before X on both sides of every LDS column length at every max-depth;
# k1 = 5 makes X the 9th id at max-depth 4, i.e. the first id the 8-slot column of the default
# geometry cannot take: X alone in the table when the map first probes it
K1S = (0, 3, 5, 9)
K2S = tuple(range(0, 41)) + tuple(range(120, 161, 2))
K2_SMALL_MAX, K2_LARGE_MIN = 40, 120
# (register ids, LDS ids) of the tier-0 instances: w8 and variant 0, variants 1, 2, 3 (the default,
# and every max-depth 6..9 batch), 4, 5, 6; variant 7 is (8, 8) again
GEOMETRIES = ((16, 4), (8, 4), (4, 12), (8, 8), (6, 8), (6, 12), (8, 6))
T0_TABLE = 256                    # entries of a tier-0 lane's HBM table; it hands up past half
WELL_INSIDE = 64                  # ids younger than X in the table for "well inside"
MIN_SIZE = 5                      # top's A, b0, c0 and X at max-depth 4, and z before X arrives again

Case = namedtuple("Case", "index tag k1 k2 gmd first_visit")
# decision, ids inserted before X, ids inserted between X and the arrival that decides (X's age
# then), the map's size at that arrival, the map's size when the search ends
Trace = namedtuple("Trace", "decision before age size final")


def sweep(gmd, first_visits=(True, False)):
    """Every case of the sweep at one global max-depth, first_visit twins next to each other."""
    out = []
    for k1 in K1S:
        for k2 in K2S:
            for fv in first_visits:
                i = len(out)
                out.append(Case(i, f"s{i:03d}_", k1, k2, gmd, fv))
    return out


def _set(case, obj):
    return SubjectSet("n", case.tag + obj, "r")


def _tup(case, obj, sub):
    return RelationTuple("n", case.tag + obj, "r", sub)


def chain_last(case):
    """The object (without tag) of the chain's last set: opened at remaining depth 1."""
    return f"c{case.gmd - 4}"


def first_visit_tuple(case):
    return _tup(case, chain_last(case), _set(case, "X"))


def user_tuple(case):
    return _tup(case, "X", SubjectID("user"))


def case_tuples(case):
    assert case.gmd >= 4
    t = [_tup(case, "top", _set(case, "A"))]
    t += [_tup(case, "A", _set(case, f"a{i:03d}")) for i in range(case.k1)]
    t.append(_tup(case, "A", _set(case, "b0")))
    prev = "b0"
    for i in range(case.gmd - 3):
        t.append(_tup(case, prev, _set(case, f"c{i}")))
        prev = f"c{i}"
    assert prev == chain_last(case)
    if case.first_visit:
        t.append(first_visit_tuple(case))
    t += [_tup(case, "A", _set(case, f"f{i:03d}")) for i in range(case.k2)]
    t.append(_tup(case, "A", _set(case, "z")))
    t.append(_tup(case, "z", _set(case, "X")))
    t.append(user_tuple(case))
    return t


def request(case):
    return RelationTuple("n", case.tag + "top", "r", SubjectID("user"))


def engine_request(case):
    return ("n", case.tag + "top", "r", ("id", "user"), 0)


def all_tuples(cases, seed=11):
    """The tuples of every case, in a shuffled commit order."""
    t = [x for c in cases for x in case_tuples(c)]
    random.Random(seed).shuffle(t)
    return t


def batch(cases, repeat=12, seed=5):
    """Every case `repeat` times in a fixed shuffled order: neighbouring lanes of a wave hold maps of
    different sizes, and a lane's successive requests differ.  Consecutive cases (a first_visit case
    and its twin, in a full sweep) stay together, at an even position: a lane that takes requests in
    4-aligned runs starts the twin on the LDS column and the table in which the case before it left
    the same X."""
    assert len(cases) % 2 == 0
    pairs = [cases[i:i + 2] for i in range(0, len(cases), 2) for _ in range(repeat)]
    random.Random(seed).shuffle(pairs)
    return [c for p in pairs for c in p]


def trace(store, case):
    """Walks the request like check.Engine (pages in the store's ORDER BY, depth first) and records
    the visited map's history for X.  The decision is the walk's own; the CPU test holds it against
    CheckEngine's."""
    x_key = _set(case, "X").string()
    req = request(case)
    order = []                    # visit keys of the (single) top-level tuple's map, as inserted
    seen = {}
    arrival = []                  # (ids before X, X's age, map size) at X's arrivals after the first

    def further(visited, query, depth):
        if depth <= 0:
            return False
        token = ""
        while True:
            try:
                rels, token = store.get_relation_tuples(*query, token=token)
            except NotFoundError:
                return False
            for sr in rels:
                v = visited
                key = sr.subject.string()
                if v is None:                              # a fresh map per top-level tuple
                    v = seen
                    seen.clear()
                    del order[:]
                elif key in v:
                    if key == x_key:
                        arrival.append((order.index(key), len(order) - 1 - order.index(key), len(order)))
                    continue
                v[key] = len(order)
                # (subject ids enter the reference's map too; the engine keeps only those whose text
                # equals some set's String(), and "user" does not: the sizes count subject sets)
                if isinstance(sr.subject, SubjectSet):
                    order.append(key)
                if req.subject.equals(sr.subject):
                    return True
                if isinstance(sr.subject, SubjectSet):
                    s = sr.subject
                    if further(v, (s.namespace, s.object, s.relation), depth - 1):
                        return True
            if token == "":
                return False

    decision = further(None, (req.namespace, req.object, req.relation), case.gmd)
    if case.first_visit:
        (before, age, size), = arrival
    else:                                                  # X's only arrival inserts it
        assert not arrival
        before, age, size = seen[x_key], 0, seen[x_key]
    return Trace(decision, before, age, size, len(order))


def home(before, age, size, rv, lv):
    """Where a lane of geometry (rv, lv) holds the id inserted after `before` others, once `age`
    younger ids have followed it and the map holds `size` ids: "reg", "lds" or "hbm"."""
    assert size == before + 1 + age
    if age < rv:
        return "reg"
    return "lds" if before < lv else "hbm"


def hand_up_size(rv, lv):
    """The map size at which a tier-0 lane gives the request to tier 1: the table takes what the
    registers and the LDS column pushed out, and refuses the entry past half of its slots."""
    return rv + lv + T0_TABLE // 2 + 1


def coverage_gaps(traces, rv, lv):
    """What the first_visit cases with these traces leave untested for geometry (rv, lv): a list of
    descriptions, empty when the sweep covers every hand-over.  X's age at the deciding arrival on
    the last register, the first and the last age the LDS column takes over, the first age past it,
    and deep in the table; the map's size at rv, rv + 1, rv + lv, rv + lv + 1 and on both sides of the
    hand-up to tier 1; X found in registers, in LDS (with and without a table behind it) and in the
    table (as its newest entry and well inside)."""
    ages = {t.age for t in traces}
    sizes = {t.size for t in traces}
    finals = {t.final for t in traces}
    homes = {(home(t.before, t.age, t.size, rv, lv), t.size > rv + lv) for t in traces}
    gaps = []
    for what, age in (("last register", rv - 1), ("first LDS slot", rv), ("last LDS slot", rv + lv - 1),
                      ("first HBM entry", rv + lv)):
        if age not in ages:
            gaps.append(f"X's age never on the {what} (age {age})")
    if not any(a >= rv + lv + WELL_INSIDE for a in ages):
        gaps.append("X never well inside the HBM table")
    # (a staircase's map holds at least gmd + 1 >= 5 ids when X arrives again, so with 4 registers
    # even the smallest case is one past them: rv + 1 stands in for rv there)
    for s in ((rv,) if rv >= MIN_SIZE else ()) + (rv + 1, rv + lv, rv + lv + 1):
        if s not in sizes:
            gaps.append(f"no map of {s} ids at the deciding arrival")
    up = hand_up_size(rv, lv)
    if not any(f >= up for f in finals):
        gaps.append(f"no map reaches {up} ids: nothing handed up to tier 1")
    if not any(rv + lv < f < up for f in finals):
        gaps.append("no map spills to the table and stays in tier 0")
    for h in (("reg", False), ("lds", False), ("lds", True), ("hbm", True)):
        if h not in homes:
            gaps.append(f"X never found in {h[0]} with the map {'past' if h[1] else 'within'} registers + LDS")
    if not any(home(t.before, t.age, t.size, rv, lv) == "hbm" and t.age == rv for t in traces):
        gaps.append("X never the table's newest entry")
    if not any(t.before == lv and t.size == rv + lv + 1 for t in traces):
        gaps.append("X never the table's only entry at the map's first probe of it")
    return gaps
