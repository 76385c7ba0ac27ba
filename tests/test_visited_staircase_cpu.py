"""The staircase sweep (tests/staircase.py) on the CPU: the SQL oracle answers false for every
first_visit case and true for its twin, so each negative hinges on the visited entry and nothing
else; and the sweep puts that entry on every hand-over of every tier-0 visited-map geometry."""
import pytest

from oracle.oracle_sql import CheckEngine, SQLStore, SubjectSet
from tests import staircase as sc


@pytest.fixture(scope="module", params=[4, 5, 6, 9])
def swept(request):
    gmd = request.param
    cases = sc.sweep(gmd)
    store = SQLStore(sc.NS, sc.all_tuples(cases))
    return gmd, cases, store, [sc.trace(store, c) for c in cases]


def _shape(case, tuples):
    """The tuples with the case's tag taken off."""
    k = len(case.tag)
    return sorted((t.object[k:], t.subject.object[k:] if isinstance(t.subject, SubjectSet) else "@" + t.subject.id)
                  for t in tuples)


def test_oracle_answers_hinge_on_the_visited_entry(swept):
    gmd, cases, store, traces = swept
    assert len(cases) == 2 * len(sc.K1S) * len(sc.K2S) == 496
    eng = CheckEngine(store, gmd)
    for c, t in zip(cases, traces):
        got = eng.subject_is_allowed(sc.request(c), 0)
        assert got == (not c.first_visit), c
        assert t.decision == got, c                       # the trace walks like the engine
    for a, b in zip(cases[0::2], cases[1::2]):            # twins differ in the one tuple
        assert (a.k1, a.k2, a.first_visit, b.first_visit) == (b.k1, b.k2, True, False)
        assert _shape(a, [t for t in sc.case_tuples(a) if t != sc.first_visit_tuple(a)]) == \
            _shape(b, sc.case_tuples(b))
        assert sc.first_visit_tuple(a) in sc.case_tuples(a)


def test_trace_counts_follow_the_stores_order(swept):
    """Ids before X: A, the k1 fillers, b0 and the chain; after it: the k2 fillers and z -- as the
    store's ORDER BY deals A's row, not as the tuples were committed (shuffled)."""
    gmd, cases, _, traces = swept
    for c, t in zip(cases, traces):
        if c.first_visit:
            assert (t.before, t.age, t.size) == (c.k1 + gmd - 1, c.k2 + 1, c.k1 + c.k2 + gmd + 1), c
            assert t.final == t.size
        else:
            assert (t.before, t.age, t.final) == (c.k1 + c.k2 + gmd, 0, c.k1 + c.k2 + gmd + 1), c


# the max-depth <= 5 instances (4 saved frames) run every geometry, max-depth 6..9 only (8, 8)
@pytest.mark.parametrize("gmds,geometries", [((4, 5), sc.GEOMETRIES), ((6, 9), ((8, 8),))],
                         ids=["frames4", "frames8"])
def test_sweep_covers_every_hand_over(gmds, geometries):
    traces, small, large = [], [], []
    for gmd in gmds:
        cases = sc.sweep(gmd)
        store = SQLStore(sc.NS, sc.all_tuples(cases))
        for c in cases:
            t = sc.trace(store, c)
            (small if c.k2 <= sc.K2_SMALL_MAX else large).append(t)
            if c.first_visit:
                traces.append(t)
    assert len(small) + len(large) == 496 * len(gmds) and sc.K2_SMALL_MAX < sc.K2_LARGE_MIN
    for rv, lv in geometries:
        assert sc.coverage_gaps(traces, rv, lv) == [], (rv, lv)
        # the split batches of the GPU matrix: tier 0 decides every small-k2 case itself, and some
        # large-k2 case is handed up
        up = sc.hand_up_size(rv, lv)
        assert max(t.final for t in small) < up, (rv, lv)
        assert max(t.final for t in large) >= up, (rv, lv)


def test_hand_over_model():
    assert sc.home(3, 15, 19, 16, 4) == "reg" and sc.home(3, 16, 20, 16, 4) == "lds"
    assert sc.home(4, 16, 21, 16, 4) == "hbm" and sc.home(0, 200, 201, 8, 8) == "lds"
    assert sc.hand_up_size(8, 8) == 145
    assert sc.coverage_gaps([], 8, 8) != []
