"""Parity of every tier-0 check kernel instance with the SQL oracle, not only of the 8-wave build
that small batches get.

The instance is picked by environment (read per call by check_core, keto_amd/csrc/engine.hip):

    w8         nothing set      check_wave_kernel_w8<4, 4, 16>  (batches under 16 requests per lane)
    default6   KETO_T0_W8=0     check_wave_kernel<4, false, 8, 8, false, false>  (the large-batch kernel)
    v0 .. v7   KETO_T0=0 .. 7   the eight entries of t0_kernel()

for global max-depth <= 5; max-depth 6..9 always runs check_wave_kernel<8, false, 8, 8, false, false>.
Each runs on the default grid (about one request per lane) and with KETO_SLOTS=256 (a lane works
through many requests, each starting on the LDS column and the table its last one left behind);
default6 also with KETO_T0_DYN_FORCE=1 (runs of 4 dealt by the XCD heads: the headline setting).

* staircase (tests/staircase.py): checks whose answer hinges on one visited entry, swept so that
  the entry sits on every hand-over of every geometry -- last register, LDS column, HBM table,
  the hand-up to tier 1 (tests/test_visited_staircase_cpu.py proves the coverage and the answers);
* the same through the instrumented (COUNT = true) builds, whose counters feed the roofline;
* the same after writes, so the visited entry comes from an overlay row;
* the quirk corpus of test_gpu_parity.py (wildcard sets, poisoned pages, collisions, a namespace
  named "") through every instance.

No call reports which kernel a batch launched: profiles/r07a_tier0_matrix_kernels.txt is the
kernel trace of this file, with a launch count for every instance named above.
"""
import numpy as np
import pytest

from oracle.oracle_sql import CheckEngine, SQLStore
from tests import staircase as sc
from tests.engine_util import rows_from_tuples, subj
from tests.randgraph import random_checks, random_store

pytestmark = pytest.mark.gpu

T0_ENV = ("KETO_T0", "KETO_T0_W8", "KETO_SLOTS", "KETO_T0_DYN_FORCE")
INSTANCES = {"w8": {}, "default6": {"KETO_T0_W8": "0"}}
INSTANCES.update({f"v{i}": {"KETO_T0": str(i)} for i in range(8)})
GRIDS = {"grid": {}, "slots256": {"KETO_SLOTS": "256"},
         "headline": {"KETO_SLOTS": "256", "KETO_T0_DYN_FORCE": "1"}}
# max-depth <= 5: every instance on both grids, and the headline configuration
CONFIGS = {f"{i}-{g}": {**INSTANCES[i], **GRIDS[g]} for i in INSTANCES for g in ("grid", "slots256")}
CONFIGS["default6-headline"] = {**INSTANCES["default6"], **GRIDS["headline"]}
# max-depth 6..9: one instance whatever KETO_T0 says, on the three grids
DEEP_CONFIGS = {f"frames8-{g}": dict(GRIDS[g]) for g in GRIDS}


def _env(monkeypatch, env):
    for k in T0_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _build(tuples):
    import keto_amd
    return keto_amd.Snapshot.build(sc.NS, rows_from_tuples(sc.NS, tuples), device=0)


def _send(snap, order, want, gmd, label):
    """One batch through check_batch: every decision the oracle's; returns the number of requests
    tier 0 handed to tier 1."""
    allowed, status = snap.check_batch([sc.engine_request(c) for c in order], gmd)
    assert not status.any(), label
    bad = sorted({c for c, a in zip(order, allowed) if bool(a) != want[c.index]})
    assert not bad, (label, f"{len(bad)} cases wrong", [tuple(c) + (want[c.index],) for c in bad[:8]])
    return snap.last_timing()[1][1]


class _Lazy:
    """Per-gmd values built on first use and kept for the module."""

    def __init__(self, make):
        self.make, self.cache = make, {}

    def __call__(self, gmd):
        if gmd not in self.cache:
            self.cache[gmd] = self.make(gmd)
        return self.cache[gmd]

    def close(self):
        for v in self.cache.values():
            v[1].close()


def _make_stairs(gmd):
    cases = sc.sweep(gmd)
    tuples = sc.all_tuples(cases)
    eng = CheckEngine(SQLStore(sc.NS, tuples), gmd)
    want = [eng.subject_is_allowed(sc.request(c), 0) for c in cases]        # once per case
    assert any(want) and not all(want)
    return cases, _build(tuples), want


@pytest.fixture(scope="module")
def stairs():
    lazy = _Lazy(_make_stairs)
    yield lazy
    lazy.close()


def _staircase(monkeypatch, stairs, label, env, gmd):
    _env(monkeypatch, env)
    cases, snap, want = stairs(gmd)
    order = sc.batch(cases)
    assert len(order) == 12 * 496
    _send(snap, order, want, gmd, label)
    # the same cases in two batches: small maps, which tier 0 decides itself, and maps that outgrow
    # its table
    small = [c for c in order if c.k2 <= sc.K2_SMALL_MAX]
    large = [c for c in order if c.k2 >= sc.K2_LARGE_MIN]
    assert len(small) + len(large) == len(order)
    assert _send(snap, small, want, gmd, label + " small k2") == 0
    assert _send(snap, large, want, gmd, label + " large k2") > 0


@pytest.mark.parametrize("gmd", [4, 5])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_staircase_matches_oracle(monkeypatch, stairs, config, gmd):
    _staircase(monkeypatch, stairs, config, CONFIGS[config], gmd)


@pytest.mark.parametrize("gmd", [6, 9])
@pytest.mark.parametrize("config", sorted(DEEP_CONFIGS))
def test_staircase_matches_oracle_8_frames(monkeypatch, stairs, config, gmd):
    _staircase(monkeypatch, stairs, config, DEEP_CONFIGS[config], gmd)


@pytest.mark.parametrize("gmd", [5, 9])
def test_staircase_instrumented_builds(monkeypatch, stairs, gmd):
    """keto_check_work_device launches the COUNT = true instantiations (variant 3's at max-depth
    5, the 8-frame one at 9): the same decisions, and counters that counted."""
    import torch
    _env(monkeypatch, {"KETO_T0": "3"})
    cases, snap, want = stairs(gmd)
    order = sc.batch(cases)
    ids, status = snap.resolve_checks([sc.engine_request(c) for c in order])
    assert not status.any()
    d = torch.from_numpy(ids.view(np.int32).reshape(-1, 4).copy()).to("cuda:0")
    out = torch.empty(len(order), dtype=torch.uint8, device="cuda:0")
    w = snap.check_work_device(d.data_ptr(), len(order), out.data_ptr(), gmd)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = sorted({c for c, a in zip(order, got) if bool(a) != want[c.index]})
    assert not bad, (f"{len(bad)} cases wrong", [tuple(c) + (want[c.index],) for c in bad[:8]])
    assert w[0] >= len(order)                               # rows entered: at least one per request


def _make_written(gmd):
    """The sweep with first_visit absent everywhere (every answer true); then one transaction that
    inserts c_last -> X for the cases of even index (the visited entry now comes from an overlay
    row) and deletes X -> user for every third.  The oracle runs on the updated tuple list."""
    cases = sc.sweep(gmd, first_visits=(False,))
    tuples = sc.all_tuples(cases)
    snap = _build(tuples)
    before = [True] * len(cases)
    _send(snap, sc.batch(cases, repeat=2), before, gmd, "before the writes")
    ins = [sc.first_visit_tuple(c) for c in cases if c.index % 2 == 0]
    dels = [sc.user_tuple(c) for c in cases if c.index % 3 == 0]
    snap.apply(rows_from_tuples(sc.NS, ins), rows_from_tuples(sc.NS, dels))
    gone = set(dels)
    eng = CheckEngine(SQLStore(sc.NS, [t for t in tuples if t not in gone] + ins), gmd)
    want = [eng.subject_is_allowed(sc.request(c), 0) for c in cases]
    # both outcomes occur, and the writes are what changed the answers
    assert any(want) and not all(want)
    assert all(want[c.index] == (c.index % 2 != 0 and c.index % 3 != 0) for c in cases)
    return cases, snap, want


@pytest.fixture(scope="module")
def written():
    lazy = _Lazy(_make_written)
    yield lazy
    lazy.close()


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_staircase_after_writes(monkeypatch, written, config):
    _env(monkeypatch, {})
    cases, snap, want = written(5)
    _env(monkeypatch, CONFIGS[config])
    _send(snap, sc.batch(cases), want, 5, config)


@pytest.mark.parametrize("config", sorted(DEEP_CONFIGS))
def test_staircase_after_writes_8_frames(monkeypatch, written, config):
    _env(monkeypatch, {})
    cases, snap, want = written(6)
    _env(monkeypatch, DEEP_CONFIGS[config])
    _send(snap, sc.batch(cases), want, 6, config)


@pytest.mark.parametrize("seed,wide", [(s, False) for s in range(0, 300, 5)] +
                         [(s, True) for s in range(1000, 1060, 5)])
def test_quirk_corpus_through_every_instance(monkeypatch, seed, wide):
    """The random graphs of test_random_graphs_match_oracle (wildcard sets, poisoned pages at page
    sizes 1-3, String() collisions, a namespace named "") through every instance on the default
    grid; the oracle answers once per seed."""
    store, ns, tuples, raw, ps, alph = random_store(seed, wide=wide)
    import keto_amd
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples, raw), page_size=ps, device=0)
    checks = random_checks(seed, alph, k=24)
    groups = []
    for g in sorted({c[2] for c in checks}):                # one global max-depth per batch
        grp = [(t, d) for t, d, gg in checks if gg == g]
        eng = CheckEngine(store, g)
        groups.append((g, grp, [(t.namespace, t.object, t.relation, subj(t.subject), d) for t, d in grp],
                       [eng.subject_is_allowed(t, d) for t, d in grp]))
    for name in INSTANCES:
        _env(monkeypatch, INSTANCES[name])
        for g, grp, reqs, want in groups:
            allowed, _ = snap.check_batch(reqs, g)
            bad = [(t, d) for (t, d), a, w in zip(grp, allowed, want) if bool(a) != w]
            assert not bad, (name, seed, g, bad[:5])
    snap.close()
