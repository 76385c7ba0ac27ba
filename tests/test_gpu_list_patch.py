"""The list index patched across writes on the GPU (the journal, the host merge and the list_splice
kernel) against Persister.GetRelationTuples restated on SQLite: random graphs under random transactions
with every page of every filter combination after each, the splice's segment / tile / parity edges
(default tile and KETO_LIST_TILE=256), the host half running ahead of the device half, deletes by query
in between, patching on against KETO_LIST_PATCH=0, results taken before the writes, and lists
concurrent with writes."""
import itertools
import json
import os
import subprocess
import sys
import threading

import pytest

from oracle.oracle_sql import RelationTuple as T, SQLStore, SubjectID, SubjectSet
from tests import delete_util, list_patch_util as lp, list_util
from tests.delete_util import PATH_DEVICE, PATH_HOST
from tests.engine_util import rows_from_tuples
from tests.randgraph import random_store

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERYTHING = ("", "", "", None, 10 ** 6, 1)


def _patched(snap, store, before, patches=1, builds=0):
    """The counters after a list call that found the device index `patches` patches (and `builds`
    rebuilds) behind; the index is current and holds exactly the store's tuples."""
    info = snap.list_index_info()
    assert (info["dev_patches"], info["dev_builds"]) == (before["dev_patches"] + patches, before["dev_builds"] + builds), \
        (before, info)
    assert (info["dev_current"], info["host_current"], info["dev_built"]) == (1, 1, 1), info
    assert info["entries"] == delete_util.n_tuples(store) and info["journal_rows"] == 0, info
    assert info["device_bytes"] >= 8 * ((info["entries"] + 2) & ~1)
    return info


def _whole_table(snap, store):
    """An unfiltered query with a page above the tuple count decodes to the whole table in ORDER BY order."""
    from tests.test_gpu_list import _compare
    (status, tup, token, total), = _compare(snap, store, [EVERYTHING])
    assert total == len(tup) == delete_util.n_tuples(store) and token == ""


# ---------------------------------------------------------------------------------- random parity
@pytest.mark.parametrize("seed", range(40))
def test_random_parity(seed):
    import keto_amd
    from tests.test_gpu_list import _all_pages, _compare
    store, ns, tuples, raw, ps, alph = random_store(seed, allow_poison=False)
    names, objs, rels, users = alph
    assert not raw and len(tuples) <= 40
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, tuples), page_size=ps, device=0)
    keys = list(itertools.product(sorted(set(names) | {""}), objs[:2] + ["0", ""], rels[:2] + [""]))
    sets = sorted({t.subject for t in tuples if isinstance(t.subject, SubjectSet)}, key=lambda s: s.string())
    subjects = [None, SubjectID(users[0]), SubjectID("zed")] + sets[:1]
    _compare(snap, store, [EVERYTHING])
    info = snap.list_index_info()
    assert (info["dev_builds"], info["dev_patches"], info["dev_current"], info["journal_valid"]) == (1, 0, 1, 1)
    rng = lp.seeded(seed)
    for rnd in range(5):
        for _ in range(rng.randint(1, 2)):
            lp.apply(snap, store, ns, *lp.random_transaction(rng, alph, store))     # raises if refused
        stale = snap.list_index_info()
        assert (stale["dev_current"], stale["journal_valid"]) == (0, 1), stale
        _compare(snap, store, _all_pages(store, keys, subjects, sizes=(0,)))
        info = _patched(snap, store, info)                      # exactly one patch, no rebuild
        assert info["dev_builds"] == 1
        _whole_table(snap, store)
        assert snap.list_index_info()["dev_patches"] == info["dev_patches"]       # current: nothing more to do
    snap.close()


# ---------------------------------------------------------------------------------- splice edges
SIZES = {"o10": 300, "o20": 600, "o30": 2, "o40": 300, "o45": 4200, "o50": 1}


def _splice_graph():
    ns = [(1, "n")]
    raw = [(1, o, "r", f"x{j:04d}", None, None, None) for o, k in SIZES.items() for j in range(k)]
    return ns, raw


def run_splice_edges():
    """Writes whose segments sit at every edge of the splice, on rows of 300, 600 and 4,200 entries (runs
    copied from the old index cross wave and tile boundaries at either tile), with whatever KETO_LIST_TILE
    the process has; the listings are compared with SQLite after every one.  Returns the patches done."""
    import keto_amd
    from tests.test_gpu_list import _compare
    ns, raw = _splice_graph()
    store = SQLStore(ns, raw_rows=raw)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, [], raw), device=0)
    row = lambda o, ids: [T("n", o, "r", SubjectID(i)) for i in ids]
    queries = lambda: [EVERYTHING, ("", "o20", "", None, 10 ** 6, 1), ("n", "o45", "r", None, 4096, 2),
                       ("", "", "r", SubjectID("x0001"), 0, 1), ("n", "", "", None, 255, 3), ("", "", "", None, 257, 2),
                       ("n", "o15", "", None, 0, 1), ("", "p0512", "", None, 0, 1)]
    _compare(snap, store, queries())
    info = snap.list_index_info()
    assert (info["dev_builds"], info["entries"]) == (1, len(raw))
    keys_bytes = lambda i: i["device_bytes"] - 8 * ((i["entries"] + 2) & ~1)
    parities, seen = set(), {}

    def write(what, ins, dels, segments=None, staged=None):
        nonlocal info
        lp.apply(snap, store, ns, ins, dels)
        _compare(snap, store, queries())
        before, info = info, _patched(snap, store, info)
        if segments is not None:
            assert (info["last_segments"], info["last_staged_entries"]) == (segments, staged), (what, info)
        parities.add(info["entries"] % 2)
        seen[what] = (before, info)
        return before, info

    # a segment at entry 0: the first row changes (its first entry too: "0a" sorts before "x0000")
    write("entry 0 changes", row("o10", ["0a"]), [], 1, 301)
    # a new row in front of everything: old_len = 0 at entry 0; the row id lies past keys[] as built
    b, a = write("a row in front of entry 0", row("o00", ["u"]), [], 1, 1)
    assert keys_bytes(a) > keys_bytes(b)
    # the last entry: the last row's only tuple is replaced, then a row is appended behind it
    write("the last entry changes", row("o50", ["y"]), row("o50", ["x0000"]), 1, 1)
    write("a row behind the last entry", row("o99", ["u", "v"]), [], 1, 2)
    # adjacent segments: two neighbouring rows in one write
    write("adjacent rows", row("o20", ["zz"]), row("o30", ["x0001"]), 2, 602)
    # growing from nothing (a new row of three) and shrinking to nothing (o30's last tuple leaves)
    write("from 0 and to 0", row("o25", ["a", "b", "c"]), row("o30", ["x0000"]), 2, 3)
    # one entry in front of the 600-entry row: everything behind it moves by an odd count
    b, a = write("an odd shift", row("o15", ["u"]), [], 1, 1)
    assert a["entries"] == b["entries"] + 1
    b, a = write("and the other parity", row("o15", ["v"]), [], 1, 2)
    assert a["entries"] == b["entries"] + 1 and parities == {0, 1}
    # a shrink in front of the long runs, and a segment in the middle of them
    write("a shrink", [], row("o10", [f"x{j:04d}" for j in range(0, 300, 2)]), 1, 151)
    write("inside the longest row", row("o45", ["x2100a"]), row("o45", ["x2100"]), 1, 4200)
    # a write that changes no tuple still brings the index to the new version
    write("nothing changes", row("o77", ["tmp"]), row("o77", ["tmp"]), 0, 0)
    # more new rows than the slack keys[] was given: it grows again
    b, a = write("1,100 new rows", [T("n", f"p{j:04d}", "r", SubjectID("u")) for j in range(1100)], [], 1100, 1100)
    assert keys_bytes(a) > keys_bytes(b)
    # every tuple leaves (N' = 0), then tuples come again
    everything = sorted(set(lp.stored(store)), key=lambda t: (t.object, t.subject.id))
    b, a = write("every tuple leaves", [], everything)
    assert a["entries"] == 0 and a["last_staged_entries"] == 0
    write("and tuples come again", row("o20", ["u"]) + row("o10", ["u", "v"]), [], 2, 3)
    assert info["dev_builds"] == 1
    return info["dev_patches"]


def test_splice_edges():
    assert "KETO_LIST_TILE" not in os.environ and "KETO_LIST_PATCH" not in os.environ
    assert run_splice_edges() == 14


def test_splice_edges_tile_256():
    env = dict(os.environ, KETO_LIST_TILE="256")
    code = "import tests.test_gpu_list_patch as t; print('splice edges ok:', t.run_splice_edges())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "splice edges ok: 14" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------- interleavings
NS = [(1, "n"), (2, "m")]
BASE = [T("n", "a", "r", SubjectID("u")), T("n", "a", "r", SubjectID("v")), T("n", "b", "r", SubjectSet("m", "g", "s")),
        T("m", "g", "s", SubjectID("u")), T("n", "c", "t", SubjectID("w")), T("n", "a", "r", SubjectID("u")),
        T("n", "d", "r", SubjectSet("m", "", "s"))]


def _small():
    import keto_amd
    store = SQLStore(NS, BASE, page_size=3)
    snap = keto_amd.Snapshot.build(NS, rows_from_tuples(NS, BASE), page_size=3, device=0)
    keys = list(itertools.product(["n", "m", ""], ["a", "b", "g", "aa", "0", ""], ["r", "s", ""]))
    subjects = [None, SubjectID("u"), SubjectSet("m", "g", "s"), SubjectSet("n", "aa", "r")]
    queries = lambda: [EVERYTHING] + [(n, o, r, s, 2, p) for (n, o, r), s in itertools.product(keys, subjects)
                                      for p in (1, 2, 3)]
    return store, snap, queries


def test_interleavings_and_old_results():
    from tests.test_gpu_list import _compare
    store, snap, queries = _small()
    _compare(snap, store, queries())
    old = snap.list_batch_raw([("", "", "", None, 100, 0)])
    old_dec = snap.decode_list_tuples(old[2])
    assert len(old_dec) == len(BASE)
    info = snap.list_index_info()
    keys = delete_util.plan_keys((["n", "m"], ["a", "aa", "b", "g", "0"], ["r", "s", "t"], []))

    # the host half advances first: a plan between the write and the list
    lp.apply(snap, store, NS, [T("n", "aa", "r", SubjectID("zed")), T("m", "g", "s", SubjectSet("n", "aa", "r")),
                               T("n", "0", "r", SubjectID("u"))], [T("n", "c", "t", SubjectID("w"))])
    delete_util.check_plans(snap, store, keys)
    mid = snap.list_index_info()
    assert (mid["host_current"], mid["dev_current"], mid["host_patches"], mid["journal_valid"]) == (1, 0, 1, 1)
    assert mid["journal_rows"] >= 4 and mid["dev_version"] == 0 and mid["host_version"] == 1
    # ... and a second write behind it: the device half is two versions behind, the host half one
    lp.apply(snap, store, NS, [T("n", "aa", "r", SubjectID("u"))], [T("n", "aa", "r", SubjectID("zed"))])
    _compare(snap, store, queries())
    info = _patched(snap, store, info)
    assert info["host_patches"] == 2 and info["dev_version"] == 2

    # two writes, then a list: one patch
    lp.apply(snap, store, NS, [T("n", "b", "r", SubjectID("q"))], [])
    lp.apply(snap, store, NS, [T("m", "h", "s", SubjectID("q"))], [T("n", "b", "r", SubjectID("q"))])
    _compare(snap, store, queries())
    info = _patched(snap, store, info)

    # a write, then a delete by query that finds the index stale: the host path, the index dropped with
    # its journal, and the next list rebuilds
    lp.apply(snap, store, NS, [T("n", "a", "s", SubjectID("u"))], [])
    want = delete_util.sql_delete(store, "", "", "", SubjectID("u"))
    got = snap.delete_query("", "", "", ("id", "u"))
    assert (got["deleted"], got["rows_touched"], got["path"], got["index_kept"]) == want + (PATH_HOST, 0)
    gone = snap.list_index_info()
    assert (gone["dev_built"], gone["journal_valid"], gone["entries"], gone["device_bytes"]) == (0, 0, 0, 0)
    _compare(snap, store, queries())
    info = _patched(snap, store, info, patches=0, builds=1)
    # ... then a write and a list: a patch again
    lp.apply(snap, store, NS, [T("n", "a", "r", SubjectID("u")), T("m", "g2", "s", SubjectID("q"))], [])
    _compare(snap, store, queries() + [("m", "g2", "", None, 0, 1)])
    info = _patched(snap, store, info)

    # a write, a list, then a delete on the device path: the patched index is patched by the delete
    lp.apply(snap, store, NS, [T("n", "e", "r", SubjectID("u"))], [])
    _compare(snap, store, queries())
    info = _patched(snap, store, info)
    want = delete_util.sql_delete(store, "n", "", "r", None)
    got = snap.delete_query("n", "", "r", None)
    assert (got["deleted"], got["rows_touched"], got["path"], got["index_kept"]) == want + (PATH_DEVICE, 1)
    info = _patched(snap, store, info)                          # delete_index_patch counts as one
    assert snap.list_batch_raw([("", "", "", None, 1, 0)])[5][0] == 0            # current: index_ms stays 0
    _compare(snap, store, queries())
    # ... and a write behind the delete is a patch of that index
    lp.apply(snap, store, NS, [T("n", "a", "r", SubjectID("u")), T("n", "d", "r", SubjectSet("m", "", "s"))], [])
    timing = snap.list_batch_raw([("", "", "", None, 1, 0)])[5]
    assert timing[0] > 0                                          # a patch reports its time, as a rebuild does
    _compare(snap, store, queries())
    info = _patched(snap, store, info)
    assert info["dev_builds"] == 2

    # row ids and string ids are only appended: the result taken before all of it decodes as before
    assert snap.decode_list_tuples(old[2]) == old_dec
    snap.close()


# ---------------------------------------------------------------------------------- patch on and off
def run_script():
    """A scripted sequence of writes and lists; prints the answers (statuses, decoded tuples, tokens,
    totals) as one JSON line and returns the index counters."""
    from tests.test_gpu_list import _compare
    store, snap, queries = _small()
    rng = lp.seeded(77)
    alph = (["n", "m"], ["a", "b", "g", "aa"], ["r", "s"], ["u", "v", "w"])
    answers = [_compare(snap, store, queries())]
    lists = 1
    for step in range(8):
        for _ in range(1 + step % 2):
            lp.apply(snap, store, NS, *lp.random_transaction(rng, alph, store))
        if step == 3:
            snap.list_plan([("n", "", "", None, 0, 0)])
        if step == 5:
            snap.delete_query("m", "", "", None)
            delete_util.sql_delete(store, "m", "", "", None)
        answers.append(_compare(snap, store, queries()))
        lists += 1
    print("answers:", json.dumps(answers))
    info = snap.list_index_info()
    return lists, info["dev_builds"], info["dev_patches"], info["host_builds"], info["host_patches"]


def _script(env):
    code = "import tests.test_gpu_list_patch as t; print('counters:', t.run_script())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    return json.loads(lines["answers"]), lines["counters"]


def test_patch_on_and_off_agree():
    assert "KETO_LIST_PATCH" not in os.environ
    on, on_counters = _script({})
    off, off_counters = _script({"KETO_LIST_PATCH": "0"})
    assert on == off and len(on) == 9
    # on: one build, one rebuild behind the stale delete, a patch for every other list; off: never a patch
    assert on_counters == "(9, 2, 7, 2, 8)", on_counters
    assert off_counters == "(9, 9, 0, 10, 0)", off_counters


# ---------------------------------------------------------------------------------- concurrency
def test_lists_concurrent_with_writes():
    import keto_amd
    ns = [(0, "m"), (1, "n")]                                     # m's tuples sort in front of n's: n's range moves
    base = [T("n", f"o{i:02d}", "r", SubjectID(f"u{j}")) for i in range(30) for j in range(3)] + \
           [T("m", "g0", "s", SubjectID("u0"))]
    store = SQLStore(ns, base, page_size=7)
    snap = keto_amd.Snapshot.build(ns, rows_from_tuples(ns, base), page_size=7, device=0)
    untouched = [("n", "", "", None, 1000, 1), ("n", "o07", "", None, 0, 1), ("", "", "r", SubjectID("u1"), 50, 2),
                 ("n", "", "", None, 7, 5)]
    want = [list_util.expected(store, q) for q in untouched]
    moving = ("m", "", "", None, 1000, 1)
    first = set(list_util.expected(store, moving)[1])
    assert snap.list_batch([list_util.to_request(q) for q in untouched]) == want
    writes = [[T("m", f"g{k % 5}", "s", SubjectID(f"w{k}"))] for k in range(20)]
    errors, totals = [], {0: [], 1: []}
    done = threading.Event()

    def lister(me):
        try:
            while True:
                last = done.is_set()
                got = snap.list_batch([list_util.to_request(q) for q in untouched + [moving]])
                assert got[:-1] == want, "a query the writes do not touch changed"
                status, tup, token, total = got[-1]
                assert status == 0 and total == len(tup) and first <= set(tup), "a tuple went missing"
                totals[me].append((total, set(tup)))
                if last:
                    return
        except BaseException as e:                               # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    def writer():
        try:
            for ins in writes:                                   # the store follows below, in its own thread
                snap.apply(rows_from_tuples(ns, ins), [])
        except BaseException as e:                               # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    threads = [threading.Thread(target=lister, args=(0,)), threading.Thread(target=lister, args=(1,)),
               threading.Thread(target=writer)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors, errors
    for ins in writes:
        store.insert(ins[0])
    final = set(list_util.expected(store, moving)[1])
    for me in (0, 1):
        seq = totals[me]
        assert seq and all(s <= final for _, s in seq)
        # the writes only insert, one tuple each: every listing is the table at some version, later ones later
        assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(seq, seq[1:]))
        assert seq[-1] == (len(final), final)                     # the call started after the last write saw it all
    info = snap.list_index_info()
    assert info["dev_builds"] == 1 and 1 <= info["dev_patches"] <= 20 and info["dev_current"] == 1
    snap.close()
