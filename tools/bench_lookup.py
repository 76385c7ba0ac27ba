"""keto_lookup_objects_batch on BASELINE config #2's graph (Drive-like, 10M tuples, tools/synth.py DRIVE_10M)
on one MI355X, next to the path a caller had to compose before it existed:

  lookup     one keto_lookup_objects_batch call: candidates, requests and decisions stay on the device, the
             allowed row ids come home (page size 2^31 - 1: all of them)
  composed   keto_list_batch over namespace + relation (every tuple crosses PCIe) -> the distinct rows on the
             host -> keto_check_batch_pairs (the requests go back over PCIe) -> a filter on the host

for every (namespace, relation) of the graph -- a spread of candidate counts -- and a handful of sampled
users, one query per call, and then for batches of --batch users per (namespace, relation): one lookup call
of that many queries against one list call, one pairs call over rows x users and the filters.

Per case one JSON line: candidates and allowed objects, the wall time of either path (median, min and max
of --reps calls after --warmup unreported ones, the two paths alternating), the library's HIP-event times
of the lookup (keto_looked_timing; median of the same calls), the ratio of the medians and the mismatch
count between the two answers (row ids, in order), which must be 0.  The first lookup call's list-index
build is reported apart in the graph line.

  python tools/bench_lookup.py [--reps 9] [--warmup 2] [--users 3] [--batch 8] [--threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = 2 ** 31 - 1


def log(msg):
    print(f"[lookup {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def summary(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


def lookup(snap, ns, rel, users):
    """-> per user the allowed row ids, and the call's raw result."""
    r = snap.lookup_objects_raw([(ns, rel, ("id", u), 0, ALL, 0) for u in users], 5)
    offs = r["offsets"]
    return [r["rows"][int(offs[i]):int(offs[i + 1])] for i in range(len(users))], r


def composed(snap, ns, rel, words):
    """The composed path for the subject words (string ids) `words` -> per word the allowed row ids."""
    from keto_amd.capi import CHECK_PAIR_DTYPE
    status, offs, tup, nxt, tot, _ = snap.list_batch_raw([(ns, "", rel, None, ALL, 0)])
    rows = tup["row"]
    if len(rows):
        rows = rows[np.r_[True, rows[1:] != rows[:-1]]]          # the tuples of a row follow one another
    pairs = np.empty(len(rows) * len(words), dtype=CHECK_PAIR_DTYPE)
    pairs["row"] = np.tile(rows, len(words))
    pairs["subject"] = np.repeat(np.asarray(words, dtype=np.uint32), len(rows))
    dec = snap.check_batch_pairs(pairs, 0, 5) if len(pairs) else np.zeros(0, dtype=np.uint8)
    dec = dec.reshape(len(words), len(rows))
    return [rows[dec[i] == 1] for i in range(len(words))], len(rows)


def mismatches(a, b):
    return sum(0 if np.array_equal(x, y) else max(1, len(np.setxor1d(x, y))) for x, y in zip(a, b))


def case(snap, ns, rel, users, words, reps, warmup):
    lw, cw, ev = [], [], []
    got = want = None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        got, raw = lookup(snap, ns, rel, users)
        t1 = time.perf_counter()
        want, n_rows = composed(snap, ns, rel, words)
        t2 = time.perf_counter()
        if k >= warmup:
            lw.append((t1 - t0) * 1e3)
            cw.append((t2 - t1) * 1e3)
            ev.append(raw["timing"])
    assert not raw["status"].any() and not raw["undecided"].any(), raw["status"]
    assert int(raw["candidates"][0]) == n_rows, (raw["candidates"], n_rows)
    l, c = summary(lw), summary(cw)
    tm = lambda j: summary([e[j] for e in ev])["median"]
    return {"namespace": ns, "relation": rel, "queries": len(users), "candidates_per_query": n_rows,
            "allowed": [int(len(x)) for x in got], "lookup_wall_ms": l, "composed_wall_ms": c,
            "lookup_event_ms": {"candidates": tm(1), "check": tm(2), "emit": tm(3)},
            "composed_over_lookup": round(c["median"] / l["median"], 2) if l["median"] else None,
            "mismatches": mismatches(got, want)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--users", type=int, default=3, help="sampled users asked one per call")
    ap.add_argument("--batch", type=int, default=8, help="users of the batched leg")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    from tools import synth

    log("graph")
    g = synth.SynthGraph(dict(synth.DRIVE_10M), threads=a.threads, kind="drive")
    u = g.unified(threads=a.threads)
    t0 = time.perf_counter()
    snap = g.snapshot_unified(u, device=0)
    log(f"snapshot of {g.n_edges} tuples, {g.n_rows} rows in {time.perf_counter() - t0:.1f} s")
    names = dict(g.namespaces)
    rel = g.relation_names()
    user_s = lambda w: f"u{int(w) - u.user_base:08x}"
    rng = np.random.default_rng(19)
    ids = u.edges[(u.edges & 0x80000000) == 0]
    words = np.unique(rng.choice(ids, size=1000))[:max(a.users, a.batch)]
    users = [user_s(w) for w in words]
    # the subject word of a user is its string id: what the list resolver makes of the name
    plan = snap.list_plan([("", "", "", ("id", x), 0, 0) for x in users])
    assert [p["subject"] for p in plan] == [int(w) for w in words]
    # every (namespace, relation) that holds rows, smallest first
    live = np.asarray(g.row_ptr[1:]) > np.asarray(g.row_ptr[:-1])
    keys = []
    for i, n in g.namespaces:
        for j, r in enumerate(rel):
            k = int(((g.row_ns == i) & (g.row_rel == j) & live).sum())
            if k:
                keys.append((k, n, r))
    keys.sort()
    t0 = time.perf_counter()
    first = snap.lookup_objects_raw([(keys[0][1], keys[0][2], ("id", users[0]), 0, ALL, 0)], 5)
    first_ms = (time.perf_counter() - t0) * 1e3
    worst = None
    for k, n, r in keys:
        for x, w in list(zip(users, words))[:a.users]:
            line = case(snap, n, r, [x], [int(w)], a.reps, a.warmup)
            line["leg"] = "one query per call"
            print(json.dumps(line), flush=True)
            if worst is None or line["composed_over_lookup"] < worst:
                worst = line["composed_over_lookup"]
    for k, n, r in keys:
        line = case(snap, n, r, users[:a.batch], [int(w) for w in words[:a.batch]], a.reps, a.warmup)
        line["leg"] = f"{a.batch} queries per call"
        print(json.dumps(line), flush=True)
        if line["composed_over_lookup"] < worst:
            worst = line["composed_over_lookup"]
    st = snap.stats()
    print(json.dumps({"graph": "config #2 Drive-like", "tuples": int(g.n_edges), "rows": int(g.n_rows),
                      "device_bytes": int(st["device_bytes"]), "first_lookup_call_ms": round(first_ms, 3),
                      "first_lookup_call_index_ms": round(first["timing"][0], 3),
                      "smallest_composed_over_lookup": worst, "reps": a.reps, "warmup": a.warmup}), flush=True)


if __name__ == "__main__":
    main()
