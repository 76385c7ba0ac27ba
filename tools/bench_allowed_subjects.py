"""keto_allowed_subjects_batch on BASELINE config #2's graph (Drive-like, 10M tuples, tools/synth.py DRIVE_10M)
on one MI355X, next to what a caller composes today and to the exact brute force:

  allowed    (a) one keto_allowed_subjects_batch call: frontier, candidates, requests and decisions stay on the
             device, the allowed string ids come home (page size 2^31 - 1: all of them)
  composed   (b) keto_subjects_batch at the same depth for the candidates (Expand's flatten) ->
             keto_check_batch_pairs over (row, id) (the requests go back over PCIe) -> a filter on the host.
             Not exact: Expand's tree is cut one level above the check's reach and keeps one visited map, so
             it can miss ids the check allows; `composed_wrong` counts the ids on which (b) differs from (a)
  brute      (c) keto_check_batch_pairs over (row, every string id of the snapshot) and a filter: exact, and
             what (a) must equal; run on the one-root-per-call legs only

Roots: a file, a folder and the largest group (by tuples) -- one per call, and 8 of each kind per call; and
--many folders (default 4096) in one call, where the BFS's frontier fans out over thousands of queries (the
line carries keto_allowed_bfs's counters: visited keys, table slots, enlargements, levels run again).

Per case one JSON line: the wall time of every path (median, min and max of --reps calls after --warmup
unreported ones, the paths alternating), the library's HIP-event times of (a) (keto_allowed_timing; median of
the same calls), the ratios of the medians, `composed_wrong`, and `mismatches` = the ids on which (a) and (c)
differ, which must be 0.

  python tools/bench_allowed_subjects.py [--reps 9] [--warmup 2] [--batch 8] [--threads 16]
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
GMD = 5


def log(msg):
    print(f"[allowed {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def summary(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


def split(ids, offs, n):
    return [ids[int(offs[i]):int(offs[i + 1])] for i in range(n)]


def allowed(snap, roots):
    r = snap.allowed_subjects_raw([(ns, obj, rel, 0, ALL, 0) for ns, obj, rel, _ in roots], GMD)
    return split(r["ids"], r["offsets"], len(roots)), r


def composed(snap, roots):
    from keto_amd.capi import CHECK_PAIR_DTYPE
    r = snap.subjects_raw([(ns, obj, rel, 0, ALL, 0) for ns, obj, rel, _ in roots], GMD)
    cand = split(r["ids"], r["offsets"], len(roots))
    pairs = np.empty(sum(len(c) for c in cand), dtype=CHECK_PAIR_DTYPE)
    pairs["row"] = np.concatenate([np.full(len(c), row, dtype=np.uint32) for c, (_, _, _, row) in zip(cand, roots)])
    pairs["subject"] = np.concatenate(cand) if len(pairs) else np.zeros(0, dtype=np.uint32)
    dec = snap.check_batch_pairs(pairs, 0, GMD) if len(pairs) else np.zeros(0, dtype=np.uint8)
    out, at = [], 0
    for c in cand:
        out.append(c[dec[at:at + len(c)] == 1])
        at += len(c)
    return out


def brute(snap, roots, n_strings):
    from keto_amd.capi import CHECK_PAIR_DTYPE
    out = []
    for _, _, _, row in roots:
        pairs = np.empty(n_strings, dtype=CHECK_PAIR_DTYPE)
        pairs["row"], pairs["subject"] = row, np.arange(n_strings, dtype=np.uint32)
        dec = snap.check_batch_pairs(pairs, 0, GMD)
        assert not (dec == 2).any()
        out.append(np.nonzero(dec == 1)[0].astype(np.uint32))
    return out


def differ(a, b):
    return sum(len(np.setxor1d(x, y)) for x, y in zip(a, b))


def case(snap, kind, roots, n_strings, reps, warmup, with_brute):
    aw, cw, bw, ev = [], [], [], []
    got = comp = exact = None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        got, raw = allowed(snap, roots)
        t1 = time.perf_counter()
        comp = composed(snap, roots)
        t2 = time.perf_counter()
        if with_brute:
            exact = brute(snap, roots, n_strings)
        t3 = time.perf_counter()
        if k >= warmup:
            aw.append((t1 - t0) * 1e3)
            cw.append((t2 - t1) * 1e3)
            bw.append((t3 - t2) * 1e3)
            ev.append(raw["timing"])
    assert not raw["status"].any() and not raw["undecided"].any(), raw["status"]
    a, c = summary(aw), summary(cw)
    tm = lambda j: summary([e[j] for e in ev])["median"]
    line = {"roots": kind, "queries": len(roots), "candidates": [int(x) for x in raw["candidates"]],
            "allowed": [int(len(x)) for x in got], "allowed_wall_ms": a, "composed_wall_ms": c,
            "allowed_event_ms": {"bfs": tm(0), "dedupe": tm(1), "check": tm(2), "emit": tm(3)},
            "composed_over_allowed": round(c["median"] / a["median"], 2) if a["median"] else None,
            "composed_ids": [int(len(x)) for x in comp], "composed_wrong": differ(got, comp), "bfs": raw["bfs"]}
    if len(roots) > 16:                                     # the per-query lists of a big batch: their sums
        for k in ("candidates", "allowed", "composed_ids"):
            line[k] = int(sum(line[k]))
    if with_brute:
        b = summary(bw)
        line.update({"brute_wall_ms": b, "brute_over_allowed": round(b["median"] / a["median"], 2) if a["median"] else None,
                     "mismatches": differ(got, exact)})
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8, help="roots of the batched legs")
    ap.add_argument("--many", type=int, default=4096, help="folders of the many-queries leg")
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
    n_strings = int(snap.stats()["n_strings"])
    sizes = np.asarray(g.row_ptr[1:]) - np.asarray(g.row_ptr[:-1])
    rng = np.random.default_rng(23)

    def roots_of(ns_name, rel_name, k, largest=False):
        """k rows of (namespace, relation) as (namespace, object, relation, row id): sampled among those with
        tuples, or the k with the most tuples."""
        ns_id = next(i for i, n in g.namespaces if n == ns_name)
        idx = np.nonzero((g.row_ns == ns_id) & (g.row_rel == rel.index(rel_name)) & (sizes > 0))[0]
        pick = idx[np.argsort(sizes[idx], kind="stable")[::-1][:k]] if largest else np.sort(rng.choice(idx, size=k, replace=False))
        return [(ns_name, f"{int(g.row_obj[r]):08x}", rel_name, int(r)) for r in pick]

    kinds = [("file", roots_of("files", "view", a.batch)), ("folder", roots_of("folders", "view", a.batch)),
             ("largest group", roots_of("groups", "member", a.batch, largest=True))]
    # the CSR row index is the snapshot's row id: the list call says so for the first root of every kind
    for _, roots in kinds:
        ns, obj, r, row = roots[0]
        assert int(snap.list_batch_raw([(ns, obj, r, None, 1, 0)])[2]["row"][0]) == row
    t0 = time.perf_counter()
    snap.allowed_subjects_raw([kinds[0][1][0][:3] + (0, ALL, 0)], GMD)
    first_ms = (time.perf_counter() - t0) * 1e3
    worst = None
    mism = 0
    for kind, roots in kinds:
        for with_brute, rs, leg in ((True, roots[:1], "one root per call"), (False, roots, f"{a.batch} roots per call")):
            line = case(snap, kind, rs, n_strings, a.reps, a.warmup, with_brute)
            line["leg"] = leg
            print(json.dumps(line), flush=True)
            mism += line.get("mismatches", 0)
            if worst is None or line["composed_over_allowed"] < worst:
                worst = line["composed_over_allowed"]
    line = case(snap, "folder", roots_of("folders", "view", a.many), n_strings, a.reps, a.warmup, False)
    line["leg"] = f"{a.many} roots per call"
    print(json.dumps(line), flush=True)
    worst = min(worst, line["composed_over_allowed"])
    st = snap.stats()
    print(json.dumps({"graph": "config #2 Drive-like", "tuples": int(g.n_edges), "rows": int(g.n_rows), "strings": n_strings,
                      "device_bytes": int(st["device_bytes"]), "global_max_depth": GMD,
                      "first_allowed_call_ms": round(first_ms, 3), "smallest_composed_over_allowed": worst,
                      "mismatches_allowed_vs_brute": mism, "reps": a.reps, "warmup": a.warmup}), flush=True)


if __name__ == "__main__":
    main()
