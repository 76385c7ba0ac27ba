"""keto_subjects_batch_ids on one MI355X next to the path a caller had to compose before it existed.

  leg 1   BASELINE config #5's workload: the 100k roots tools/bench_configs.py draws on the config #3 graph
          (nested groups, 100M tuples), request depth 0 at global max-depth 5
  leg 2   one root with as many id leaves as the config #2 graph (Drive-like, 10M tuples) offers: of its
          --candidates rows of highest degree, the one whose tree at max-depth 5 has the most SubjectID leaves
          (that graph's largest group: 265,915 members)
  leg 3   one root with 1.6M id leaves: a hub of 4 groups of 400,000 members each, drawn from one pool of
          10^6 users (loaded with keto_snapshot_from_csr) -- the radix-sorted class at scale, its leaves four
          ascending runs with duplicates across them

Per leg one JSON line with the wall times (median, min and max of --reps calls after --warmup unreported
ones, the paths alternating in every repetition) of

  subjects   keto_subjects_batch_ids at page size 2^31: everything stays on the device, 4 B per distinct id
             of the page come home
  composed   keto_expand_batch_ids (the node arena crosses PCIe) + the vectorised numpy flatten of
             tests/subjects_util.py's yardstick (B): unique of (tree << 32 | id-leaf word).  The per-tree node
             counts it needs are gathered outside the timed window (100k ctypes calls a C caller would not
             pay), which favours this path
  expand     keto_expand_batch_ids alone
  proto      keto_expand_encode_batch_ids (protobuf) alone

the library's HIP-event times of the flatten per stage (keto_subjects_stages: compact, the wave, block and
radix-sorted classes, emit; medians) and of its expand half (host wall), and the mismatches between the
two answers (ids, in order, and the totals), which must be 0.

  python tools/bench_subjects.py [--reps 9] [--warmup 2] [--threads 16] [--candidates 16] [--legs 1,2,3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = 2 ** 31
SET = np.uint32(0x80000000)


def log(msg):
    print(f"[subjects {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def summary(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Arena:
    """A keto_expand_batch_ids arena kept open: its nodes as one numpy view."""

    def __init__(self, snap, roots, depths, gmd):
        self.lib, self.a, self.n = snap.lib, C.c_void_p(), len(roots)
        t0 = time.perf_counter()
        rc = self.lib.keto_expand_batch_ids(snap.h, ptr(roots), ptr(depths), C.c_uint32(self.n), C.c_int32(gmd), C.byref(self.a))
        self.ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, self.lib.keto_last_error()

    def counts(self):
        """Per-tree node counts and the address of the first node (untimed: see the module docstring)."""
        cnt, base = np.zeros(self.n, dtype=np.int64), 0
        nn = C.c_uint64()
        for i in range(self.n):
            p = self.lib.keto_tree_nodes(self.a, C.c_uint32(i), C.byref(nn))
            cnt[i] = nn.value
            if nn.value and not base:
                base = C.cast(p, C.c_void_p).value
        return cnt, base

    def free(self):
        self.lib.keto_tree_arena_free(self.a)


def flatten(cnt, base):
    """The numpy flatten of yardstick (B) over a whole arena -> sorted distinct (tree << 32 | word) keys."""
    total = int(cnt.sum())
    if not total:
        return np.zeros(0, dtype=np.uint64)
    nodes = np.frombuffer((C.c_uint32 * (2 * total)).from_address(base), dtype=np.uint32).reshape(-1, 2)
    leaf = ((nodes[:, 1] & SET) != 0) & ((nodes[:, 0] & SET) == 0)
    tree = np.repeat(np.arange(len(cnt), dtype=np.uint64), cnt)[leaf]
    return np.unique((tree << np.uint64(32)) | nodes[leaf, 0].astype(np.uint64))


def leg(snap, name, roots, depths, gmd, reps, warmup):
    n = len(roots)
    sizes, pages = np.full(n, ALL, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    sw, cw, ew, pw, stages, exp_half, flat_ev = [], [], [], [], [], [], []
    got = want = r = None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        r = snap.subjects_ids_raw(roots, depths, sizes, pages, gmd)
        t1 = time.perf_counter()
        ar = Arena(snap, roots, depths, gmd)
        cnt, base = ar.counts()
        t2 = time.perf_counter()
        want = flatten(cnt, base)
        t3 = time.perf_counter()
        ar.free()
        ar2 = Arena(snap, roots, depths, gmd)
        ar2.free()
        t4 = time.perf_counter()
        snap.expand_batch_ids_encoded(roots, depths, gmd, "proto")
        t5 = time.perf_counter()
        if k >= warmup:
            sw.append((t1 - t0) * 1e3)
            cw.append(ar.ms + (t3 - t2) * 1e3)
            ew.append(ar2.ms)
            pw.append((t5 - t4) * 1e3)
            stages.append(r["stages"])
            exp_half.append(r["timing"][0])
            flat_ev.append(r["timing"][1])
    per = np.diff(r["offsets"].astype(np.int64))
    got = (np.repeat(np.arange(n, dtype=np.uint64), per) << np.uint64(32)) | r["ids"].astype(np.uint64)
    bad = 0 if np.array_equal(got, want) else max(1, len(np.setxor1d(got, want)))
    bad += int((r["totals"].astype(np.int64) != per).sum())                    # page size 2^31: the page is everything
    s, c = summary(sw), summary(cw)
    med = lambda xs: summary(xs)["median"]
    names = ("compact", "wave_class", "block_class", "radix_class", "emit")
    return {"leg": name, "roots": n, "global_max_depth": gmd, "nodes": int(cnt.sum()), "id_leaves": int(r["leaves"].sum()),
            "set_leaves": int(r["set_leaves"].sum()), "distinct_ids": int(len(r["ids"])),
            "largest_segment": int(r["leaves"].max()) if n else 0,
            "subjects_wall_ms": s, "composed_wall_ms": c, "expand_alone_wall_ms": summary(ew), "proto_alone_wall_ms": summary(pw),
            "subjects_expand_half_ms": med(exp_half), "flatten_event_ms": med(flat_ev),
            "flatten_stage_event_ms": {nm: med([st[j] for st in stages]) for j, nm in enumerate(names)},
            "composed_over_subjects": round(c["median"] / s["median"], 2) if s["median"] else None,
            "faster_than_composed": bool(s["max"] < c["min"]), "mismatches": bad, "reps": reps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--legs", default="1,2,3")
    ap.add_argument("--hub-groups", type=int, default=4)
    ap.add_argument("--hub-members", type=int, default=400_000)
    ap.add_argument("--hub-pool", type=int, default=1_000_000)
    a = ap.parse_args()
    from tools import synth
    legs = a.legs.split(",")
    if "1" in legs:
        log("config #3 graph")
        g = synth.SynthGraph(dict(synth.NESTED_100M), threads=a.threads, kind="nested", chain=32)
        snap = g.snapshot(device=0)
        rng = np.random.default_rng(5)                                      # tools/bench_configs.py config5's roots
        n = 100_000
        roots = rng.integers(0, g.n_rows, size=n).astype(np.uint32) | SET
        log("leg 1")
        print(json.dumps(leg(snap, "config #5: 100k roots on the config #3 graph", roots, np.zeros(n, dtype=np.int32), 5,
                             a.reps, a.warmup)), flush=True)
        snap.close()
        del g, snap
    if "2" in legs:
        log("config #2 graph")
        g = synth.SynthGraph(dict(synth.DRIVE_10M), threads=a.threads, kind="drive")
        snap = g.snapshot(device=0)
        deg = np.diff(np.asarray(g.row_ptr))
        cand = np.argsort(deg)[::-1][:a.candidates].astype(np.uint32)
        k = len(cand)
        probe = snap.subjects_ids_raw(cand | SET, np.zeros(k, dtype=np.int32), np.ones(k, dtype=np.uint32),
                                      np.zeros(k, dtype=np.uint32), 5)
        best = int(np.argmax(probe["leaves"]))
        log(f"leg 2: row {int(cand[best])} (degree {int(deg[cand[best]])}) has {int(probe['leaves'][best])} id leaves; "
            f"the candidates' leaves: {probe['leaves'].tolist()}")
        one = np.array([cand[best]], dtype=np.uint32) | SET
        print(json.dumps(leg(snap, "one root: the largest tree of the config #2 graph's highest-degree rows", one,
                             np.zeros(1, dtype=np.int32), 5, a.reps, a.warmup)), flush=True)
        snap.close()
    if "3" in legs:
        log("hub graph")
        snap, leaves = hub_snapshot(a.hub_groups, a.hub_members, a.hub_pool)
        one = np.array([0], dtype=np.uint32) | SET
        line = leg(snap, f"one root: a hub of {a.hub_groups} groups x {a.hub_members} members drawn from {a.hub_pool} users",
                   one, np.zeros(1, dtype=np.int32), 5, a.reps, a.warmup)
        assert line["id_leaves"] == leaves, (line["id_leaves"], leaves)
        print(json.dumps(line), flush=True)
        snap.close()


def hub_snapshot(groups, members, pool):
    """One namespace, row 0 = a hub whose tuples are `groups` subject sets, rows 1.. = the groups, each
    `members` distinct user ids drawn (seeded) from a pool of `pool`: the hub's id leaves are `groups`
    ascending runs, unsorted as a whole, with duplicates across the runs (keto_snapshot_from_csr, no strings)."""
    from keto_amd.capi import Snapshot
    rng = np.random.default_rng(23)
    runs = [np.sort(rng.choice(pool, size=members, replace=False)).astype(np.uint32) for _ in range(groups)]
    edges = np.concatenate([np.arange(1, groups + 1, dtype=np.uint32) | SET] + runs)
    row_ptr = np.concatenate([[0, groups], groups + members * np.arange(1, groups + 1)]).astype(np.uint64)
    n_rows = groups + 1
    snap = Snapshot.from_csr([(1, "n")], np.ones(n_rows, dtype=np.int32), np.arange(n_rows, dtype=np.uint32),
                             np.zeros(n_rows, dtype=np.uint32), row_ptr, edges, device=0)
    return snap, groups * members


if __name__ == "__main__":
    main()
