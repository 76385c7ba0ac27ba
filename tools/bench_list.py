"""keto_list_batch on BASELINE config #2's graph (Drive-like, 10M tuples, tools/synth.py DRIVE_10M) on one
MI355X: three batches --

  rows       1,000 one-row queries (namespace + object + relation of sampled rows)
  subjects   100 namespace + subject-id queries (every tuple of a namespace held by one user)
  pages      10 unfiltered namespace pages (page size 100, pages spread over each namespace)

For each batch one JSON line: wall time per batch (best of --reps calls, the first call's index build
reported apart), the library's index_ms / scan_ms, the bytes the scan kernels must read (8 B per entry
of the queries' ranges, 16 B where a row key is compared too, from keto_list_plan) over scan_ms against
the HBM peak -- a lower bound of the kernels' rate, since scan_ms also covers the copies and the scan --
and a parity sample: the same queries through tests/list_util.py on SQLite stores that hold exactly
the tuples those queries can return (the sampled rows; every tuple of the sampled users), tuples, token
and total compared.  The unfiltered pages are compared on their tuples for page 1 (a store of each
namespace's first rows) and on their totals against the CSR's own counts.

  python tools/bench_list.py [--reps 5] [--sample 200] [--threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def log(msg):
    print(f"[list {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def timed(snap, queries, reps):
    first = time.perf_counter()
    raw = snap.list_batch_raw(queries)
    first = time.perf_counter() - first
    best, best_t = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = snap.list_batch_raw(queries)
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, best_t = dt, r[5]
    return raw, first, best, best_t


def scan_bytes(snap, queries):
    total = 0
    for p in snap.list_plan(queries):
        total += (p["hi"] - p["lo"]) * (16 if p["obj"] is not None or p["rel"] is not None else 8)
    return total


def report(name, snap, queries, reps):
    raw, first, best, (index_ms, scan_ms) = timed(snap, queries, reps)
    nbytes = scan_bytes(snap, queries)
    gbs = nbytes / (scan_ms * 1e-3) / 1e9 if scan_ms > 0 else 0.0
    status, offs, tup, nxt, tot, first_t = raw
    return raw, {"batch": name, "queries": len(queries), "tuples_returned": int(offs[-1]),
                 "matches": int(tot.sum()), "statuses": np.bincount(status, minlength=3).tolist(),
                 "first_call_ms": round(first * 1e3, 3), "first_call_index_ms": round(first_t[0], 3),
                 "wall_ms": round(best * 1e3, 3), "index_ms": round(index_ms, 3), "scan_ms": round(scan_ms, 3),
                 "scan_bytes": int(nbytes),
                 "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": round(gbs / HBM_PEAK_GBS, 5),
                              "what": "range bytes / scan_ms (count + scan + emit + copies): a lower bound"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=200, help="queries per batch compared with SQLite")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    from oracle.oracle_sql import _NID, SQLStore, SubjectID
    from tests import list_util
    from tools import synth

    log("graph")
    g = synth.SynthGraph(dict(synth.DRIVE_10M), threads=a.threads, kind="drive")
    u = g.unified(threads=a.threads)
    t0 = time.perf_counter()
    snap = g.snapshot_unified(u, device=0)
    log(f"snapshot of {g.n_edges} tuples, {g.n_rows} rows in {time.perf_counter() - t0:.1f} s")
    names = dict(g.namespaces)
    rel = g.relation_names()
    obj_s = lambda r: f"{int(g.row_obj[r]):08x}"
    rel_s = lambda r: rel[int(g.row_rel[r])]
    user_s = lambda w: f"u{int(w) - u.user_base:08x}"
    rng = np.random.default_rng(11)
    R, E = g.n_rows, g.n_edges
    row_ptr = g.row_ptr

    def sql_edges(pairs):
        """keto_relation_tuples rows of the CSR edges (row, edge index) in `pairs`; commit_time = the
        edge index, so equal tuples keep their stored order."""
        out = []
        for r, k in pairs:
            e = int(u.edges[k])
            base = (f"s{k:010d}", _NID, int(g.row_ns[r]), obj_s(r), rel_s(r))
            if e & 0x80000000:
                t = e & 0x7FFFFFFF
                out.append(base + (None, int(g.row_ns[t]), obj_s(t), rel_s(t), k))
            else:
                out.append(base + (user_s(e), None, None, None, k))
        return out

    def sql_rows(rows):
        return sql_edges((r, k) for r in rows for k in range(int(row_ptr[r]), int(row_ptr[r + 1])))

    def compare(store, queries, got, fields=(0, 1, 2, 3)):
        bad = 0
        for q, gq in zip(queries, got):
            want = list_util.expected(store, q)
            bad += any(gq[f] != want[f] for f in fields)
        return bad

    def decoded(raw, k):
        status, offs, tup, nxt, tot, _ = raw
        dec = snap.decode_list_tuples(tup[: int(offs[k])])
        return [(int(status[i]), dec[int(offs[i]):int(offs[i + 1])], str(int(nxt[i])) if nxt[i] else "", int(tot[i]))
                for i in range(k)]

    # ---- 1,000 one-row queries
    rows = rng.choice(R, size=1000, replace=False)
    q_rows = [(names[int(g.row_ns[r])], obj_s(r), rel_s(r), None, 0, 0) for r in rows]
    raw, line = report("rows: 1000 one-row queries", snap, q_rows, a.reps)
    k = min(a.sample, len(rows))
    store = SQLStore(g.namespaces, bulk_rows=sql_rows(rows[:k]))
    line["parity"] = {"sample": k, "mismatches": compare(store, q_rows[:k], decoded(raw, k)),
                      "what": "SQLite store of the sampled rows' tuples: tuples, token and total"}
    print(json.dumps(line), flush=True)

    # ---- 100 namespace + subject-id queries
    ids = u.edges[(u.edges & 0x80000000) == 0]
    users = np.unique(rng.choice(ids, size=1000))[:100]
    ns_names = [n for _, n in g.namespaces]
    q_sub = [(ns_names[i % len(ns_names)], "", "", SubjectID(user_s(w)), 0, 0) for i, w in enumerate(users)]
    raw, line = report("subjects: 100 namespace + subject-id queries", snap,
                       [list_util.to_request(q) for q in q_sub], a.reps)
    k = min(a.sample, len(users))
    log("parity store of the sampled users' tuples")
    hit = np.flatnonzero(np.isin(u.edges, users[:k]))
    store = SQLStore(g.namespaces, bulk_rows=sql_edges(zip(np.searchsorted(row_ptr, hit, side="right") - 1, hit)))
    line["parity"] = {"sample": k, "mismatches": compare(store, q_sub[:k], decoded(raw, k)),
                      "what": "SQLite store of every tuple held by the sampled users: tuples, token and total"}
    print(json.dumps(line), flush=True)

    # ---- 10 unfiltered namespace pages
    per_ns = {i: int((row_ptr[1:][g.row_ns == i] - row_ptr[:-1][g.row_ns == i]).sum()) for i, _ in g.namespaces}
    q_pages = []
    for j in range(10):
        i, n = g.namespaces[j % len(g.namespaces)]
        pages = max(1, -(-per_ns[i] // 100))
        q_pages.append((n, "", "", None, 100, 1 if j < len(g.namespaces) else 1 + (j * 7919) % pages))
    raw, line = report("pages: 10 unfiltered namespace pages of 100", snap, q_pages, a.reps)
    got = decoded(raw, len(q_pages))
    first_rows = np.concatenate([np.flatnonzero(g.row_ns == i)[:120] for i, _ in g.namespaces])
    store = SQLStore(g.namespaces, bulk_rows=sql_rows(first_rows))
    k = len(g.namespaces)
    line["parity"] = {"sample": len(q_pages),
                      "page1_tuple_mismatches": compare(store, q_pages[:k], got[:k], fields=(0, 1)),
                      "total_mismatches": sum(got[j][3] != per_ns[g.namespaces[j % k][0]] for j in range(len(q_pages))),
                      "what": "page 1 of each namespace against a SQLite store of its first rows (tuples); "
                              "every page's total against the CSR's tuple count of the namespace"}
    print(json.dumps(line), flush=True)
    st = snap.stats()
    print(json.dumps({"graph": "config #2 Drive-like", "tuples": int(E), "rows": int(R),
                      "device_bytes": int(st["device_bytes"]), "list_index_bytes": 8 * (int(E) + 2) + 8 * int(st["n_rows"])}),
          flush=True)


if __name__ == "__main__":
    main()
