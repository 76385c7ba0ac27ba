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

--writes N adds the write leg: N transactions of 100 tuples (60 inserts into stored rows, 30 into rows
the graph does not hold yet, 11 deletes) applied with keto_snapshot_apply, each followed by one one-row
list call, the first after a write, which brings the list index to the new version.  The leg runs on two
snapshots of the graph in the same process, the same transactions in the same order: one with the index
patched from the journal of written rows, one with KETO_LIST_PATCH=0 (the index rebuilt, as before
patching existed).  Per leg one JSON line: that call's index_ms (the library's figure: host merge or
rebuild, staging, upload and splice) and wall time per transaction, keto_list_index_info after the last,
and the call's parity against a SQLite store of the queried rows; then a line with the ratio.
--sweep K1,K2,... follows with single transactions touching K distinct rows each (one insert per row) on
both snapshots, after one unreported 100-row transaction that warms each: where a patch stops paying
against a rebuild (KETO_LIST_PATCH_MAX_ROWS, which the sweep raises to its largest size).
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
    ap.add_argument("--writes", type=int, default=0, help="transactions of the write leg (0: no write leg)")
    ap.add_argument("--sweep", default="", help="rows touched by the sweep's transactions, e.g. 100,10000,1000000")
    a = ap.parse_args()
    from oracle.oracle_sql import _NID, SQLStore, SubjectID
    from tests import list_util
    from tools import synth

    log("graph")
    g = synth.SynthGraph(dict(synth.DRIVE_10M), threads=a.threads, kind="drive")
    u = g.unified(threads=a.threads)
    t0 = time.perf_counter()
    snap = g.snapshot_unified(u, device=0)
    snap0 = snap
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

    def decoded(raw, k, snap=None):
        snap = snap or snap0
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

    if a.writes or a.sweep:
        snap.close()
        write_legs(a, g, u, names, obj_s, rel_s, user_s, sql_rows, decoded)


def write_legs(a, g, u, names, obj_s, rel_s, user_s, sql_rows, decoded):
    from oracle.oracle_sql import RelationTuple, SQLStore, SubjectID
    from tests import list_util
    rng = np.random.default_rng(23)
    R, row_ptr = g.n_rows, g.row_ptr
    key = lambda r: (int(g.row_ns[r]), obj_s(r), rel_s(r))

    def first_id(r):
        """The row's first stored subject id, or None."""
        for k in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            e = int(u.edges[k])
            if not e & 0x80000000:
                return user_s(e)
        return None

    def transaction(i, rows):
        """100 tuples over `rows` (100 distinct stored rows); rows[0] is the row the list call asks for."""
        ins = [key(r) + (f"w{i:05d}-{j:02d}",) for j, r in enumerate(rows[:60])]
        ins += [(int(g.row_ns[r]), "new-" + obj_s(r), rel_s(r), f"w{i:05d}-{j:02d}") for j, r in enumerate(rows[60:90])]
        dels = [key(r) + (first_id(r),) for r in [rows[0]] + list(rows[90:]) if first_id(r) is not None]
        return {"row": int(rows[0]), "ins": ins, "dels": dels}

    def one(snap, store, t, patch):
        """The transaction on the snapshot and, for the queried row, on the store; then the list call."""
        os.environ["KETO_LIST_PATCH"] = "1" if patch else "0"
        t0 = time.perf_counter()
        snap.apply(t["ins"], t["dels"])
        apply_ms = (time.perf_counter() - t0) * 1e3
        ns_id, obj, rel = key(t["row"])
        for x in t["ins"]:
            if x[:3] == (ns_id, obj, rel):
                store.insert_raw(ns_id, obj, rel, x[3], None, None, None)
        for x in t["dels"]:
            if x[:3] == (ns_id, obj, rel):
                store.delete(RelationTuple(names[ns_id], obj, rel, SubjectID(x[3])))
        q = (names[ns_id], obj, rel, None, 0, 0)
        t0 = time.perf_counter()
        raw = snap.list_batch_raw([q])
        wall_ms = (time.perf_counter() - t0) * 1e3
        bad = decoded(raw, 1, snap)[0] != list_util.expected(store, q)
        return {"apply_ms": apply_ms, "wall_ms": wall_ms, "index_ms": raw[5][0], "scan_ms": raw[5][1], "bad": int(bad)}

    def fresh(patch):
        os.environ["KETO_LIST_PATCH"] = "1" if patch else "0"
        s = g.snapshot_unified(u, device=0)
        s.list_batch_raw([("", "", "", None, 1, 0)])            # the index of version 0
        return s

    def summary(xs):
        xs = sorted(xs)
        return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}

    def info_of(snap):
        info = snap.list_index_info()
        return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in info.items()}

    medians = {}
    if a.writes:
        rows = rng.choice(R, size=100 * a.writes, replace=False).reshape(a.writes, 100)
        txns = [transaction(i, rows[i]) for i in range(a.writes)]
        for patch in (True, False):
            log(f"write leg, patching {'on' if patch else 'off'}")
            snap = fresh(patch)
            store = SQLStore(g.namespaces, bulk_rows=sql_rows([t["row"] for t in txns]))
            res = [one(snap, store, t, patch) for t in txns]
            medians[patch] = summary([r["index_ms"] for r in res])["median"]
            print(json.dumps({"leg": "writes: 100-tuple transactions, each followed by a one-row list call",
                              "patching": "on" if patch else "off (KETO_LIST_PATCH=0)", "transactions": len(res),
                              "index_ms": summary([r["index_ms"] for r in res]),
                              "list_call_wall_ms": summary([r["wall_ms"] for r in res]),
                              "scan_ms": summary([r["scan_ms"] for r in res]),
                              "apply_ms": summary([r["apply_ms"] for r in res]),
                              "index_ms_each": [round(r["index_ms"], 3) for r in res],
                              "parity": {"sample": len(res), "mismatches": sum(r["bad"] for r in res),
                                         "what": "the one-row list call after each transaction against a SQLite store "
                                                 "of the queried rows under the same writes"},
                              "index_info_after": info_of(snap)}), flush=True)
            snap.close()
        print(json.dumps({"leg": "writes", "index_ms_median_patched": medians[True], "index_ms_median_rebuilt": medians[False],
                          "rebuilt_over_patched": round(medians[False] / medians[True], 2) if medians[True] else None}),
              flush=True)
    if a.sweep:
        sizes = [int(x) for x in a.sweep.split(",")]
        os.environ["KETO_LIST_PATCH_MAX_ROWS"] = str(max(sizes))    # the bound is what the sweep is about
        snaps = {True: fresh(True), False: fresh(False)}
        perm, at = rng.permutation(R), 100                      # every transaction its own rows
        for patch in (True, False):                             # not reported: each snapshot's first patch or
            warm = {"row": int(perm[0]), "ins": [key(r) + ("warm",) for r in perm[:100]], "dels": []}     # rebuild
            one(snaps[patch], SQLStore(g.namespaces, bulk_rows=sql_rows([warm["row"]])), warm, patch)
        for i, k in enumerate(sizes):
            log(f"sweep: one transaction touching {k} rows")
            rows, at = perm[at:at + k], at + k
            t = {"row": int(rows[0]), "ins": [key(r) + (f"s{i}-{j:07d}",) for j, r in enumerate(rows)], "dels": []}
            line = {"leg": "sweep: one transaction, one insert per touched row", "rows_touched": k}
            for patch in (True, False):
                store = SQLStore(g.namespaces, bulk_rows=sql_rows([t["row"]]))
                # the store holds the row as the graph has it: earlier sweep transactions chose other rows
                r = one(snaps[patch], store, t, patch)
                info = info_of(snaps[patch])
                line["patched" if patch else "rebuilt"] = {
                    "index_ms": round(r["index_ms"], 3), "list_call_wall_ms": round(r["wall_ms"], 3),
                    "apply_ms": round(r["apply_ms"], 3), "parity_mismatches": r["bad"],
                    "dev_patches": info["dev_patches"], "dev_builds": info["dev_builds"],
                    "last_segments": info["last_segments"], "last_staged_entries": info["last_staged_entries"],
                    "last_host_ms": info["last_host_ms"], "last_device_ms": info["last_device_ms"]}
            line["rebuilt_over_patched"] = round(line["rebuilt"]["index_ms"] / line["patched"]["index_ms"], 2) \
                if line["patched"]["index_ms"] else None
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
