"""keto_snapshot_delete_query on BASELINE config #2's graph (Drive-like, 10M tuples, tools/synth.py
DRIVE_10M) on one MI355X, the way tools/bench_list.py runs keto_list_batch.  One JSON line per delete
with the library's scan_ms / apply_ms, the wall time, and the mismatches against DeleteAllRelationTuples
restated on SQLite (tests/delete_util.py) over a store holding exactly the tuples the query can match:

  (a) keyed       a fully keyed single-tuple delete (the REST delete of one tuple): the host finds the row
  (b) subject     subject_id only, over the whole graph: once with the device list index not current
                  (host path) and once with it current (device path, the index patched)
  (c) object      a namespace + object delete (device path)
  (d) namespace   a whole-namespace delete with the row cap lifted: the cost per touched row, from which
                  the cost at the default cap (2^20 rows) follows; its counts are compared with the
                  CSR's own (no SQLite store of millions of tuples is built)

and, for comparison, what a delete by query cost before this call existed: the build of the same
graph's snapshot (the rebuild the Go server started) and the list index build the next list call paid.

  python tools/bench_delete_query.py [--threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(msg):
    print(f"[delete {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    from oracle.oracle_sql import _NID, SQLStore, SubjectID
    from tests import delete_util
    from tools import synth

    log("graph")
    g = synth.SynthGraph(dict(synth.DRIVE_10M), threads=a.threads, kind="drive")
    u = g.unified(threads=a.threads)
    t0 = time.perf_counter()
    snap = g.snapshot_unified(u, device=0)
    build_s = time.perf_counter() - t0
    log(f"snapshot of {g.n_edges} tuples, {g.n_rows} rows in {build_s:.1f} s")
    names = dict(g.namespaces)
    rel = g.relation_names()
    obj_s = lambda r: f"{int(g.row_obj[r]):08x}"
    rel_s = lambda r: rel[int(g.row_rel[r])]
    user_s = lambda w: f"u{int(w) - u.user_base:08x}"
    row_ptr = g.row_ptr
    E = int(g.n_edges)
    edge_row = np.repeat(np.arange(g.n_rows), np.diff(row_ptr).astype(np.int64))
    alive = np.ones(E, dtype=bool)
    rng = np.random.default_rng(23)

    def sql_edges(ks):
        out = []
        for k in ks:
            r, e = int(edge_row[k]), int(u.edges[k])
            base = (f"s{k:010d}", _NID, int(g.row_ns[r]), obj_s(r), rel_s(r))
            if e & 0x80000000:
                t = e & 0x7FFFFFFF
                out.append(base + (None, int(g.row_ns[t]), obj_s(t), rel_s(t), int(k)))
            else:
                out.append(base + (user_s(e), None, None, None, int(k)))
        return out

    def run(name, query, mask, candidates=None, note=None):
        """mask: the edges the query matches in the build's CSR; candidates: the edges of the SQLite store
        (a superset of the matches, nothing else the query could match) or None = compare with the CSR."""
        hit = mask & alive
        want = (int(hit.sum()), int(np.unique(edge_row[hit]).size))
        if candidates is not None:
            store = SQLStore(g.namespaces, bulk_rows=sql_edges(np.flatnonzero(candidates & alive)))
            want_sql = delete_util.sql_delete(store, *query)
        else:
            want_sql = want
        n0 = snap.stats()["n_tuples"]
        t0 = time.perf_counter()
        info = snap.delete_query(*delete_util.request(query))
        wall = time.perf_counter() - t0
        alive[hit] = False
        t0 = time.perf_counter()
        raw = snap.list_batch_raw([delete_util.request(query) + (1, 0)])
        list_after = time.perf_counter() - t0
        got = (info["deleted"], info["rows_touched"])
        bad = int(got != want_sql) + int(got != want) + int(int(raw[4][0]) != 0) + int(n0 - snap.stats()["n_tuples"] != want[0])
        line = {"delete": name, "deleted": info["deleted"], "rows_touched": info["rows_touched"],
                "path": ["host", "device"][info["path"]], "index_kept": info["index_kept"],
                "scan_ms": round(info["scan_ms"], 3), "apply_ms": round(info["apply_ms"], 3), "wall_ms": round(wall * 1e3, 3),
                "next_list_call_ms": round(list_after * 1e3, 3), "next_list_index_ms": round(raw[5][0], 3),
                "parity": {"mismatches": bad,
                           "what": ("SQLite store of the tuples the query can match" if candidates is not None else
                                    "the CSR's own counts") + ": deleted, rows_touched; the query lists nothing "
                                   "afterwards; n_tuples fell by `deleted`"}}
        if note:
            line["note"] = note
        print(json.dumps(line), flush=True)
        return info

    ids = u.edges[(u.edges & 0x80000000) == 0]
    users = np.unique(rng.choice(ids, size=64))

    # ---- (a) a fully keyed single-tuple delete; no list call has been made: no index exists
    k = int(rng.choice(np.flatnonzero((u.edges & 0x80000000) == 0)))
    r = int(edge_row[k])
    run("(a) keyed: namespace + object + relation + subject id, no list index yet",
        (names[int(g.row_ns[r])], obj_s(r), rel_s(r), SubjectID(user_s(u.edges[k]))),
        (edge_row == r) & (u.edges == u.edges[k]), edge_row == r)
    # ---- (b) subject id only, host path: the list call after (a) built the index, a write makes it stale
    row = (int(g.row_ns[r]), "zz-bench", rel_s(r), "zz-bench")
    snap.apply([row], [row])                                   # a tuple nobody holds, inserted and deleted
    run("(b) subject id only over the whole graph, list index not current", ("", "", "", SubjectID(user_s(users[0]))),
        u.edges == users[0], u.edges == users[0])
    # ---- (b) device path: the list call after the host-path delete rebuilt the index
    run("(b) subject id only over the whole graph, list index current", ("", "", "", SubjectID(user_s(users[1]))),
        u.edges == users[1], u.edges == users[1])
    # ---- (a) again with the index current: the host finds the row, the index is patched
    k = int(rng.choice(np.flatnonzero(alive & ((u.edges & 0x80000000) == 0))))
    r = int(edge_row[k])
    run("(a) keyed, list index current", (names[int(g.row_ns[r])], obj_s(r), rel_s(r), SubjectID(user_s(u.edges[k]))),
        (edge_row == r) & (u.edges == u.edges[k]), edge_row == r)
    # ---- (c) namespace + object
    r = int(rng.choice(g.n_rows))
    same = (g.row_ns == g.row_ns[r]) & (g.row_obj == g.row_obj[r])
    run("(c) namespace + object", (names[int(g.row_ns[r])], obj_s(r), "", None), same[edge_row], same[edge_row])
    # ---- (d) a whole namespace with the cap lifted
    per_ns = {i: int(np.count_nonzero(alive & (g.row_ns[edge_row] == i))) for i, _ in g.namespaces}
    i = min(per_ns, key=lambda x: (per_ns[x] == 0, per_ns[x]))                # the smallest non-empty namespace
    os.environ["KETO_DELETE_QUERY_MAX_ROWS"] = str(2 ** 31)
    info = run("(d) a whole namespace, KETO_DELETE_QUERY_MAX_ROWS lifted", (names[i], "", "", None), g.row_ns[edge_row] == i,
               note="per touched row: the cost at the default cap of 2^20 rows follows from it")
    del os.environ["KETO_DELETE_QUERY_MAX_ROWS"]
    per_row_us = (info["scan_ms"] + info["apply_ms"]) * 1e3 / max(1, info["rows_touched"])
    print(json.dumps({"graph": "config #2 Drive-like", "tuples": E, "rows": int(g.n_rows),
                      "snapshot_build_s": round(build_s, 3),
                      "what": "snapshot_build_s: the build of this graph's snapshot from its CSR (upload included), the "
                              "rebuild a delete by query started before; the build code is the parent commit's",
                      "per_touched_row_us": round(per_row_us, 3),
                      "derived_at_default_cap_ms": round(per_row_us * 2 ** 20 / 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
