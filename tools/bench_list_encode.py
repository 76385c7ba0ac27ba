"""keto_list_encode_batch on BASELINE config #2's graph (Drive-like, 10M tuples, tools/synth.py DRIVE_10M)
on one MI355X, in both encodings, against the path a caller has without it.  Four workloads --

  a  rows       1,000 one-row queries (namespace + object + relation of sampled rows)
  b  objects    1,000 namespace + object queries with 100-tuple pages
  c  subjects   100 namespace + subject-id queries
  d  namespace  one unfiltered query returning every tuple of the largest namespace (page size 2^31 - 1)

Three paths alternate in one process, 2 warm-up rounds and then --reps measured ones (default 9):

  composed      keto_list_batch, then keto_subject_fields twice (size, fill) over the batch's distinct
                references -- each tuple's row and its subject -- which is what gpu.ListBatch does before it
                builds InternalRelationTuple values.  No marshal step is timed (none runs here), which
                favours this path.
  fused, LDS    keto_list_encode_batch with the wave-staged write
  fused, direct keto_list_encode_batch with KETO_LIST_ENC_LDS=0

All three are driven through ctypes straight at the C ABI and leave their results where the library
put them (nothing is copied out inside the timed region).  Per workload and encoding one JSON line:
wall time per call (median of the measured rounds, min and max), the library's scan_ms / encode_ms,
the bytes out and bytes out / encode_ms, and `mismatches`: the fused bodies (both write paths) against
bodies built here from the composed path's strings.

Workload d runs each encoding in a child process of its own.  The library's pinned pool keeps at most
1 GiB of idle blocks and reuses a block only for a request of at least about half its size, so d's two
bodies (814 MB of JSON, 337 MB of protobuf) in one process evict each other's block and every round
times a hipHostMalloc and a hipHostFree of hundreds of MB instead of the call (seen here: 85 ms for the
protobuf call after the JSON rounds).  A fresh process has the steady state of a server that answers
one such query shape: the block is allocated by the first warm-up call and reused afterwards.

  python tools/bench_list_encode.py [--reps 9] [--threads 16] [--skip-d-check]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from keto_amd import capi                                     # noqa: E402
from tests.list_encode_util import go_json_string             # noqa: E402


def log(msg):
    print(f"[list-encode {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def summary(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


class Composed:
    """One keto_list_batch + two keto_subject_fields calls; keeps what the calls returned for the check."""

    def __init__(self, snap, reqs, n):
        self.snap, self.reqs, self.n = snap, reqs, n

    def run(self):
        lib, snap, n = self.snap.lib, self.snap, self.n
        t0 = time.perf_counter()
        h = C.c_void_p()
        capi._check(lib.keto_list_batch(snap.h, self.reqs, C.c_uint32(n), C.byref(h)))
        total = C.c_uint64()
        p = lib.keto_listed_tuples(h, C.byref(total))
        k = total.value
        if k:
            words = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(2 * k,))
            pairs = words.reshape(k, 2)
            refs = np.unique(np.concatenate([pairs[:, 0] | np.uint32(0x80000000), pairs[:, 1]]))
        else:
            pairs, refs = np.zeros((0, 2), dtype=np.uint32), np.zeros(0, dtype=np.uint32)
        m = len(refs)
        lens = np.zeros(max(1, 3 * m), dtype=np.uint32)
        rp, lp = refs.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p)
        size = lib.keto_subject_fields(snap.h, None, rp, C.c_uint64(m), None, C.c_uint64(0), lp)
        text = np.empty(max(1, size), dtype=np.uint8)
        got = lib.keto_subject_fields(snap.h, None, rp, C.c_uint64(m), text.ctypes.data_as(C.c_void_p), C.c_uint64(size), lp)
        dt = time.perf_counter() - t0
        assert size >= 0 and got == size
        sms = C.c_float()
        lib.keto_listed_timing(h, None, C.byref(sms))
        self.last = (h, pairs, refs, lens, text)
        return dt, sms.value

    def release(self):
        self.snap.lib.keto_listed_free(self.last[0])
        self.last = None

    def bodies(self, enc):
        """The bodies of the last call, built from its strings (before release)."""
        lib, n = self.snap.lib, self.n
        h, pairs, refs, lens, text = self.last
        get = lambda f, nbytes, dt: np.frombuffer(C.string_at(f(h), nbytes), dtype=dt)
        status = get(lib.keto_listed_status, n, np.uint8)
        offs = get(lib.keto_listed_offsets, 8 * (n + 1), np.uint64)
        nxt = get(lib.keto_listed_next_page, 8 * n, np.uint64)
        raw = text.tobytes()
        ends = np.cumsum(lens.astype(np.int64))
        index = {int(r): i for i, r in enumerate(refs.tolist())}
        fields = {}

        def strs(ref):
            got = fields.get(ref)
            if got is None:
                i = index[ref]
                e = ends[3 * i:3 * i + 3].tolist()
                b = e[0] - int(lens[3 * i])
                got = fields[ref] = (raw[b:e[0]], raw[e[0]:e[1]], raw[e[1]:e[2]])
            return got
        pairs = pairs.tolist()
        out = []
        for q in range(n):
            if status[q] != 0:
                out.append(b"")
                continue
            page = pairs[int(offs[q]):int(offs[q + 1])]
            token = str(int(nxt[q])).encode() if nxt[q] else b""
            out.append((json_body if enc == "json" else proto_body)(page, strs, token))
        return out


_PLAIN = re.compile(rb'^[ !#-%\'-;=?-\[\]-~]*$')
_ESC = {}


def esc(s):
    r = _ESC.get(s)
    if r is None:
        r = _ESC[s] = b'"' + s + b'"' if _PLAIN.match(s) else go_json_string(s)
    return r


def json_body(page, strs, token):
    parts = []
    for row, sub in page:
        ns, obj, rel = strs(row | 0x80000000)
        head = b'{"namespace":' + esc(ns) + b',"object":' + esc(obj) + b',"relation":' + esc(rel)
        if sub & 0x80000000:
            a, b, c = strs(sub)
            parts.append(head + b',"subject_set":{"namespace":' + esc(a) + b',"object":' + esc(b) + b',"relation":' + esc(c) + b"}}")
        else:
            parts.append(head + b',"subject_id":' + esc(strs(sub)[0]) + b"}")
    return b'{"relation_tuples":[' + b",".join(parts) + b'],"next_page_token":"' + token + b'"}'


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def field(tag, s, keep_empty=False):
    return bytes([tag]) + varint(len(s)) + s if s or keep_empty else b""


def proto_body(page, strs, token):
    parts = []
    for row, sub in page:
        ns, obj, rel = strs(row | 0x80000000)
        if sub & 0x80000000:
            a, b, c = strs(sub)
            s = field(0x12, field(0x0A, a) + field(0x12, b) + field(0x1A, c), keep_empty=True)
        else:
            s = field(0x0A, strs(sub)[0], keep_empty=True)
        parts.append(field(0x0A, field(0x0A, ns) + field(0x12, obj) + field(0x1A, rel) + field(0x22, s, True), True))
    return b"".join(parts) + field(0x12, token)


class Fused:
    def __init__(self, snap, reqs, n, enc, lds):
        self.snap, self.reqs, self.n, self.enc, self.lds = snap, reqs, n, capi.ENCODINGS[enc], lds

    def run(self):
        lib, snap = self.snap.lib, self.snap
        os.environ["KETO_LIST_ENC_LDS"] = "1" if self.lds else "0"
        t0 = time.perf_counter()
        h = C.c_void_p()
        capi._check(lib.keto_list_encode_batch(snap.h, self.reqs, C.c_uint32(self.n), C.c_uint32(self.enc), C.byref(h)))
        total = C.c_uint64()
        lib.keto_list_encoded_bytes(h, C.byref(total))
        dt = time.perf_counter() - t0
        ims, sms, ems = C.c_float(), C.c_float(), C.c_float()
        lib.keto_list_encoded_timing(h, C.byref(ims), C.byref(sms), C.byref(ems))
        self.last = h
        return dt, sms.value, ems.value, total.value

    def bodies(self):
        lib, n, h = self.snap.lib, self.n, self.last
        total = C.c_uint64()
        p = lib.keto_list_encoded_bytes(h, C.byref(total))
        raw = C.string_at(p, total.value) if total.value else b""
        offs = np.frombuffer(C.string_at(lib.keto_list_encoded_offsets(h), 8 * (n + 1)), dtype=np.uint64).tolist()
        return [raw[offs[i]:offs[i + 1]] for i in range(n)]

    def release(self):
        t0 = time.perf_counter()
        self.snap.lib.keto_list_encoded_free(self.last)
        self.last = None
        return time.perf_counter() - t0


def bench(name, snap, queries, reps, check=True, encodings=("json", "proto")):
    keep = capi._Keep()
    n = len(queries)
    reqs = snap._list_reqs(keep, queries)
    for enc in encodings:
        comp = Composed(snap, reqs, n)
        fused = {"lds": Fused(snap, reqs, n, enc, True), "direct": Fused(snap, reqs, n, enc, False)}
        t = {"composed": [], "lds": [], "direct": []}
        lib_ms = {"composed": [], "lds": [], "direct": []}
        mismatches, out_bytes, tuples = 0, 0, 0
        for rnd in range(2 + reps):
            last = rnd == 1 + reps
            dt, sms = comp.run()
            want = comp.bodies(enc) if last and check else None
            tuples = len(comp.last[1])
            comp.release()
            if rnd >= 2:
                t["composed"].append(dt * 1e3)
                lib_ms["composed"].append((sms, 0.0))
            for path, f in fused.items():
                dt, sms, ems, out_bytes = f.run()
                if want is not None:
                    mismatches += sum(a != b for a, b in zip(f.bodies(), want))
                dt += f.release()
                if rnd >= 2:
                    t[path].append(dt * 1e3)
                    lib_ms[path].append((sms, ems))
        line = {"workload": name, "encoding": enc, "queries": n, "tuples": tuples, "bytes_out": out_bytes,
                "rounds": reps, "mismatches": mismatches if check else None,
                "composed": {"wall_ms": summary(t["composed"]), "scan_ms": summary([x[0] for x in lib_ms["composed"]])}}
        for path in ("lds", "direct"):
            ems = summary([x[1] for x in lib_ms[path]])
            line["fused_" + path] = {"wall_ms": summary(t[path]), "scan_ms": summary([x[0] for x in lib_ms[path]]),
                                     "encode_ms": ems,
                                     "encode_GBs": round(out_bytes / (ems["median"] * 1e-3) / 1e9, 2) if ems["median"] else None}
        c, spread = line["composed"]["wall_ms"], None
        spread = c["max"] - c["min"]
        for path in ("lds", "direct"):
            f = line["fused_" + path]["wall_ms"]
            line["fused_" + path]["composed_over_fused"] = round(c["median"] / f["median"], 2) if f["median"] else None
            line["fused_" + path]["wins_by_more_than_composed_spread"] = bool(c["median"] - f["median"] > spread)
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-d-check", action="store_true", help="do not build workload d's bodies on the host")
    ap.add_argument("--only-d", default="", help="(the tool's own child processes) workload d alone, in this encoding")
    a = ap.parse_args()
    from tools import synth
    import subprocess

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
    R, row_ptr = g.n_rows, g.row_ptr
    snap.list_batch_raw([("", "", "", None, 1, 0)])              # the list index, outside every timing
    snap.list_encode_raw([("", "", "", None, 1, 0)], "json")     # the strings on the device likewise

    deg = (row_ptr[1:] - row_ptr[:-1]).astype(np.int64)
    per_ns = {i: int(deg[g.row_ns == i].sum()) for i, _ in g.namespaces}
    big = max(per_ns, key=per_ns.get)
    if a.only_d:
        bench(f"d: every tuple of the largest namespace ({per_ns[big]} tuples), one query", snap,
              [(names[big], "", "", None, 2 ** 31 - 1, 0)], a.reps, check=not a.skip_d_check, encodings=(a.only_d,))
        return

    rows = rng.choice(R, size=1000, replace=False)
    bench("a: 1000 one-row queries", snap, [(names[int(g.row_ns[r])], obj_s(r), rel_s(r), None, 0, 0) for r in rows], a.reps)
    # objects with the most tuples first, so that the 100-tuple pages are as full as the graph allows
    busy = np.argsort(-deg, kind="stable")[:1000]
    bench("b: 1000 namespace + object queries, pages of 100", snap,
          [(names[int(g.row_ns[r])], obj_s(r), "", None, 100, 0) for r in busy], a.reps)
    ids = u.edges[(u.edges & 0x80000000) == 0]
    users = np.unique(rng.choice(ids, size=1000))[:100]
    ns_names = [n for _, n in g.namespaces]
    bench("c: 100 namespace + subject-id queries", snap,
          [(ns_names[i % len(ns_names)], "", "", ("id", user_s(w)), 0, 0) for i, w in enumerate(users)], a.reps)
    st = snap.stats()
    snap.close()
    # workload d, each encoding in a process of its own, one after the other (see the docstring)
    log(f"workload d: namespace {names[big]!r} holds {per_ns[big]} tuples")
    for enc in ("json", "proto"):
        cmd = [sys.executable, os.path.abspath(__file__), "--only-d", enc, "--reps", str(a.reps), "--threads", str(a.threads)]
        subprocess.run(cmd + (["--skip-d-check"] if a.skip_d_check else []), check=True)
    print(json.dumps({"graph": "config #2 Drive-like", "tuples": int(g.n_edges), "rows": int(R),
                      "device_bytes": int(st["device_bytes"])}), flush=True)


if __name__ == "__main__":
    main()
