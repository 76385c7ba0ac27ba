// ListRelationTuples from the snapshot: keto_list_batch / keto_list_plan.
//
// Replaces, for a batch of queries, sql.(*Persister).GetRelationTuples as a list
// (internal/persistence/sql/relationtuples.go:238-277, paths relative to the reference tree): whereQuery
// (:178-198) with the optional whereSubject (:151-176), the ORDER BY (:250), pop's LIMIT / OFFSET page
// and the COUNT(*) behind the next page token (:262-265), and toInternal over the page (:43-80,
// :268-274).
//
// The list index (per snapshot version, built on the first list call after a write):
//   T[]     8-B entries {row id, subject word} of every tuple in the global ORDER BY: the tuple rows
//           (keys without an ANY field; materialized wildcard rows are views and stay out) in key
//           order -- Snapshot::rows_in_key_order -- and inside a row its full ORDER BY sequence,
//           duplicates and EDGE_POISON markers included (Snapshot::row_edges).  On the device.
//   keys[]  per row id {object string id, relation string id}: what a scan compares when the entry
//           range alone does not imply the filter.  On the device.
//   ord[], first[]  the tuple rows in key order and the first entry of each: the resolver's binary
//           searches.  On the host (no kernel reads them).
// A query resolves to an entry range [lo, hi) -- a namespace filter is always a contiguous run of
// ord, namespace + object a narrower one, all three one row -- and the predicates left over (object
// or relation without the fields before it, the subject word).  The scan is a filtered, ordered
// stream compaction of that range:
//   list_count  one 256-thread block per (query, tile) item, each wave a quarter of the tile, 16-B
//               loads of two entries per lane, matches counted with 64-bit ballots; writes the item's
//               count and its four wave counts
//   scan        hipcub exclusive sum over the item counts (64-bit); a query's total is the distance
//               between its first item's base and the next query's
//   list_emit   items whose rank range misses the page window exit; the others recompute their
//               matches and store those whose rank = item base + waves before + matches before in
//               the wave falls in the window at out[offset + rank - window start]
// No atomic decides an order: the only atomics OR a per-query poison flag.  One host sync sits between
// the passes (totals -> result sizes, statuses, tokens).
//
// Across writes: keto_snapshot_apply leaves the index stale and notes the rows it changed in a journal
// (list_note_rows).  The first list call after it patches the index: ord / first by a merge of the
// journal's tuple rows (host_patch), T by a splice (device_patch: a segment per changed row, the new
// entries staged and uploaded, list_splice writing a fresh T' from T and the staged block, the part in
// front of the first segment a plain copy), keys[] by the appended rows' keys.  The host half may run
// ahead of the device half (keto_list_plan, a delete's host scan); the journal is always relative to
// the device half.  A journal past KETO_LIST_PATCH_MAX_ROWS rows, KETO_LIST_PATCH=0, a delete that found
// the index stale or a failing patch mean a rebuild of everything, as on the first call.
//
// keto_snapshot_delete_query (DeleteAllRelationTuples, relationtuples.go:225-236) uses the same
// resolver and, when the device index is current, the same passes to find the rows a query touches:
// list_count_heads counts matches and heads (the first match of each row's run: one per touched row)
// and flags poisoned tuples, list_emit_heads writes the heads' row ids.  After the commit a current
// index follows the delete instead of going stale: a new T is built out of place from a copy of
// [0, lo), list_emit_keep over [lo, hi) (the entries that do not match, each moved down by the matches
// before it) and a copy of [hi, N); keys[] stays (a delete adds no row), ord / first are rebuilt on
// the host.  Without a current device index the host scans the candidate rows ord[p0, p1) instead,
// and no index is built for a delete.
//
// keto_lookup_objects_batch (which objects of a namespace does a subject have a relation on; the
// reference would run one SubjectIsAllowed, internal/check/engine.go:116-123, per object) uses the HEAD
// passes too: the heads of a namespace + relation query without a subject are its tuple rows in key
// order, the only objects the check can allow.  lookup_make_reqs turns a chunk of them into row-id check
// requests, device_check_rows decides them into one byte each, and lookup_count / scan / lookup_emit
// compact the allowed ones, in order, into the page -- candidates, requests and decisions stay on the
// device.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_check.hpp"
#include "list.hpp"
#include "parallel.hpp"
#include "snapshot.hpp"

namespace keto {

namespace {

inline std::string_view sv(const keto_str& s) { return std::string_view(s.p ? s.p : "", s.n); }

constexpr uint32_t LIST_THREADS = 256;
constexpr uint32_t LIST_WAVES = LIST_THREADS / 64;
constexpr uint64_t LIST_GROUP_ITEMS = 1ull << 20;   // items per launch (a bigger batch runs in query groups)

struct LQuery {          // what the scan is asked: entries [lo, hi), predicates (ANY: not compared)
    uint64_t lo, hi;
    uint32_t obj, rel, subj, pad;
};
struct LWindow {         // ranks [wlo, whi) of the query's matches go to out[off ...)
    uint64_t wlo, whi, off;
};
struct LItem {
    uint32_t q, tile;
};

struct LBuf {            // a grow-only device buffer
    void* p = nullptr;
    uint64_t cap = 0;
    LBuf() = default;
    LBuf(const LBuf&) = delete;
    LBuf& operator=(const LBuf&) = delete;
    template <class T>
    T* get(uint64_t n) {
        const uint64_t want = std::max<uint64_t>(16, n * sizeof(T));
        if (want > cap) {
            release();
            const hipError_t e = hipMalloc(&p, want + want / 8);
            if (e != hipSuccess) {
                p = nullptr;
                throw Error{KETO_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)};
            }
            cap = want + want / 8;
        }
        return (T*)p;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    ~LBuf() { release(); }
};

// does entry e pass the query's row-key predicates / is it a match
__device__ inline void list_test(const LQuery& Q, const uint2* __restrict__ keys, uint2 e, bool& match, bool& poison) {
    bool k = true;
    if (Q.obj != ANY || Q.rel != ANY) {
        const uint2 key = keys[e.x];
        k = (Q.obj == ANY || key.x == Q.obj) && (Q.rel == ANY || key.y == Q.rel);
    }
    poison = k && e.y == EDGE_POISON;
    match = k && (Q.subj == ANY || e.y == Q.subj);
}

// The two entries a lane holds of the wave's 128-entry step starting at the even entry p0: e0 = p0 +
// 2 lane and e0 + 1, tested when they lie in the wave's range [ws, we).  T is padded to an even
// count, so the 16-B load of a pair whose second entry is past the range stays inside it.
__device__ inline void list_pair(const uint2* __restrict__ T, const uint2* __restrict__ keys, const LQuery& Q,
                                 uint64_t p0, uint32_t lane, uint64_t ws, uint64_t we, uint2& a, uint2& b, bool& m0,
                                 bool& m1, bool& poison) {
    const uint64_t e0 = p0 + 2ull * lane;
    const bool v0 = e0 >= ws && e0 < we, v1 = e0 + 1 >= ws && e0 + 1 < we;
    m0 = m1 = poison = false;
    a = b = make_uint2(0, 0);
    if (v0 || v1) {
        const uint4 w = *reinterpret_cast<const uint4*>(T + e0);
        a = make_uint2(w.x, w.y);
        b = make_uint2(w.z, w.w);
        bool p = false;
        if (v0) {
            list_test(Q, keys, a, m0, p);
            poison = p;
        }
        if (v1) {
            list_test(Q, keys, b, m1, p);
            poison = poison || p;
        }
    }
}

// What an entry has to be for a pass to count or emit it (a compile-time mode of the count and emit
// bodies): MATCH -- the query's predicate (lists); HEAD -- a match that starts its row's run of
// matches: entry i of [lo, hi) matches and (i == lo, or T[i-1] is another row's, or T[i-1] does not
// match) -- key predicates hold for a whole row and equal subject words are adjacent in the ORDER BY,
// so the matches of one row are one contiguous run and the heads are the distinct touched rows, in
// key order; KEEP -- an entry of the range that does not match (what a delete leaves behind).
constexpr int LIST_MATCH = 0, LIST_HEAD = 1, LIST_KEEP = 2;

// is the matching entry e = T[i] a head; prev = T[i-1] when the caller holds it (have_prev)
__device__ inline bool list_head(const LQuery& Q, const uint2* __restrict__ T, uint64_t i, uint2 e, bool m,
                                 bool have_prev, uint2 prev) {
    if (!m) return false;
    if (i == Q.lo) return true;
    const uint2 pv = have_prev ? prev : T[i - 1];
    // the same row passes the same key predicates: only the subject word can differ
    return pv.x != e.x || (Q.subj != ANY && pv.y != Q.subj);
}

// HEADS: the delete scan's form -- also counts the heads (hcnt, hwcnt) and flags any poisoned tuple
// among the tuples matching the key part, subject filter or not (it is a match, or may be one)
template <bool HEADS>
__device__ __forceinline__ void list_count_body(const uint2* __restrict__ T, const uint2* __restrict__ keys,
                                                const LQuery* __restrict__ qs, const LItem* __restrict__ items,
                                                uint32_t tile, uint32_t* __restrict__ cnt, uint32_t* __restrict__ wcnt,
                                                uint32_t* __restrict__ qpoison, uint32_t* __restrict__ hcnt,
                                                uint32_t* __restrict__ hwcnt, uint32_t* wsum, uint32_t* wpoi,
                                                uint32_t* whead) {
    const LItem it = items[blockIdx.x];
    const LQuery Q = qs[it.q];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, quarter = tile / LIST_WAVES;
    const uint64_t ia = Q.lo + (uint64_t)it.tile * tile, ib = min(ia + tile, Q.hi);
    const uint64_t ws = min(ia + (uint64_t)wave * quarter, ib), we = min(ws + quarter, ib);
    uint32_t c = 0, hc = 0;
    bool anyp = false;
    for (uint64_t p0 = ws & ~1ull; p0 < we; p0 += 128) {
        uint2 a, b;
        bool m0, m1, p;
        list_pair(T, keys, Q, p0, lane, ws, we, a, b, m0, m1, p);
        c += __popcll(__ballot(m0)) + __popcll(__ballot(m1));
        if constexpr (HEADS) {
            const uint64_t e0 = p0 + 2ull * lane;
            const bool h0 = list_head(Q, T, e0, a, m0, false, a), h1 = list_head(Q, T, e0 + 1, b, m1, true, a);
            hc += __popcll(__ballot(h0)) + __popcll(__ballot(h1));
        }
        const uint64_t bp = __ballot(p);
        anyp = anyp || bp != 0ull;
    }
    if (lane == 0) {
        wsum[wave] = c;
        wpoi[wave] = anyp ? 1u : 0u;
        if constexpr (HEADS) whead[wave] = hc;
    }
    __syncthreads();
    if (threadIdx.x < LIST_WAVES) {
        wcnt[(uint64_t)blockIdx.x * LIST_WAVES + threadIdx.x] = wsum[threadIdx.x];
        if constexpr (HEADS) hwcnt[(uint64_t)blockIdx.x * LIST_WAVES + threadIdx.x] = whead[threadIdx.x];
    }
    if (threadIdx.x == 0) {
        uint32_t s = 0, p = 0;
        for (uint32_t w = 0; w < LIST_WAVES; ++w) {
            s += wsum[w];
            p |= wpoi[w];
        }
        cnt[blockIdx.x] = s;
        if constexpr (HEADS) {
            uint32_t h = 0;
            for (uint32_t w = 0; w < LIST_WAVES; ++w) h += whead[w];
            hcnt[blockIdx.x] = h;
            if (p) atomicOr(qpoison + it.q, 1u);
        } else {
            // only a subject-filtered query reads it: a poisoned tuple among the tuples matching its
            // namespace, object and relation may be a match the snapshot cannot see
            if (p && Q.subj != ANY) atomicOr(qpoison + it.q, 1u);
        }
    }
}

__global__ void __launch_bounds__(LIST_THREADS)
list_count(const uint2* __restrict__ T, const uint2* __restrict__ keys, const LQuery* __restrict__ qs,
           const LItem* __restrict__ items, uint32_t tile, uint32_t* __restrict__ cnt, uint32_t* __restrict__ wcnt,
           uint32_t* __restrict__ qpoison) {
    __shared__ uint32_t wsum[LIST_WAVES];
    __shared__ uint32_t wpoi[LIST_WAVES];
    list_count_body<false>(T, keys, qs, items, tile, cnt, wcnt, qpoison, nullptr, nullptr, wsum, wpoi, nullptr);
}

__global__ void __launch_bounds__(LIST_THREADS)
list_count_heads(const uint2* __restrict__ T, const uint2* __restrict__ keys, const LQuery* __restrict__ qs,
                 const LItem* __restrict__ items, uint32_t tile, uint32_t* __restrict__ cnt,
                 uint32_t* __restrict__ wcnt, uint32_t* __restrict__ qpoison, uint32_t* __restrict__ hcnt,
                 uint32_t* __restrict__ hwcnt) {
    __shared__ uint32_t wsum[LIST_WAVES];
    __shared__ uint32_t wpoi[LIST_WAVES];
    __shared__ uint32_t whead[LIST_WAVES];
    list_count_body<true>(T, keys, qs, items, tile, cnt, wcnt, qpoison, hcnt, hwcnt, wsum, wpoi, whead);
}

// totals of the group's queries [g0, g0 + nq): the distance between their first items' bases
__global__ void __launch_bounds__(256) list_totals(const uint64_t* __restrict__ base, const uint32_t* __restrict__ ioff,
                                                   uint32_t g0, uint32_t nq, uint64_t* __restrict__ tot) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) tot[g0 + i] = base[ioff[i + 1]] - base[ioff[i]];
}

// MATCH: the list page (above).  HEAD: cnt / wcnt / base are the head counts; the heads' row ids go to
// out, read as uint32_t[].  KEEP: cnt / wcnt / base are the match counts; entry e of [lo, hi) that does
// not match goes to out[W.off + (e - lo) - (matches before e)]: the range with its matches squeezed out.
template <int MODE>
__device__ __forceinline__ void list_emit_body(const uint2* __restrict__ T, const uint2* __restrict__ keys,
                                               const LQuery* __restrict__ qs, const LItem* __restrict__ items,
                                               uint32_t tile, const uint32_t* __restrict__ cnt,
                                               const uint32_t* __restrict__ wcnt, const uint64_t* __restrict__ base,
                                               const uint32_t* __restrict__ ioff, uint32_t g0,
                                               const LWindow* __restrict__ wins, uint2* __restrict__ out, uint64_t out_n,
                                               uint32_t* __restrict__ qpage_poison) {
    const LItem it = items[blockIdx.x];
    const LWindow W = wins[it.q];
    if (W.whi <= W.wlo) return;
    const uint64_t r0 = base[blockIdx.x] - base[ioff[it.q - g0]];        // rank of the item's first match
    if constexpr (MODE != LIST_KEEP)
        if (r0 + cnt[blockIdx.x] <= W.wlo || r0 >= W.whi) return;
    const LQuery Q = qs[it.q];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, quarter = tile / LIST_WAVES;
    const uint64_t ia = Q.lo + (uint64_t)it.tile * tile, ib = min(ia + tile, Q.hi);
    const uint64_t ws = min(ia + (uint64_t)wave * quarter, ib), we = min(ws + quarter, ib);
    uint64_t r = r0;
    for (uint32_t w = 0; w < wave; ++w) r += wcnt[(uint64_t)blockIdx.x * LIST_WAVES + w];
    if constexpr (MODE != LIST_KEEP)
        if (r + wcnt[(uint64_t)blockIdx.x * LIST_WAVES + wave] <= W.wlo) return;    // the wave's matches miss the window
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint64_t p0 = ws & ~1ull; p0 < we && (MODE == LIST_KEEP || r < W.whi); p0 += 128) {
        uint2 a, b;
        bool m0, m1, p;
        list_pair(T, keys, Q, p0, lane, ws, we, a, b, m0, m1, p);
        if constexpr (MODE == LIST_HEAD) {
            const uint64_t e0 = p0 + 2ull * lane;
            const bool h0 = list_head(Q, T, e0, a, m0, false, a), h1 = list_head(Q, T, e0 + 1, b, m1, true, a);
            m0 = h0;
            m1 = h1;
        }
        const uint64_t b0 = __ballot(m0), b1 = __ballot(m1);
        const uint64_t k0 = r + __popcll(b0 & below) + __popcll(b1 & below), k1 = k0 + (m0 ? 1u : 0u);
        if constexpr (MODE == LIST_KEEP) {
            const uint64_t e0 = p0 + 2ull * lane;
            if (!m0 && e0 >= ws && e0 < we) {
                const uint64_t at = W.off + (e0 - Q.lo) - k0;
                if (at < out_n) out[at] = a;
            }
            if (!m1 && e0 + 1 >= ws && e0 + 1 < we) {
                const uint64_t at = W.off + (e0 + 1 - Q.lo) - k1;
                if (at < out_n) out[at] = b;
            }
        } else {
            if (m0 && k0 >= W.wlo && k0 < W.whi) {
                const uint64_t at = W.off + (k0 - W.wlo);
                if constexpr (MODE == LIST_HEAD) {
                    if (at < out_n) reinterpret_cast<uint32_t*>(out)[at] = a.x;
                } else {
                    if (at < out_n) out[at] = a;
                    if (a.y == EDGE_POISON) atomicOr(qpage_poison + it.q, 1u);
                }
            }
            if (m1 && k1 >= W.wlo && k1 < W.whi) {
                const uint64_t at = W.off + (k1 - W.wlo);
                if constexpr (MODE == LIST_HEAD) {
                    if (at < out_n) reinterpret_cast<uint32_t*>(out)[at] = b.x;
                } else {
                    if (at < out_n) out[at] = b;
                    if (b.y == EDGE_POISON) atomicOr(qpage_poison + it.q, 1u);
                }
            }
        }
        r += __popcll(b0) + __popcll(b1);
    }
}

#define LIST_EMIT_KERNEL(NAME, MODE)                                                                                  \
    __global__ void __launch_bounds__(LIST_THREADS)                                                                   \
    NAME(const uint2* __restrict__ T, const uint2* __restrict__ keys, const LQuery* __restrict__ qs,                  \
         const LItem* __restrict__ items, uint32_t tile, const uint32_t* __restrict__ cnt,                            \
         const uint32_t* __restrict__ wcnt, const uint64_t* __restrict__ base, const uint32_t* __restrict__ ioff,     \
         uint32_t g0, const LWindow* __restrict__ wins, uint2* __restrict__ out, uint64_t out_n,                      \
         uint32_t* __restrict__ qpage_poison) {                                                                       \
        list_emit_body<MODE>(T, keys, qs, items, tile, cnt, wcnt, base, ioff, g0, wins, out, out_n, qpage_poison);    \
    }
LIST_EMIT_KERNEL(list_emit, LIST_MATCH)
LIST_EMIT_KERNEL(list_emit_heads, LIST_HEAD)
LIST_EMIT_KERNEL(list_emit_keep, LIST_KEEP)
#undef LIST_EMIT_KERNEL

// ---- keto_lookup_objects_batch: the candidates of a query are the HEAD pass's rows (above); what
// follows turns them into check requests and compacts the allowed ones, in order, into the page.
struct LSubj {           // the subject of a lookup query in the row-id form of keto_check_ids
    uint32_t target, flags;
    int32_t max_depth;
    uint32_t pad;
};

// The 16-B requests of candidates [c0, c0 + m) of cand[] (query-major): a candidate's query is the
// last one whose first candidate qoff[q] is at or before it (empty queries share their successor's
// offset and are passed over).  One 16-B store per lane.
__global__ void __launch_bounds__(LIST_THREADS)
lookup_make_reqs(const uint32_t* __restrict__ cand, const uint64_t* __restrict__ qoff, uint32_t nq,
                 const LSubj* __restrict__ subj, uint64_t c0, uint32_t m, uint4* __restrict__ reqs) {
    const uint32_t i = blockIdx.x * LIST_THREADS + threadIdx.x;
    if (i >= m) return;
    const uint64_t g = c0 + i;
    uint32_t lo = 0, hi = nq;                              // qoff[lo] <= g; qoff[hi] > g or hi == nq
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (qoff[mid] <= g) lo = mid;
        else hi = mid;
    }
    const LSubj s = subj[lo];
    reqs[i] = make_uint4(cand[g], s.target, s.flags, (uint32_t)s.max_depth);
}

// The four decisions a lane holds of the wave's 256-candidate step starting at the 4-aligned p0:
// bytes e0 = p0 + 4 lane .. e0 + 3, those inside the wave's range [ws, we) as bit k of `allowed`
// (decision 1) and `undecided` (KETO_UNDECIDED).  dec[] is padded, so the 4-B load of a word whose
// last bytes are past the range stays inside it.
__device__ inline void lookup_quad(const uint8_t* __restrict__ dec, uint64_t p0, uint32_t lane, uint64_t ws, uint64_t we,
                                   uint32_t& allowed, uint32_t& undecided) {
    const uint64_t e0 = p0 + 4ull * lane;
    allowed = undecided = 0;
    if (e0 < we && e0 + 4 > ws) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(dec + e0);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t e = e0 + k;
            if (e < ws || e >= we) continue;
            const uint32_t b = (w >> (8 * k)) & 0xFFu;
            allowed |= (b == 1u ? 1u : 0u) << k;
            undecided |= (b == KETO_UNDECIDED ? 1u : 0u) << k;
        }
    }
}

// the wave's range of candidates of item `it`: a quarter of the tile [ia, ib) of the query's candidates
__device__ inline void lookup_range(const uint64_t* __restrict__ qoff, const LItem& it, uint32_t tile, uint32_t wave,
                                    uint64_t& ws, uint64_t& we) {
    const uint32_t quarter = tile / LIST_WAVES;
    const uint64_t ia = qoff[it.q] + (uint64_t)it.tile * tile, ib = min(ia + tile, qoff[it.q + 1]);
    ws = min(ia + (uint64_t)wave * quarter, ib);
    we = min(ws + quarter, ib);
}

// one block per (query, tile of its candidates): the allowed decisions of the item and of its four
// waves; undecided ones are added to the query's counter (a count, no order hangs on it)
__global__ void __launch_bounds__(LIST_THREADS)
lookup_count(const uint8_t* __restrict__ dec, const uint64_t* __restrict__ qoff, const LItem* __restrict__ items,
             uint32_t tile, uint32_t* __restrict__ cnt, uint32_t* __restrict__ wcnt,
             unsigned long long* __restrict__ qund) {
    __shared__ uint32_t wsum[LIST_WAVES];
    __shared__ uint32_t wund[LIST_WAVES];
    const LItem it = items[blockIdx.x];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t ws, we;
    lookup_range(qoff, it, tile, wave, ws, we);
    uint32_t c = 0, u = 0;
    for (uint64_t p0 = ws & ~3ull; p0 < we; p0 += 256) {
        uint32_t a, d;
        lookup_quad(dec, p0, lane, ws, we, a, d);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) c += __popcll(__ballot((a >> k) & 1u));
        if (__ballot(d != 0u) != 0ull) {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) u += __popcll(__ballot((d >> k) & 1u));
        }
    }
    if (lane == 0) {
        wsum[wave] = c;
        wund[wave] = u;
    }
    __syncthreads();
    if (threadIdx.x < LIST_WAVES) wcnt[(uint64_t)blockIdx.x * LIST_WAVES + threadIdx.x] = wsum[threadIdx.x];
    if (threadIdx.x == 0) {
        uint32_t s = 0, un = 0;
        for (uint32_t w = 0; w < LIST_WAVES; ++w) {
            s += wsum[w];
            un += wund[w];
        }
        cnt[blockIdx.x] = s;
        if (un) atomicAdd(qund + it.q, (unsigned long long)un);
    }
}

// items whose rank range misses the query's window exit; the others recompute their decisions and
// store the candidates whose rank = item base + waves before + allowed before in the wave falls in
// the window at out[offset + rank - window start].  A lane's four candidates follow one another, so
// the allowed ones before a lane's k-th are those of the lower lanes (all four bits) and its own
// lower bits.
__global__ void __launch_bounds__(LIST_THREADS)
lookup_emit(const uint8_t* __restrict__ dec, const uint32_t* __restrict__ cand, const uint64_t* __restrict__ qoff,
            const LItem* __restrict__ items, uint32_t tile, const uint32_t* __restrict__ cnt,
            const uint32_t* __restrict__ wcnt, const uint64_t* __restrict__ base, const uint32_t* __restrict__ ioff,
            const LWindow* __restrict__ wins, uint32_t* __restrict__ out, uint64_t out_n) {
    const LItem it = items[blockIdx.x];
    const LWindow W = wins[it.q];
    if (W.whi <= W.wlo) return;
    const uint64_t r0 = base[blockIdx.x] - base[ioff[it.q]];
    if (r0 + cnt[blockIdx.x] <= W.wlo || r0 >= W.whi) return;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t ws, we;
    lookup_range(qoff, it, tile, wave, ws, we);
    uint64_t r = r0;
    for (uint32_t w = 0; w < wave; ++w) r += wcnt[(uint64_t)blockIdx.x * LIST_WAVES + w];
    if (r + wcnt[(uint64_t)blockIdx.x * LIST_WAVES + wave] <= W.wlo) return;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint64_t p0 = ws & ~3ull; p0 < we && r < W.whi; p0 += 256) {
        uint32_t a, d;
        lookup_quad(dec, p0, lane, ws, we, a, d);
        uint64_t k0 = r;
        uint32_t step = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t b = __ballot((a >> k) & 1u);
            k0 += __popcll(b & below);
            step += __popcll(b);
        }
        const uint64_t e0 = p0 + 4ull * lane;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (!((a >> k) & 1u)) continue;
            const uint64_t rank = k0 + __popc(a & ((1u << k) - 1u));
            if (rank >= W.wlo && rank < W.whi) {
                const uint64_t at = W.off + (rank - W.wlo);
                if (at < out_n) out[at] = cand[e0 + k];
            }
        }
        r += step;
    }
}

// One changed tuple row of a splice: its entries [old_pos, old_pos + old_len) of T become
// [new_pos, new_pos + new_len) of T', taken from the staged block at `staged`.  A new row has
// old_len = 0 at its insertion point, a row that left the index new_len = 0.  Sorted by position (old
// and new alike: the rows between two segments keep their entries and their order).
struct LSeg {
    uint64_t old_pos, old_len, new_pos, new_len, staged;
};

// T'[base, newN), base = the first segment's position: one block per tile of output entries.  Entry j
// belongs to the last segment s whose new_pos is at or before it (of several segments at one position
// only the last can have entries): inside s's new extent it is a staged entry, behind it the entry of
// T as far behind s's old extent.  The block narrows the segments of its tile by two binary searches,
// a lane searches only those; 8-B accesses, consecutive lanes on consecutive entries on both sides
// (old and new positions differ by any count, odd ones included, so nothing wider is assumed).
__global__ void __launch_bounds__(LIST_THREADS)
list_splice(const uint2* __restrict__ T, uint64_t old_n, const LSeg* __restrict__ segs, uint32_t nseg,
            const uint2* __restrict__ staged, uint64_t staged_n, uint64_t base, uint32_t tile, uint2* __restrict__ out,
            uint64_t new_n) {
    const uint64_t ja = base + (uint64_t)blockIdx.x * tile;
    if (ja >= new_n || nseg == 0) return;
    const uint64_t jb = min(ja + tile, new_n);
    uint32_t lo = 0, hi = nseg;                             // segs[lo].new_pos <= ja: segs[0].new_pos == base
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (segs[mid].new_pos <= ja) lo = mid;
        else hi = mid;
    }
    const uint32_t s_lo = lo;
    hi = nseg;                                              // the last segment starting inside the tile, or s_lo
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (segs[mid].new_pos < jb) lo = mid;
        else hi = mid;
    }
    const uint32_t s_hi = lo;
    for (uint64_t j = ja + threadIdx.x; j < jb; j += LIST_THREADS) {
        uint32_t a = s_lo, b = s_hi + 1;
        while (b - a > 1) {
            const uint32_t mid = a + (b - a) / 2;
            if (segs[mid].new_pos <= j) a = mid;
            else b = mid;
        }
        const LSeg g = segs[a];
        const uint64_t ne = g.new_pos + g.new_len;
        uint2 v = make_uint2(0, 0);
        if (j < ne) {
            const uint64_t at = g.staged + (j - g.new_pos);
            if (at < staged_n) v = staged[at];
        } else {
            const uint64_t at = g.old_pos + g.old_len + (j - ne);
            if (at < old_n) v = T[at];
        }
        out[j] = v;
    }
}

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() {
        HIP_OK(hipEventCreate(&a));
        if (hipEventCreate(&b) != hipSuccess) {
            (void)hipEventDestroy(a);
            throw Error{KETO_E_HIP, "hipEventCreate"};
        }
    }
    ~EventPair() {
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
    }
};

uint32_t list_tile() {
    const char* e = getenv("KETO_LIST_TILE");
    if (!e) return 4096;
    const long v = atol(e);
    if (v < 256 || v > (1l << 20) || v % 256 != 0)
        throw Error{KETO_E_INVALID, "KETO_LIST_TILE must be a multiple of 256 in [256, 2^20]"};
    return (uint32_t)v;
}

}  // namespace

struct ListState {
    // host part (any snapshot): the tuple rows in key order and their first entries
    bool host_built = false;
    uint64_t version = ~0ull;
    std::vector<uint32_t> ord;
    std::vector<uint64_t> first;     // ord.size() + 1
    // device part: T of dev_n entries and keys[] of keys_n rows (keys_cap allocated), of dev_version
    int device = -1;
    bool dev_built = false;
    uint64_t dev_version = ~0ull;
    uint64_t dev_n = 0, keys_n = 0, keys_cap = 0;
    uint2* T = nullptr;
    uint2* keys = nullptr;
    uint64_t bytes = 0;
    float build_ms = 0;
    hipStream_t stream = nullptr;
    LBuf qs, items, ioff, cnt, wcnt, base, tot, qpoison, qpage, wins, out, tmp;
    LBuf hcnt, hwcnt, hbase;         // the delete scan's head counts (keto_snapshot_delete_query)
    LBuf segs, staged;               // the splice's segment table and new entries
    // keto_lookup_objects_batch: candidates (4 B each) and their decisions (1 B each), a chunk's check
    // requests (16 B each), the queries' candidate offsets, subjects and undecided counts
    LBuf lk_cand, lk_dec, lk_reqs, lk_qoff, lk_subj, lk_und;
    hipEvent_t lk_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // a lookup's phase marks on `stream`
    // a big lookup's candidate, decision and request buffers do not linger (as the splice's upload buffers)
    void lookup_trim() {
        for (LBuf* b : {&lk_cand, &lk_dec, &lk_reqs})
            if (b->cap > (256ull << 20)) b->release();
    }
    // The device half may lag the host half (a keto_list_plan or a delete's host scan patched the host
    // half first): then dev_ord / dev_first are the ord / first T was built from, moved here by that
    // patch.  Otherwise ord / first describe T.
    bool dev_desc = false;
    std::vector<uint32_t> dev_ord;
    std::vector<uint64_t> dev_first;
    // The journal: rows written since dev_version (since `version` without a device half), complete up to
    // the snapshot version j_upto.  Appended raw by writers, deduplicated by journal_settle; [0, j_mark)
    // is sorted and distinct.
    bool j_valid = false;
    uint64_t j_upto = 0;
    size_t j_mark = 0;
    std::vector<uint32_t> journal;
    // keto_list_index_info
    uint64_t host_builds = 0, host_patches = 0, dev_builds = 0, dev_patches = 0;
    uint64_t last_segments = 0, last_staged = 0;
    float last_host_ms = 0, last_device_ms = 0;
    void free_index() {
        if (T) (void)hipFree(T);
        if (keys) (void)hipFree(keys);
        T = keys = nullptr;
        bytes = 0;
        dev_n = keys_n = keys_cap = 0;
        dev_built = false;
        drop_dev_desc();
    }
    void drop_dev_desc() {
        dev_desc = false;
        std::vector<uint32_t>().swap(dev_ord);
        std::vector<uint64_t>().swap(dev_first);
    }
    void journal_reset(bool valid, uint64_t upto) {
        j_valid = valid;
        j_upto = upto;
        j_mark = 0;
        std::vector<uint32_t>().swap(journal);
    }
    ~ListState() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        free_index();
        for (hipEvent_t x : lk_ev)
            if (x) (void)hipEventDestroy(x);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

void ListStateDeleter::operator()(ListState* l) const { delete l; }

uint64_t list_device_bytes(ListCache& C) {
    std::lock_guard<std::mutex> lk(C.mu);
    return C.state ? C.state->bytes : 0;
}

namespace {

void host_tables(const Snapshot& S, ListState& L);
void host_patch(const Snapshot& S, ListState& L);

bool patch_enabled() {
    const char* e = getenv("KETO_LIST_PATCH");
    return !e || atol(e) != 0;
}

// The most distinct rows a journal holds.  Measured on the 10M-tuple graph (4.3M rows,
// profiles/config2_list_patch.log): a patch beats the rebuild 2x to 20x at 100 touched rows, is level
// with it around 10,000 and loses 4x at 10^6; 2^12 stays on the winning side.
uint64_t patch_max_rows() {
    const char* e = getenv("KETO_LIST_PATCH_MAX_ROWS");
    return e ? (uint64_t)std::max(0ll, atoll(e)) : 1ull << 12;
}

// the journal as a sorted set; past the row bound it marks itself invalid and frees its memory
void journal_settle(ListState& L) {
    if (!L.j_valid) return;
    if (L.j_mark != L.journal.size()) {
        std::sort(L.journal.begin(), L.journal.end());
        L.journal.erase(std::unique(L.journal.begin(), L.journal.end()), L.journal.end());
        L.j_mark = L.journal.size();
    }
    if (L.journal.size() > patch_max_rows()) L.journal_reset(false, 0);
}

float ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the caller holds C.mu and S.rw shared
ListState& host_index(const Snapshot& S, ListCache& C) {
    if (!C.state) C.state.reset(new ListState);
    ListState& L = *C.state;
    const uint64_t ver = S.version.load();
    if (L.host_built && L.version == ver) return L;
    const auto t0 = std::chrono::steady_clock::now();
    journal_settle(L);
    if (L.host_built && L.j_valid && L.j_upto == ver && patch_enabled()) {
        host_patch(S, L);                      // the device half follows on the next list_batch, by a splice
    } else {
        L.dev_built = false;                   // the device tables follow on the next list_batch, rebuilt
        L.drop_dev_desc();
        host_tables(S, L);
    }
    L.last_host_ms = ms_since(t0);
    return L;
}

// ord and first of the snapshot as it stands, stamped with its version; the journal starts afresh
void host_tables(const Snapshot& S, ListState& L) {
    const uint64_t ver = S.version.load();
    L.host_built = false;
    L.journal_reset(false, 0);
    L.ord = S.rows_in_key_order(RowKey{ANY_NS, ANY, ANY});
    const uint64_t m = L.ord.size();
    L.first.assign(m + 1, 0);
    const unsigned th = m >= par_min() ? build_threads() : 1u;
    par_chunks(m, th, 1 << 14, [&](uint64_t b, uint64_t e, unsigned) {
        for (uint64_t i = b; i < e; ++i) L.first[i + 1] = S.row_edges(L.ord[i]).second;
    });
    for (uint64_t i = 0; i < m; ++i) L.first[i + 1] += L.first[i];
    L.version = ver;
    L.host_built = true;
    L.host_builds += 1;
    L.journal_reset(patch_enabled(), ver);
}

// is row r one that holds tuples (not a materialized wildcard row), and is it a member of ord now:
// Snapshot::rows_in_key_order's rule
inline bool tuple_row(const Snapshot& S, uint32_t r) {
    if (r < S.n_real_rows) return true;
    const RowKey& k = S.row_key[r];
    return k.ns != ANY_NS && k.obj != ANY && k.rel != ANY;
}
inline bool in_ord(const Snapshot& S, uint32_t r) {
    if (r < S.n_real_rows) return true;
    auto it = S.row_over.find(r);
    return it != S.row_over.end() && !it->second.empty();
}

// the journal's tuple rows in key order (the journal is settled: ascending row ids).  The build's real
// rows are in key order by id; only rows added since need sorting, and one merge joins the two.
std::vector<uint32_t> journal_tuple_rows(const Snapshot& S, const ListState& L) {
    std::vector<uint32_t> real, extra;
    real.reserve(L.journal.size());
    for (uint32_t r : L.journal) {
        if (r >= S.n_rows() || !tuple_row(S, r)) continue;
        (r < S.n_real_rows ? real : extra).push_back(r);
    }
    if (extra.empty()) return real;
    auto less = [&](uint32_t a, uint32_t b) { return S.key_cmp_bytes(S.row_key[a], S.row_key[b]) < 0; };
    std::sort(extra.begin(), extra.end(), less);
    std::vector<uint32_t> jr(real.size() + extra.size());
    std::merge(real.begin(), real.end(), extra.begin(), extra.end(), jr.begin(), less);
    return jr;
}

// Where row r is in ord[from, ...) or would be inserted (row keys never change and are distinct: a
// search by key); found: ord holds it there.  The callers walk the journal in key order, so the place
// is usually near `from`: the search gallops from there before it bisects.
inline uint64_t ord_place(const Snapshot& S, const std::vector<uint32_t>& ord, uint64_t from, uint32_t r, bool& found) {
    const RowKey& k = S.row_key[r];
    auto before = [&](uint64_t i) { return S.key_cmp_bytes(S.row_key[ord[i]], k) < 0; };
    const uint64_t m = ord.size();
    uint64_t lo = from, hi = m;                             // ord[lo - 1] < k (or lo == from), ord[hi] >= k (or hi == m)
    for (uint64_t step = 1; lo < m; step *= 2) {
        const uint64_t probe = std::min(m - 1, lo + step - 1);
        if (!before(probe)) {
            hi = probe;
            break;
        }
        lo = probe + 1;
    }
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (before(mid)) lo = mid + 1;
        else hi = mid;
    }
    found = lo < m && ord[lo] == r;
    return lo;
}

// ord and first brought to the snapshot's version from the journal: every journal row (a superset of
// the rows written since the host half's version) is looked up, or placed, by its key and takes its
// membership and length as they are now; the other rows keep theirs.  Equal to what host_tables builds.
void host_patch(const Snapshot& S, ListState& L) {
    const uint64_t ver = S.version.load();
    const std::vector<uint32_t> jr = journal_tuple_rows(S, L);
    const uint64_t m = L.ord.size();
    std::vector<uint32_t> ord(m + jr.size());
    std::vector<uint64_t> first(m + jr.size() + 1);
    first[0] = 0;
    uint64_t i = 0, k = 0;                                  // old rows taken, new rows written
    auto keep = [&](uint64_t to) {                          // old rows [i, to) as they are, their entries shifted
        if (to == i) return;
        std::copy(L.ord.begin() + i, L.ord.begin() + to, ord.begin() + k);
        const uint64_t shift = first[k] - L.first[i];       // wraps when the entries move down
        const uint64_t* of = L.first.data() + i + 1;
        uint64_t* nf = first.data() + k + 1;
        for (uint64_t j = 0; j < to - i; ++j) nf[j] = of[j] + shift;
        k += to - i;
        i = to;
    };
    for (uint32_t r : jr) {
        bool found;
        const uint64_t p = ord_place(S, L.ord, i, r, found);
        keep(p);
        if (found) ++i;
        if (in_ord(S, r)) {
            ord[k] = r;
            first[k + 1] = first[k] + S.row_edges(r).second;
            ++k;
        }
    }
    keep(m);
    ord.resize(k);
    first.resize(k + 1);
    if (L.dev_built && !L.dev_desc) {                       // what T was built from stays until the splice
        L.dev_ord = std::move(L.ord);
        L.dev_first = std::move(L.first);
        L.dev_desc = true;
    }
    L.ord = std::move(ord);
    L.first = std::move(first);
    L.version = ver;
    L.host_patches += 1;
    if (!L.dev_built) L.journal_reset(true, ver);           // no device half: the journal is relative to the host half
}

// T and keys of the current host index, filled on host threads into pinned staging and uploaded
void device_index(const Snapshot& S, ListState& L, int device) {
    const auto t0 = std::chrono::steady_clock::now();
    L.device = device;
    L.free_index();
    if (!L.stream) HIP_OK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    const uint64_t N = L.first.back(), R = S.n_rows(), m = L.ord.size();
    const uint64_t t_entries = (N + 2) & ~1ull;                       // even, and never empty
    HIP_OK(hipMalloc((void**)&L.T, t_entries * sizeof(uint2)));
    HIP_OK(hipMalloc((void**)&L.keys, std::max<uint64_t>(R, 1) * sizeof(uint2)));
    L.bytes = t_entries * sizeof(uint2) + std::max<uint64_t>(R, 1) * sizeof(uint2);
    HIP_OK(hipMemsetAsync(L.T + N, 0, (t_entries - N) * sizeof(uint2), L.stream));
    const unsigned th = std::max(N, R) >= par_min() ? build_threads() : 1u;
    constexpr uint64_t CHUNK = 1ull << 22;                            // entries per staging block (32 MB)
    struct Staging {
        void* p;
        explicit Staging(uint64_t bytes) : p(pinned_take(bytes)) {}
        ~Staging() { pinned_give(p); }
    } stage(std::min<uint64_t>(CHUNK, std::max<uint64_t>(std::max(N, R), 1)) * sizeof(uint2));
    uint2* h = static_cast<uint2*>(stage.p);
    for (uint64_t c0 = 0; c0 < R; c0 += CHUNK) {
        const uint64_t c1 = std::min(R, c0 + CHUNK);
        par_chunks(c1 - c0, th, 1 << 16, [&](uint64_t b, uint64_t e, unsigned) {
            for (uint64_t r = c0 + b; r < c0 + e; ++r) h[r - c0] = make_uint2(S.row_key[r].obj, S.row_key[r].rel);
        });
        HIP_OK(hipMemcpyAsync(L.keys + c0, h, (c1 - c0) * sizeof(uint2), hipMemcpyHostToDevice, L.stream));
        HIP_OK(hipStreamSynchronize(L.stream));
    }
    for (uint64_t c0 = 0; c0 < N; c0 += CHUNK) {
        const uint64_t c1 = std::min(N, c0 + CHUNK);
        par_chunks(c1 - c0, th, 1 << 16, [&](uint64_t b, uint64_t e, unsigned) {
            uint64_t at = c0 + b;
            const uint64_t end = c0 + e;
            // the row holding entry `at`: the last one whose first entry is at or before it
            uint64_t i = (uint64_t)(std::upper_bound(L.first.begin(), L.first.begin() + m + 1, at) - L.first.begin()) - 1;
            while (at < end) {
                const uint32_t row = L.ord[i];
                const auto ed = S.row_edges(row);
                const uint64_t stop = std::min(end, L.first[i + 1]);
                for (uint64_t k = at - L.first[i]; at < stop; ++at, ++k) h[at - c0] = make_uint2(row, ed.first[k]);
                ++i;
            }
        });
        HIP_OK(hipMemcpyAsync(L.T + c0, h, (c1 - c0) * sizeof(uint2), hipMemcpyHostToDevice, L.stream));
        HIP_OK(hipStreamSynchronize(L.stream));
    }
    HIP_OK(hipStreamSynchronize(L.stream));
    L.dev_built = true;
    L.dev_version = L.version;
    L.dev_n = N;
    L.keys_n = R;
    L.keys_cap = std::max<uint64_t>(R, 1);
    L.dev_builds += 1;
    L.last_device_ms = 0;
    L.journal_reset(L.j_valid, L.version);                  // from here on relative to this T
    L.build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The device half brought from dev_version to the host half's version (which is the snapshot's): the
// segment table of the journal's tuple rows between the two descriptions, the rows' new entries staged
// in one pinned block, a fresh T' = copy of [0, first segment) + list_splice over the rest, and the
// new rows' keys.  T and T' live together until the splice is done.  Throws on any failure, the old
// index untouched: the caller frees it and rebuilds.
void device_patch(const Snapshot& S, ListState& L) {
    const uint32_t tile = list_tile();
    hipStream_t st = L.stream;
    const std::vector<uint32_t> jr = journal_tuple_rows(S, L);
    std::vector<LSeg> segs;
    std::vector<uint32_t> seg_row;
    const uint64_t N = L.dev_first.back(), newN = L.first.back();
    if (N != L.dev_n) throw Error{KETO_E_INVALID, "the list index does not match its description"};
    uint64_t io = 0, in = 0, staged = 0, gone = 0;
    for (uint32_t r : jr) {
        bool fo, fn;
        const uint64_t po = ord_place(S, L.dev_ord, io, r, fo), pn = ord_place(S, L.ord, in, r, fn);
        io = po + (fo ? 1 : 0);
        in = pn + (fn ? 1 : 0);
        const LSeg g{L.dev_first[po], fo ? L.dev_first[po + 1] - L.dev_first[po] : 0, L.first[pn],
                     fn ? L.first[pn + 1] - L.first[pn] : 0, staged};
        if (!g.old_len && !g.new_len) continue;
        // the rows between two segments are the same rows with the same entries: the shift is the same
        if (g.new_pos + gone != g.old_pos + staged) throw Error{KETO_E_INVALID, "the list journal misses a written row"};
        if (fn && S.row_edges(r).second != g.new_len) throw Error{KETO_E_INVALID, "the list index is not of this version"};
        segs.push_back(g);
        seg_row.push_back(r);
        staged += g.new_len;
        gone += g.old_len;
    }
    if (newN + gone != N + staged) throw Error{KETO_E_INVALID, "the list journal misses a written row"};
    const uint64_t R = S.n_rows(), new_keys = R > L.keys_n ? R - L.keys_n : 0, nseg = segs.size();
    if (nseg > 0xFFFFFFF0ull) throw Error{KETO_E_RANGE, "the list journal holds too many rows"};

    // ---- staging: the segments' new entries, then the new rows' keys
    struct Staging {
        void* p;
        explicit Staging(uint64_t bytes) : p(pinned_take(bytes)) {}
        ~Staging() { pinned_give(p); }
    } stage(std::max<uint64_t>(staged + new_keys, 1) * sizeof(uint2));
    uint2* h = static_cast<uint2*>(stage.p);
    const unsigned th = staged >= par_min() ? build_threads() : 1u;
    par_chunks(nseg, th, 64, [&](uint64_t b, uint64_t e, unsigned) {
        for (uint64_t s = b; s < e; ++s) {
            if (!segs[s].new_len) continue;
            const uint32_t row = seg_row[s];
            const auto ed = S.row_edges(row);
            uint2* to = h + segs[s].staged;
            for (uint64_t k = 0; k < segs[s].new_len; ++k) to[k] = make_uint2(row, ed.first[k]);
        }
    });
    for (uint64_t r = L.keys_n; r < R; ++r) h[staged + (r - L.keys_n)] = make_uint2(S.row_key[r].obj, S.row_key[r].rel);

    // ---- device: out of place
    struct Fresh {
        uint2* p = nullptr;
        ~Fresh() {
            if (p) (void)hipFree(p);
        }
    } fresh, fresh_keys;
    const uint64_t t_entries = (newN + 2) & ~1ull, old_entries = (N + 2) & ~1ull;
    EventPair ev;
    HIP_OK(hipEventRecord(ev.a, st));
    uint64_t keys_cap = L.keys_cap;
    if (R > L.keys_cap) {                                   // row ids were appended past the allocation
        keys_cap = R + R / 8 + 1024;
        HIP_OK(hipMalloc((void**)&fresh_keys.p, keys_cap * sizeof(uint2)));
        if (L.keys_n)
            HIP_OK(hipMemcpyAsync(fresh_keys.p, L.keys, L.keys_n * sizeof(uint2), hipMemcpyDeviceToDevice, st));
    }
    uint2* keys = fresh_keys.p ? fresh_keys.p : L.keys;
    if (new_keys)
        HIP_OK(hipMemcpyAsync(keys + L.keys_n, h + staged, new_keys * sizeof(uint2), hipMemcpyHostToDevice, st));
    if (nseg) {
        const uint64_t base = segs[0].new_pos;               // == its old_pos: nothing in front of it moved
        const uint64_t blocks = (newN - base + tile - 1) / tile;
        if (blocks > 0x7FFFFFFFull) throw Error{KETO_E_RANGE, "the list splice spans more than 2^31 tiles"};
        HIP_OK(hipMalloc((void**)&fresh.p, t_entries * sizeof(uint2)));
        HIP_OK(hipMemsetAsync(fresh.p + newN, 0, (t_entries - newN) * sizeof(uint2), st));
        if (base) HIP_OK(hipMemcpyAsync(fresh.p, L.T, base * sizeof(uint2), hipMemcpyDeviceToDevice, st));
        LSeg* d_segs = L.segs.get<LSeg>(nseg);
        uint2* d_staged = L.staged.get<uint2>(staged);
        HIP_OK(hipMemcpyAsync(d_segs, segs.data(), nseg * sizeof(LSeg), hipMemcpyHostToDevice, st));
        if (staged) HIP_OK(hipMemcpyAsync(d_staged, h, staged * sizeof(uint2), hipMemcpyHostToDevice, st));
        if (blocks) {
            hipLaunchKernelGGL(list_splice, dim3((uint32_t)blocks), dim3(LIST_THREADS), 0, st, (const uint2*)L.T, N,
                               (const LSeg*)d_segs, (uint32_t)nseg, (const uint2*)d_staged, staged, base, tile, fresh.p, newN);
            HIP_OK(hipGetLastError());
        }
    }
    HIP_OK(hipEventRecord(ev.b, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipEventElapsedTime(&L.last_device_ms, ev.a, ev.b));
    if (fresh.p) {
        std::swap(L.T, fresh.p);                            // the old T is freed with `fresh`
        L.bytes = L.bytes - old_entries * sizeof(uint2) + t_entries * sizeof(uint2);
    }
    if (fresh_keys.p) {
        std::swap(L.keys, fresh_keys.p);
        L.bytes = L.bytes - L.keys_cap * sizeof(uint2) + keys_cap * sizeof(uint2);
        L.keys_cap = keys_cap;
    }
    L.keys_n = std::max(L.keys_n, R);
    L.dev_n = newN;
    L.dev_version = L.version;
    L.drop_dev_desc();
    L.journal_reset(true, L.version);
    L.dev_patches += 1;
    L.last_segments = nseg;
    L.last_staged = staged;
    if (L.staged.cap > (64ull << 20)) L.staged.release();   // a big patch's upload buffers do not linger
    if (L.segs.cap > (64ull << 20)) L.segs.release();
}

struct Plan {
    LQuery q{0, 0, ANY, ANY, ANY, 0};
    int64_t ns = ANY_NS;
    uint8_t status = KETO_LIST_OK;
    uint64_t p0 = 0, p1 = 0;         // the rows ord[p0, p1) the range is made of
};

// whereQuery + whereSubject against the host tables: statuses, the entry range and the predicates
Plan resolve_list(const Snapshot& S, const ListState& L, const keto_list_req& rq) {
    Plan P;
    const std::string_view ns = sv(rq.namespace_), obj = sv(rq.object), rel = sv(rq.relation);
    if (!ns.empty()) {
        const int c = S.ns_index(ns);
        if (c < 0) {                                     // GetNamespaceByName (:180)
            P.status = KETO_LIST_NOT_FOUND;
            return P;
        }
        P.ns = S.ns_ids[c];
    }
    RowKey sk{ANY_NS, ANY, ANY};                          // a subject set's row key
    if (rq.has_subject && rq.subject.kind != 0) {
        const std::string_view sn = sv(rq.subject.set_namespace);
        const int c = S.ns_index(sn);
        if (c < 0) {                                     // GetNamespaceByName (:161), "" included
            P.status = KETO_LIST_NOT_FOUND;
            return P;
        }
        sk.ns = sn.empty() ? ANY_NS : (int64_t)S.ns_ids[c];   // as the builder keys the target row
    }
    bool empty = false;
    uint32_t o = ANY, r = ANY;
    if (!obj.empty()) {
        const int64_t x = S.lookup_str(obj);
        if (x < 0) empty = true;
        o = (uint32_t)x;
    }
    if (!rel.empty()) {
        const int64_t x = S.lookup_str(rel);
        if (x < 0) empty = true;
        r = (uint32_t)x;
    }
    if (rq.has_subject && !empty) {
        if (rq.subject.kind == 0) {
            const int64_t x = S.lookup_str(sv(rq.subject.id));
            if (x < 0) empty = true;
            P.q.subj = (uint32_t)x;
        } else {
            // an empty object / relation is stored as the target key's ANY field (snapshot.cpp)
            const std::string_view so = sv(rq.subject.set_object), sr = sv(rq.subject.set_relation);
            const int64_t xo = so.empty() ? -2 : S.lookup_str(so), xr = sr.empty() ? -2 : S.lookup_str(sr);
            if (xo == -1 || xr == -1) empty = true;
            else {
                sk.obj = xo == -2 ? ANY : (uint32_t)xo;
                sk.rel = xr == -2 ? ANY : (uint32_t)xr;
                int64_t row = sk.ns != ANY_NS && sk.obj != ANY && sk.rel != ANY ? S.real_row(sk) : -1;
                if (row < 0) {
                    auto it = S.row_of.find(sk);
                    if (it != S.row_of.end()) row = it->second;
                }
                if (row < 0) empty = true;               // no stored subject set names it
                else P.q.subj = EDGE_SET | (uint32_t)row;
            }
        }
    }
    if (empty) return P;                                 // lo == hi == 0
    // the entry range: binary searches over the tuple rows in key order
    uint64_t p0 = 0, p1 = L.ord.size();
    if (P.ns != ANY_NS) {
        auto lo = std::lower_bound(L.ord.begin(), L.ord.end(), P.ns, [&](uint32_t row, int64_t v) { return S.row_key[row].ns < v; });
        auto hi = std::upper_bound(lo, L.ord.end(), P.ns, [&](int64_t v, uint32_t row) { return v < S.row_key[row].ns; });
        p0 = lo - L.ord.begin();
        p1 = hi - L.ord.begin();
        if (o != ANY) {
            auto b = L.ord.begin() + p0, e = L.ord.begin() + p1;
            auto lo2 = std::lower_bound(b, e, o, [&](uint32_t row, uint32_t v) { return S.str_cmp(S.row_key[row].obj, v) < 0; });
            auto hi2 = std::upper_bound(lo2, e, o, [&](uint32_t v, uint32_t row) { return S.str_cmp(v, S.row_key[row].obj) < 0; });
            p0 = lo2 - L.ord.begin();
            p1 = hi2 - L.ord.begin();
            if (r != ANY) {
                auto b3 = L.ord.begin() + p0, e3 = L.ord.begin() + p1;
                auto lo3 = std::lower_bound(b3, e3, r, [&](uint32_t row, uint32_t v) { return S.str_cmp(S.row_key[row].rel, v) < 0; });
                auto hi3 = std::upper_bound(lo3, e3, r, [&](uint32_t v, uint32_t row) { return S.str_cmp(v, S.row_key[row].rel) < 0; });
                p0 = lo3 - L.ord.begin();
                p1 = hi3 - L.ord.begin();
            }
        } else if (r != ANY) {
            P.q.rel = r;
        }
    } else {
        P.q.obj = o;
        P.q.rel = r;
    }
    P.q.lo = L.first[p0];
    P.q.hi = L.first[p1];
    P.p0 = p0;
    P.p1 = p1;
    if (P.q.lo == P.q.hi) P.q.lo = P.q.hi = 0, P.q.obj = P.q.rel = ANY, P.p0 = P.p1 = 0;
    return P;
}

}  // namespace

void list_plan(const Snapshot& S, ListCache& C, const keto_list_req* reqs, uint32_t n, keto_list_plan_t* out) {
    const ListState* L;
    {
        std::lock_guard<std::mutex> lk(C.mu);
        L = &host_index(S, C);
    }
    // the index of this version is not rebuilt while the caller holds the snapshot's lock shared
    const unsigned th = n >= 4096 ? build_threads() : 1u;
    par_chunks(n, th, 1024, [&](uint64_t b, uint64_t e, unsigned) {
        for (uint64_t i = b; i < e; ++i) {
            const Plan P = resolve_list(S, *L, reqs[i]);
            out[i] = keto_list_plan_t{P.q.lo, P.q.hi, P.ns, P.q.obj, P.q.rel, P.q.subj, P.status};
        }
    });
}

void list_note_rows(ListCache& C, const uint32_t* rows, uint64_t n, uint64_t ver_before, uint64_t ver_after) noexcept {
    std::lock_guard<std::mutex> lk(C.mu);
    if (!C.state) return;
    ListState& L = *C.state;
    if (!L.host_built || !L.j_valid) return;
    if (L.j_upto != ver_before) {                           // a version went by unnoted
        L.journal_reset(false, 0);
        return;
    }
    try {
        L.journal.insert(L.journal.end(), rows, rows + n);
        L.j_upto = ver_after;
        // raw appends are deduplicated when they outgrow the distinct rows, so the journal stays within
        // twice its bound; the bound itself is applied to the distinct rows
        if (L.journal.size() > 2 * L.j_mark + 1024) journal_settle(L);
    } catch (...) {
        L.journal_reset(false, 0);
    }
}

void list_index_info(const Snapshot& S, ListCache& C, keto_list_index_info_t* out) {
    std::memset(out, 0, sizeof(*out));
    std::lock_guard<std::mutex> lk(C.mu);
    if (!C.state) return;
    ListState& L = *C.state;
    journal_settle(L);
    const uint64_t ver = S.version.load();
    out->host_built = L.host_built ? 1u : 0u;
    out->host_current = L.host_built && L.version == ver ? 1u : 0u;
    out->dev_built = L.dev_built ? 1u : 0u;
    out->dev_current = L.dev_built && L.host_built && L.dev_version == ver ? 1u : 0u;
    out->host_version = L.host_built ? L.version : 0;
    out->dev_version = L.dev_built ? L.dev_version : 0;
    out->entries = L.dev_built ? L.dev_n : 0;
    out->device_bytes = L.bytes;
    out->journal_valid = L.host_built && L.j_valid && L.j_upto == ver && patch_enabled() ? 1u : 0u;
    out->journal_rows = (uint32_t)std::min<uint64_t>(L.journal.size(), 0xFFFFFFFFull);
    out->host_builds = L.host_builds;
    out->host_patches = L.host_patches;
    out->dev_builds = L.dev_builds;
    out->dev_patches = L.dev_patches;
    out->last_segments = L.last_segments;
    out->last_staged_entries = L.last_staged;
    out->last_host_ms = L.last_host_ms;
    out->last_device_ms = L.last_device_ms;
}

namespace {

// The list index of the snapshot's version on `device`, both halves: built, patched from the journal
// or rebuilt as need be.  index_ms: a build's or a patch's time, host part included (left as it is
// when the index was current).  The caller holds C.mu and S.rw shared.
ListState& current_index(const Snapshot& S, ListCache& C, int device, float& index_ms) {
    HIP_OK(hipSetDevice(device));
    const auto ti = std::chrono::steady_clock::now();
    auto work = [&] {
        const ListState* l = C.state.get();
        return l ? l->host_builds + l->host_patches + l->dev_builds + l->dev_patches : 0;
    };
    const uint64_t work0 = work();
    ListState& L = host_index(S, C);
    if (L.dev_built && L.dev_version != L.version) {
        // the device half is behind: spliced from the journal, or -- the journal gone, or any step of
        // the patch failing -- freed and rebuilt below, where one T is all that is needed
        bool ok = false;
        if (L.dev_desc && L.j_valid && L.j_upto == L.version && L.device == device && patch_enabled()) {
            try {
                device_patch(S, L);
                ok = true;
            } catch (const Error&) {
            } catch (const std::bad_alloc&) {
            }
        }
        if (!ok) {
            (void)hipGetLastError();
            L.free_index();
            L.journal_reset(L.j_valid, L.version);
        }
    }
    if (!L.dev_built) device_index(S, L, device);
    if (work() != work0) index_ms = ms_since(ti);
    return L;
}

void scan_counts(ListState& L, const uint32_t* d_cnt, uint64_t* d_base, uint32_t m);

// The count pass of a batch of queries over the index, shared by lists (MATCH counts) and lookups (HEAD
// counts): the items per query, the query groups of at most LIST_GROUP_ITEMS items (a single query may
// exceed it; the item buffers hold one group at a time), and per group the items' upload, the count
// kernel, the scan of its counts and the queries' totals into d_tot.
struct GroupedCount {
    ListState& L;
    hipStream_t st;
    uint32_t tile;
    bool heads;                      // list_count_heads into hcnt / hwcnt / hbase, else list_count into cnt / wcnt / base
    const LQuery* d_qs;
    uint64_t* d_tot;
    uint32_t* d_qpoison;
    std::vector<uint64_t> qitems;    // n + 1: items before each query
    std::vector<uint32_t> groups;    // query boundaries of the groups
    std::vector<LItem> items;
    std::vector<uint32_t> ioff;

    GroupedCount(ListState& l, uint32_t tile_, bool heads_, const std::vector<LQuery>& qs, const LQuery* dq, uint64_t* dt,
                 uint32_t* dp, const char* who)
        : L(l), st(l.stream), tile(tile_), heads(heads_), d_qs(dq), d_tot(dt), d_qpoison(dp) {
        const uint32_t n = (uint32_t)qs.size();
        const std::string too_many = std::string(who) + ": a query spans more than 2^32 tiles";
        qitems.assign((uint64_t)n + 1, 0);
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t k = (qs[i].hi - qs[i].lo + tile - 1) / tile;
            if (k > 0xFFFFFFF0ull) throw Error{KETO_E_RANGE, too_many};
            qitems[i + 1] = qitems[i] + k;
        }
        groups.push_back(0);
        for (uint32_t i = 0; i < n; ++i)
            if (qitems[i + 1] - qitems[groups.back()] > LIST_GROUP_ITEMS && i > groups.back()) groups.push_back(i);
        groups.push_back(n);
        for (size_t g = 0; g + 1 < groups.size(); ++g)
            if (qitems[groups[g + 1]] - qitems[groups[g]] > 0xFFFFFFF0ull) throw Error{KETO_E_RANGE, too_many};
    }
    bool one_group() const { return groups.size() == 2; }
    size_t n_groups() const { return groups.size() - 1; }

    // the count pass of group g; returns its item count.  Afterwards L.items / L.ioff and the count, wave
    // count and base buffers of the mode describe this group.
    uint32_t count(size_t g) {
        const uint32_t g0 = groups[g], g1 = groups[g + 1];
        const uint32_t m = (uint32_t)(qitems[g1] - qitems[g0]);
        if (m == 0) return 0;
        items.resize(m);
        ioff.resize((uint64_t)(g1 - g0) + 1);
        for (uint32_t q = g0; q < g1; ++q) {
            const uint64_t at = qitems[q] - qitems[g0], k = qitems[q + 1] - qitems[q];
            ioff[q - g0] = (uint32_t)at;
            for (uint64_t t = 0; t < k; ++t) items[at + t] = LItem{q, (uint32_t)t};
        }
        ioff[g1 - g0] = m;
        LItem* d_items = L.items.get<LItem>(m);
        uint32_t* d_ioff = L.ioff.get<uint32_t>(ioff.size());
        uint32_t* d_cnt = L.cnt.get<uint32_t>((uint64_t)m + 1);
        uint32_t* d_wcnt = L.wcnt.get<uint32_t>((uint64_t)m * LIST_WAVES);
        uint64_t* d_base = L.base.get<uint64_t>((uint64_t)m + 1);
        HIP_OK(hipMemcpyAsync(d_items, items.data(), (uint64_t)m * sizeof(LItem), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_ioff, ioff.data(), ioff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (heads) {
            uint32_t* d_hcnt = L.hcnt.get<uint32_t>((uint64_t)m + 1);
            uint32_t* d_hwcnt = L.hwcnt.get<uint32_t>((uint64_t)m * LIST_WAVES);
            uint64_t* d_hbase = L.hbase.get<uint64_t>((uint64_t)m + 1);
            HIP_OK(hipMemsetAsync(d_hcnt + m, 0, sizeof(uint32_t), st));
            hipLaunchKernelGGL(list_count_heads, dim3(m), dim3(LIST_THREADS), 0, st, L.T, L.keys, d_qs, d_items, tile, d_cnt,
                               d_wcnt, d_qpoison, d_hcnt, d_hwcnt);
            HIP_OK(hipGetLastError());
            scan_counts(L, d_hcnt, d_hbase, m);
            d_base = d_hbase;
        } else {
            HIP_OK(hipMemsetAsync(d_cnt + m, 0, sizeof(uint32_t), st));
            hipLaunchKernelGGL(list_count, dim3(m), dim3(LIST_THREADS), 0, st, L.T, L.keys, d_qs, d_items, tile, d_cnt, d_wcnt,
                               d_qpoison);
            HIP_OK(hipGetLastError());
            scan_counts(L, d_cnt, d_base, m);
        }
        hipLaunchKernelGGL(list_totals, dim3((g1 - g0 + 255) / 256), dim3(256), 0, st, d_base, d_ioff, g0, g1 - g0, d_tot);
        HIP_OK(hipGetLastError());
        // several groups share `items` / `ioff`: the copies above must have read them before the next refill
        if (!one_group()) HIP_OK(hipStreamSynchronize(st));
        return m;
    }
};

// What the count, scan and emit passes of a batch leave behind, before any tuple goes to the host: the
// page's entries in L.out at the windows' offsets (a page holding a poisoned entry included: its
// flag is d_qpage[q], still on the device), the windows on both sides, and the statuses, tokens and
// totals as far as the host knows them (out.status / next_page / totals: all but the page-poison rule).
struct ListPasses {
    std::vector<LQuery> qs;
    std::vector<LWindow> wins;
    uint64_t total_out = 0;
    uint2* d_out = nullptr;                  // total_out entries (NULL when there are none)
    LWindow* d_wins = nullptr;               // n (uploaded when there are entries, or on request)
    uint32_t* d_qpage = nullptr;             // n
    EventPair ev;                            // ev.a: recorded in front of the passes, on L.stream
};

// The caller holds C.mu and has the index current.  Everything is enqueued on L.stream; the one host
// sync between the passes is inside.  want_wins: upload the windows also when no entry is emitted.
void list_passes(Snapshot& S, ListState& L, const keto_list_req* reqs, uint32_t n, uint32_t tile, bool want_wins,
                 ListResult& out, ListPasses& P) {
    hipStream_t st = L.stream;

    // ---- resolve (host threads)
    std::vector<LQuery>& qs = P.qs;
    qs.resize(n);
    const unsigned th = n >= 4096 ? build_threads() : 1u;
    par_chunks(n, th, 1024, [&](uint64_t b, uint64_t e, unsigned) {
        for (uint64_t i = b; i < e; ++i) {
            const Plan Pl = resolve_list(S, L, reqs[i]);
            qs[i] = Pl.q;
            out.status[i] = Pl.status;
        }
    });
    LQuery* d_qs = L.qs.get<LQuery>(n);
    uint64_t* d_tot = L.tot.get<uint64_t>(n);
    uint32_t* d_qpoison = L.qpoison.get<uint32_t>(n);
    uint32_t* d_qpage = L.qpage.get<uint32_t>(n);
    HIP_OK(hipEventRecord(P.ev.a, st));
    HIP_OK(hipMemcpyAsync(d_qs, qs.data(), (uint64_t)n * sizeof(LQuery), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_tot, 0, (uint64_t)n * sizeof(uint64_t), st));
    HIP_OK(hipMemsetAsync(d_qpoison, 0, (uint64_t)n * sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(d_qpage, 0, (uint64_t)n * sizeof(uint32_t), st));

    // the count pass, group by group (the buffers hold one group at a time)
    GroupedCount G(L, tile, /*heads=*/false, qs, d_qs, d_tot, d_qpoison, "keto_list_batch");
    uint32_t m_last = 0;
    for (size_t g = 0; g < G.n_groups(); ++g) m_last = G.count(g);

    // ---- the one host sync between the passes: totals -> sizes, statuses, tokens
    std::vector<uint64_t> tot(n);
    std::vector<uint32_t> qpoison(n);
    HIP_OK(hipMemcpyAsync(tot.data(), d_tot, (uint64_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(qpoison.data(), d_qpoison, (uint64_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    std::vector<LWindow>& wins = P.wins;
    wins.resize(n);
    uint64_t total_out = 0;
    for (uint32_t i = 0; i < n; ++i) {
        wins[i] = LWindow{0, 0, total_out};
        if (out.status[i] != KETO_LIST_OK) continue;
        if (qs[i].subj != ANY && qpoison[i]) {
            out.status[i] = KETO_LIST_UNDECIDED;
            continue;
        }
        const uint64_t size = reqs[i].page_size ? reqs[i].page_size : S.page_size;
        const uint64_t page = std::max<uint32_t>(reqs[i].page, 1u);
        const uint64_t first = (page - 1) * size;                       // < 2^63
        const uint64_t k = tot[i] > first ? std::min(size, tot[i] - first) : 0;
        out.totals[i] = tot[i];
        out.next_page[i] = page >= (tot[i] + size - 1) / size ? 0 : page + 1;
        wins[i].wlo = first;
        wins[i].whi = first + k;
        total_out += k;
    }
    P.total_out = total_out;
    P.d_qpage = d_qpage;
    if (total_out || want_wins) {
        P.d_wins = L.wins.get<LWindow>(n);
        HIP_OK(hipMemcpyAsync(P.d_wins, wins.data(), (uint64_t)n * sizeof(LWindow), hipMemcpyHostToDevice, st));
    }
    if (total_out) {
        uint2* d_out = P.d_out = L.out.get<uint2>(total_out);
        for (size_t g = 0; g < G.n_groups(); ++g) {
            const uint32_t m = G.one_group() ? m_last : G.count(g);
            if (m == 0) continue;
            hipLaunchKernelGGL(list_emit, dim3(m), dim3(LIST_THREADS), 0, st, L.T, L.keys, d_qs, (const LItem*)L.items.p, tile,
                               (const uint32_t*)L.cnt.p, (const uint32_t*)L.wcnt.p, (const uint64_t*)L.base.p,
                               (const uint32_t*)L.ioff.p, G.groups[g], P.d_wins, d_out, total_out, d_qpage);
            HIP_OK(hipGetLastError());
        }
    }
}

// what every list call checks and clears first
void list_begin(const Snapshot& S, uint32_t n, ListResult& out) {
    out.status.assign(n, KETO_LIST_OK);
    out.offsets.assign((uint64_t)n + 1, 0);
    out.next_page.assign(n, 0);
    out.totals.assign(n, 0);
    out.tuples = nullptr;
    out.index_ms = out.scan_ms = 0;
}

}  // namespace

void list_batch(Snapshot& S, ListCache& C, const keto_list_req* reqs, uint32_t n, ListResult& out) {
    if (S.n_parts > 1) throw Error{KETO_E_INVALID, "keto_list_batch: a part of a partitioned snapshot holds only some rows"};
    const DevView V = device_view(S);                        // KETO_E_HIP on a host-only snapshot
    list_begin(S, n, out);
    if (n == 0) return;
    const uint32_t tile = list_tile();
    std::lock_guard<std::mutex> lk(C.mu);                    // one list call at a time per snapshot
    ListState& L = current_index(S, C, V.device, out.index_ms);
    hipStream_t st = L.stream;
    ListPasses P;
    list_passes(S, L, reqs, n, tile, /*want_wins=*/false, out, P);
    const std::vector<LWindow>& wins = P.wins;
    const uint64_t total_out = P.total_out;

    std::vector<uint32_t> qpage(n, 0);
    struct Block {                                          // the result's pinned block until it is handed over
        void* p = nullptr;
        ~Block() { pinned_give(p); }
    } block;
    if (total_out) {
        block.p = pinned_take(total_out * sizeof(keto_list_tuple));
        static_assert(sizeof(keto_list_tuple) == sizeof(uint2), "a list tuple is an index entry");
        HIP_OK(hipMemcpyAsync(block.p, P.d_out, total_out * sizeof(uint2), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(qpage.data(), P.d_qpage, (uint64_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipEventRecord(P.ev.b, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipEventElapsedTime(&out.scan_ms, P.ev.a, P.ev.b));

    // ---- offsets; a page holding a poisoned tuple fails as a whole (toInternal over the page)
    keto_list_tuple* tup = static_cast<keto_list_tuple*>(block.p);
    uint64_t w = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t k = wins[i].whi - wins[i].wlo, from = wins[i].off;
        out.offsets[i] = w;
        if (k && qpage[i]) {
            out.status[i] = KETO_LIST_NOT_FOUND;
            out.totals[i] = 0;
            out.next_page[i] = 0;
            continue;
        }
        if (k && w != from) std::memmove(tup + w, tup + from, k * sizeof(keto_list_tuple));
        w += k;
    }
    out.offsets[n] = w;
    out.tuples = tup;
    block.p = nullptr;
}

// keto_list_encode_batch: the same passes, then the encoder (proto.hip) over the entries where list_emit
// left them.  The encoder takes S.mu under C.mu (the order: rw shared -> C.mu -> S.mu) and runs on the
// list stream; C.mu is not released while a kernel that reads L.out may be in flight.
void list_encode_batch(Snapshot& S, ListCache& C, const keto_list_req* reqs, uint32_t n, uint32_t encoding,
                       ListEncoded& out) {
    if (encoding != KETO_ENC_PROTO && encoding != KETO_ENC_JSON)
        throw Error{KETO_E_INVALID, "unknown encoding " + std::to_string(encoding)};
    if (S.n_parts > 1)
        throw Error{KETO_E_INVALID, "keto_list_encode_batch: a part of a partitioned snapshot holds only some rows"};
    const DevView V = device_view(S);                        // KETO_E_HIP on a host-only snapshot
    list_begin(S, n, out.r);
    out.offsets.assign((uint64_t)n + 1, 0);                  // n = 0: offsets {0}, not an empty vector's NULL
    out.tuples.assign(n, 0);
    out.bytes = nullptr;
    out.total = 0;
    out.encode_ms = 0;
    if (n == 0) return;
    const uint32_t tile = list_tile();
    std::lock_guard<std::mutex> lk(C.mu);
    ListState& L = current_index(S, C, V.device, out.r.index_ms);
    hipStream_t st = L.stream;
    struct Drain {                                           // also when anything below throws
        hipStream_t st;
        ~Drain() { (void)hipStreamSynchronize(st); }
    } drain{st};
    ListPasses P;
    list_passes(S, L, reqs, n, tile, /*want_wins=*/true, out.r, P);
    HIP_OK(hipEventRecord(P.ev.b, st));
    static_assert(sizeof(LWindow) == 3 * sizeof(uint64_t), "the encoder reads a window as three words");
    // per query: the token's number, or LIST_ENC_FAILED for a query that is not OK on the host's side
    std::vector<uint64_t> meta(n);
    for (uint32_t i = 0; i < n; ++i) meta[i] = out.r.status[i] == KETO_LIST_OK ? out.r.next_page[i] : LIST_ENC_FAILED;
    ListEncodeIn in{P.d_out, P.total_out, reinterpret_cast<const uint64_t*>(P.d_wins), P.d_qpage, meta.data(), n, st};
    std::vector<uint32_t> qpage;
    device_list_encode(S, in, encoding, out, qpage);
    HIP_OK(hipEventElapsedTime(&out.r.scan_ms, P.ev.a, P.ev.b));
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t k = P.wins[i].whi - P.wins[i].wlo;
        if (k && qpage[i]) {                                 // the page-poison rule, as in list_batch
            out.r.status[i] = KETO_LIST_NOT_FOUND;
            out.r.totals[i] = 0;
            out.r.next_page[i] = 0;
        }
    }
}

// ---- keto_snapshot_delete_query: the rows a query touches, and the index after the delete
namespace {

struct Widen {
    __host__ __device__ uint64_t operator()(uint32_t c) const { return c; }
};

// items of the one query Q (entries [lo, hi) in tiles) and the exclusive sum of their counts
struct OneQuery {
    uint32_t m = 0;
    LQuery* d_qs = nullptr;
    LItem* d_items = nullptr;
    uint32_t* d_ioff = nullptr;
};

OneQuery one_query(ListState& L, const LQuery& Q, uint32_t tile, std::vector<LItem>& items, uint32_t (&ioff)[2]) {
    const uint64_t k = (Q.hi - Q.lo + tile - 1) / tile;
    if (k > 0xFFFFFFF0ull) throw Error{KETO_E_RANGE, "keto_snapshot_delete_query: the query spans more than 2^32 tiles"};
    OneQuery o;
    o.m = (uint32_t)k;
    items.resize(o.m);
    for (uint32_t t = 0; t < o.m; ++t) items[t] = LItem{0, t};
    ioff[0] = 0;
    ioff[1] = o.m;
    o.d_qs = L.qs.get<LQuery>(1);
    o.d_items = L.items.get<LItem>(o.m);
    o.d_ioff = L.ioff.get<uint32_t>(2);
    HIP_OK(hipMemcpyAsync(o.d_qs, &Q, sizeof(LQuery), hipMemcpyHostToDevice, L.stream));
    HIP_OK(hipMemcpyAsync(o.d_items, items.data(), (uint64_t)o.m * sizeof(LItem), hipMemcpyHostToDevice, L.stream));
    HIP_OK(hipMemcpyAsync(o.d_ioff, ioff, 2 * sizeof(uint32_t), hipMemcpyHostToDevice, L.stream));
    return o;
}

void scan_counts(ListState& L, const uint32_t* d_cnt, uint64_t* d_base, uint32_t m) {
    hipcub::TransformInputIterator<uint64_t, Widen, const uint32_t*> cit(d_cnt, Widen{});
    size_t tb = 0;
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cit, d_base, (uint64_t)m + 1, L.stream));
    void* tmp = L.tmp.get<uint8_t>(tb);
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cit, d_base, (uint64_t)m + 1, L.stream));
}

// the device pass: one count launch (matches, heads, the poison flag), the scans, one host sync, then
// the HEAD emit of the touched row ids into a pinned block sized exactly.  The caller holds C.mu.
void scan_device(ListState& L, const LQuery& Q, uint64_t max_rows, DeleteScan& out) {
    const uint32_t tile = list_tile();
    hipStream_t st = L.stream;
    EventPair ev;
    HIP_OK(hipEventRecord(ev.a, st));
    std::vector<LItem> items;
    uint32_t ioff[2];
    uint64_t tot[2] = {0, 0};
    uint32_t poison = 0;
    const OneQuery o = one_query(L, Q, tile, items, ioff);
    const uint32_t m = o.m;
    if (m) {
        uint32_t* d_cnt = L.cnt.get<uint32_t>((uint64_t)m + 1);
        uint32_t* d_wcnt = L.wcnt.get<uint32_t>((uint64_t)m * LIST_WAVES);
        uint64_t* d_base = L.base.get<uint64_t>((uint64_t)m + 1);
        uint32_t* d_hcnt = L.hcnt.get<uint32_t>((uint64_t)m + 1);
        uint32_t* d_hwcnt = L.hwcnt.get<uint32_t>((uint64_t)m * LIST_WAVES);
        uint64_t* d_hbase = L.hbase.get<uint64_t>((uint64_t)m + 1);
        uint32_t* d_qpoison = L.qpoison.get<uint32_t>(1);
        HIP_OK(hipMemsetAsync(d_cnt + m, 0, sizeof(uint32_t), st));
        HIP_OK(hipMemsetAsync(d_hcnt + m, 0, sizeof(uint32_t), st));
        HIP_OK(hipMemsetAsync(d_qpoison, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(list_count_heads, dim3(m), dim3(LIST_THREADS), 0, st, L.T, L.keys, o.d_qs, o.d_items, tile, d_cnt,
                           d_wcnt, d_qpoison, d_hcnt, d_hwcnt);
        HIP_OK(hipGetLastError());
        scan_counts(L, d_cnt, d_base, m);
        scan_counts(L, d_hcnt, d_hbase, m);
        HIP_OK(hipMemcpyAsync(&tot[0], d_base + m, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(&tot[1], d_hbase + m, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(&poison, d_qpoison, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));                 // the one host sync: totals -> the block's size
    }
    out.matches = tot[0];
    out.heads = tot[1];
    out.poisoned = poison != 0;
    if (m && out.heads && !out.poisoned && out.heads <= max_rows) {
        const LWindow win{0, out.heads, 0};
        LWindow* d_wins = L.wins.get<LWindow>(1);
        uint32_t* d_out = L.out.get<uint32_t>(out.heads);
        HIP_OK(hipMemcpyAsync(d_wins, &win, sizeof(LWindow), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(list_emit_heads, dim3(m), dim3(LIST_THREADS), 0, st, L.T, L.keys, o.d_qs, (const LItem*)o.d_items,
                           tile, (const uint32_t*)L.hcnt.p, (const uint32_t*)L.hwcnt.p, (const uint64_t*)L.hbase.p,
                           (const uint32_t*)o.d_ioff, 0u, d_wins, reinterpret_cast<uint2*>(d_out), out.heads, nullptr);
        HIP_OK(hipGetLastError());
        struct Block {
            void* p;
            ~Block() { pinned_give(p); }
        } block{pinned_take(out.heads * sizeof(uint32_t))};
        HIP_OK(hipMemcpyAsync(block.p, d_out, out.heads * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        const uint32_t* r = static_cast<const uint32_t*>(block.p);
        out.rows.assign(r, r + out.heads);
    }
    HIP_OK(hipEventRecord(ev.b, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipEventElapsedTime(&out.scan_ms, ev.a, ev.b));
}

// the host pass over the candidate rows ord[p0, p1): key predicates per row, the subject word by a
// scan of the row's edges
void scan_host(const Snapshot& S, const ListState& L, const Plan& P, DeleteScan& out) {
    const uint64_t n = P.p1 - P.p0;
    const unsigned th = (P.q.hi - P.q.lo) >= par_min() ? build_threads() : 1u;
    struct Part {
        std::vector<uint32_t> rows;
        uint64_t matches = 0;
        bool poisoned = false;
    };
    std::vector<Part> parts(std::max(1u, th));
    par_chunks(n, th, 1 << 12, [&](uint64_t b, uint64_t e, unsigned t) {
        Part& p = parts[t];
        for (uint64_t i = P.p0 + b; i < P.p0 + e; ++i) {
            const uint32_t row = L.ord[i];
            const RowKey& k = S.row_key[row];
            if ((P.q.obj != ANY && k.obj != P.q.obj) || (P.q.rel != ANY && k.rel != P.q.rel)) continue;
            const auto ed = S.row_edges(row);
            if (S.row_pp[row] != NO_PAGE && std::find(ed.first, ed.first + ed.second, EDGE_POISON) != ed.first + ed.second)
                p.poisoned = true;
            const uint64_t c = P.q.subj == ANY ? ed.second : (uint64_t)std::count(ed.first, ed.first + ed.second, P.q.subj);
            if (!c) continue;
            p.matches += c;
            p.rows.push_back(row);
        }
    });
    for (Part& p : parts) {
        out.matches += p.matches;
        out.poisoned = out.poisoned || p.poisoned;
        out.rows.insert(out.rows.end(), p.rows.begin(), p.rows.end());
    }
    out.heads = out.rows.size();
}

}  // namespace

void delete_scan(const Snapshot& S, ListCache& C, const keto_list_req& rq, uint64_t max_rows, DeleteScan& out) {
    out = DeleteScan{};
    const auto t0 = std::chrono::steady_clock::now();
    const bool keyed = rq.namespace_.n && rq.object.n && rq.relation.n;      // one row: always the host's
    std::unique_lock<std::mutex> lk(C.mu);
    const ListState& L = host_index(S, C);
    const Plan P = resolve_list(S, L, rq);
    if (P.status != KETO_LIST_OK) {
        // GetNamespaceByName fails the reference's transaction (relationtuples.go:161,180)
        std::string_view name = sv(rq.namespace_);
        if (name.empty() || S.ns_index(name) >= 0) name = sv(rq.subject.set_namespace);
        throw Error{KETO_E_INVALID, "Unknown namespace with name " + std::string(name) + "."};
    }
    out.subject = P.q.subj;
    out.lo = P.q.lo;
    out.hi = P.q.hi;
    out.obj = P.q.obj;
    out.rel = P.q.rel;
    out.version = L.version;
    if (P.q.lo == P.q.hi) {                               // nothing can match
        out.scan_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return;
    }
    if (!keyed && S.dev && S.n_parts == 1 && L.dev_built && L.dev_version == L.version && L.device >= 0) {
        out.path = KETO_DELETE_PATH_DEVICE;
        HIP_OK(hipSetDevice(L.device));
        scan_device(*C.state, P.q, max_rows, out);
    } else {
        // the host tables of this version stay as they are while the caller holds the lock shared:
        // list calls go on during the scan
        lk.unlock();
        scan_host(S, L, P, out);
        out.scan_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (out.heads > max_rows) out.rows.clear();
    std::sort(out.rows.begin(), out.rows.end());
    out.rows.erase(std::unique(out.rows.begin(), out.rows.end()), out.rows.end());
}

namespace {

// the new T: entries [0, lo), the kept entries of [lo, hi), entries [hi, N) behind them
void patch_device(ListState& L, const DeleteScan& sc, uint64_t N) {
    const uint32_t tile = list_tile();
    hipStream_t st = L.stream;
    const uint64_t newN = N - sc.matches, t_entries = (newN + 2) & ~1ull, old_entries = (N + 2) & ~1ull;
    struct Fresh {
        uint2* p = nullptr;
        ~Fresh() {
            if (p) (void)hipFree(p);
        }
    } fresh;
    HIP_OK(hipMalloc((void**)&fresh.p, t_entries * sizeof(uint2)));
    HIP_OK(hipMemsetAsync(fresh.p + newN, 0, (t_entries - newN) * sizeof(uint2), st));
    if (sc.lo) HIP_OK(hipMemcpyAsync(fresh.p, L.T, sc.lo * sizeof(uint2), hipMemcpyDeviceToDevice, st));
    const LQuery Q{sc.lo, sc.hi, sc.obj, sc.rel, sc.subject, 0};
    std::vector<LItem> items;
    uint32_t ioff[2];
    const OneQuery o = one_query(L, Q, tile, items, ioff);
    const uint32_t m = o.m;
    uint32_t* d_cnt = L.cnt.get<uint32_t>((uint64_t)m + 1);
    uint32_t* d_wcnt = L.wcnt.get<uint32_t>((uint64_t)m * LIST_WAVES);
    uint64_t* d_base = L.base.get<uint64_t>((uint64_t)m + 1);
    uint32_t* d_qpoison = L.qpoison.get<uint32_t>(1);
    HIP_OK(hipMemsetAsync(d_cnt + m, 0, sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(d_qpoison, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(list_count, dim3(m), dim3(LIST_THREADS), 0, st, L.T, L.keys, o.d_qs, o.d_items, tile, d_cnt, d_wcnt,
                       d_qpoison);
    HIP_OK(hipGetLastError());
    scan_counts(L, d_cnt, d_base, m);
    uint64_t total = 0;
    HIP_OK(hipMemcpyAsync(&total, d_base + m, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (total != sc.matches) throw Error{KETO_E_INVALID, "the list index does not hold the deleted tuples"};
    const LWindow win{0, sc.hi - sc.lo, sc.lo};
    LWindow* d_wins = L.wins.get<LWindow>(1);
    HIP_OK(hipMemcpyAsync(d_wins, &win, sizeof(LWindow), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(list_emit_keep, dim3(m), dim3(LIST_THREADS), 0, st, L.T, L.keys, o.d_qs, (const LItem*)o.d_items, tile,
                       (const uint32_t*)d_cnt, (const uint32_t*)d_wcnt, (const uint64_t*)d_base, (const uint32_t*)o.d_ioff, 0u,
                       d_wins, fresh.p, sc.hi - sc.matches, nullptr);
    HIP_OK(hipGetLastError());
    if (N > sc.hi)
        HIP_OK(hipMemcpyAsync(fresh.p + (sc.hi - sc.matches), L.T + sc.hi, (N - sc.hi) * sizeof(uint2), hipMemcpyDeviceToDevice,
                              st));
    HIP_OK(hipStreamSynchronize(st));
    std::swap(L.T, fresh.p);                              // the old T is freed with `fresh`
    L.bytes = L.bytes - old_entries * sizeof(uint2) + t_entries * sizeof(uint2);
}

}  // namespace

bool delete_index_patch(const Snapshot& S, ListCache& C, const DeleteScan& sc) noexcept {
    std::lock_guard<std::mutex> lk(C.mu);
    if (!C.state) return false;
    ListState& L = *C.state;
    try {
        // a list call may have built the device half between the scan and the commit: it is of the
        // scanned version all the same (writes are one at a time)
        // (a device half behind the scanned version is not kept: a delete never patches from the journal)
        bool dev = L.dev_built && L.host_built && L.version == sc.version && L.dev_version == sc.version && S.dev &&
                   S.n_parts == 1;
        if (dev && sc.matches) {
            HIP_OK(hipSetDevice(L.device));
            patch_device(L, sc, L.first.back());
        }
        if (!dev) {
            // no device half to keep: the host half is rebuilt by the next list call, under the shared
            // lock, instead of here under the exclusive one; the journal goes with the index
            L.host_built = false;
            L.journal_reset(false, 0);
            if (L.device >= 0) {
                (void)hipSetDevice(L.device);
                L.free_index();
            }
            L.drop_dev_desc();
            return false;
        }
        host_tables(S, L);
        L.dev_built = true;
        L.dev_version = L.version;
        L.dev_n = L.first.back();
        L.dev_patches += 1;
        return true;
    } catch (...) {
        L.host_built = false;
        L.journal_reset(false, 0);
        if (L.device >= 0) {
            (void)hipSetDevice(L.device);
            L.free_index();
        }
        return false;
    }
}

// ---- keto_lookup_objects_batch: which objects of a namespace does a subject have a relation on
namespace {

uint64_t lookup_env(const char* name, uint64_t def, uint64_t lo, uint64_t hi) {
    const char* e = getenv(name);
    if (!e) return def;
    const long long v = atoll(e);
    if (v < (long long)lo || (uint64_t)v > hi)
        throw Error{KETO_E_INVALID, std::string(name) + " must lie in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]"};
    return (uint64_t)v;
}

}  // namespace

void lookup_objects(Snapshot& S, ListCache& C, const keto_lookup_req* reqs, uint32_t n, int32_t gmd, LookupResult& out) {
    if (S.n_parts > 1)
        throw Error{KETO_E_INVALID, "keto_lookup_objects_batch: a part of a partitioned snapshot holds only some rows"};
    const DevView V = device_view(S);                        // KETO_E_HIP on a host-only snapshot
    out.status.assign(n, KETO_LOOKUP_OK);
    out.offsets.assign((uint64_t)n + 1, 0);
    out.next_page.assign(n, 0);
    out.totals.assign(n, 0);
    out.candidates.assign(n, 0);
    out.undecided.assign(n, 0);
    out.rows = nullptr;
    out.index_ms = out.candidates_ms = out.check_ms = out.emit_ms = 0;
    if (n == 0) return;
    const uint32_t tile = list_tile();
    const uint64_t chunk = lookup_env("KETO_LOOKUP_CHUNK", 1ull << 22, 64, 1ull << 30);
    const uint64_t max_cand = lookup_env("KETO_LOOKUP_MAX_CANDIDATES", 1ull << 28, 0, 1ull << 40);
    std::lock_guard<std::mutex> lk(C.mu);                    // one list or lookup call at a time per snapshot
    ListState& L = current_index(S, C, V.device, out.index_ms);
    hipStream_t st = L.stream;
    struct Trim {
        ListState& l;
        ~Trim() { l.lookup_trim(); }
    } trim{L};

    // ---- plan (host): namespace + relation through the list resolver, the subject as a check target
    std::vector<LQuery> qs(n);
    std::vector<LSubj> subj(n);
    const unsigned th = n >= 4096 ? build_threads() : 1u;
    par_chunks(n, th, 1024, [&](uint64_t pb, uint64_t pe, unsigned) {
        for (uint64_t i = pb; i < pe; ++i) {
            const keto_lookup_req& rq = reqs[i];
            qs[i] = LQuery{0, 0, ANY, ANY, ANY, 0};
            subj[i] = LSubj{KETO_NO_TARGET, 0, rq.max_depth, 0};
            const keto_subject& sb = rq.subject;
            if (!rq.namespace_.n || !rq.relation.n ||
                (sb.kind != 0 && (!sb.set_namespace.n || !sb.set_object.n || !sb.set_relation.n))) {
                out.status[i] = KETO_LOOKUP_UNSUPPORTED;
                continue;
            }
            keto_list_req lr;
            std::memset(&lr, 0, sizeof lr);
            lr.namespace_ = rq.namespace_;
            lr.relation = rq.relation;
            const Plan P = resolve_list(S, L, lr);
            if (P.status != KETO_LIST_OK) {
                out.status[i] = KETO_LOOKUP_UNKNOWN_NAMESPACE;
                continue;
            }
            qs[i] = P.q;
            if (sb.kind == 0) {
                const int64_t sid = S.lookup_str(sv(sb.id));
                if (sid >= 0) subj[i].target = (uint32_t)sid;
            } else {
                const int64_t t = S.resolve_query(sv(sb.set_namespace), sv(sb.set_object), sv(sb.set_relation));
                if (t >= 0) {
                    subj[i].target = (uint32_t)t;
                    subj[i].flags = 1;
                }
            }
        }
    });

    // ---- candidates: the HEAD passes over all queries, in query groups as in list_batch
    LQuery* d_qs = L.qs.get<LQuery>(n);
    uint64_t* d_tot = L.tot.get<uint64_t>(n);
    uint32_t* d_qpoison = L.qpoison.get<uint32_t>(n);        // written by the HEAD count, never read here
    for (hipEvent_t& x : L.lk_ev)                            // made once, kept with the index state
        if (!x) HIP_OK(hipEventCreate(&x));
    hipEvent_t* const ev = L.lk_ev;
    HIP_OK(hipEventRecord(ev[0], st));
    HIP_OK(hipMemcpyAsync(d_qs, qs.data(), (uint64_t)n * sizeof(LQuery), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_tot, 0, (uint64_t)n * sizeof(uint64_t), st));
    HIP_OK(hipMemsetAsync(d_qpoison, 0, (uint64_t)n * sizeof(uint32_t), st));
    GroupedCount G(L, tile, /*heads=*/true, qs, d_qs, d_tot, d_qpoison, "keto_lookup_objects_batch");
    uint32_t m_last = 0;
    for (size_t g = 0; g < G.n_groups(); ++g) m_last = G.count(g);

    // ---- the first host sync: candidates per query -> qoff, the cap, the buffers' sizes
    std::vector<uint64_t> qoff((uint64_t)n + 1, 0);
    HIP_OK(hipMemcpyAsync(out.candidates.data(), d_tot, (uint64_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n; ++i) qoff[i + 1] = qoff[i] + out.candidates[i];
    const uint64_t H = qoff[n];
    if (H > max_cand)
        throw Error{KETO_E_INVALID, "keto_lookup_objects_batch: " + std::to_string(H) + " candidates, more than KETO_LOOKUP_MAX_CANDIDATES (" +
                                        std::to_string(max_cand) + ")"};
    if (H == 0) {
        HIP_OK(hipEventRecord(ev[1], st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipEventElapsedTime(&out.candidates_ms, ev[0], ev[1]));
        return;                                              // every total is 0
    }
    uint32_t* d_cand = L.lk_cand.get<uint32_t>(H);
    uint64_t* d_qoff = L.lk_qoff.get<uint64_t>((uint64_t)n + 1);
    LSubj* d_subj = L.lk_subj.get<LSubj>(n);
    std::vector<LWindow> wins(n);
    for (uint32_t i = 0; i < n; ++i) wins[i] = LWindow{0, out.candidates[i], qoff[i]};
    LWindow* d_wins = L.wins.get<LWindow>(n);
    HIP_OK(hipMemcpyAsync(d_wins, wins.data(), (uint64_t)n * sizeof(LWindow), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_qoff, qoff.data(), ((uint64_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_subj, subj.data(), (uint64_t)n * sizeof(LSubj), hipMemcpyHostToDevice, st));
    for (size_t g = 0; g < G.n_groups(); ++g) {
        const uint32_t m = G.one_group() ? m_last : G.count(g);
        if (m == 0) continue;
        hipLaunchKernelGGL(list_emit_heads, dim3(m), dim3(LIST_THREADS), 0, st, L.T, L.keys, d_qs, (const LItem*)L.items.p, tile,
                           (const uint32_t*)L.hcnt.p, (const uint32_t*)L.hwcnt.p, (const uint64_t*)L.hbase.p,
                           (const uint32_t*)L.ioff.p, G.groups[g], d_wins, reinterpret_cast<uint2*>(d_cand), H, nullptr);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(ev[1], st));

    // ---- check, in chunks: requests made on the device, decisions written straight into dec[]
    const uint64_t dec_bytes = (H + 7) & ~3ull;             // padded: lookup_quad loads whole words
    uint8_t* d_dec = L.lk_dec.get<uint8_t>(dec_bytes);
    uint4* d_reqs = L.lk_reqs.get<uint4>(std::min(chunk, H));
    HIP_OK(hipMemsetAsync(d_dec + (H & ~3ull), 0, dec_bytes - (H & ~3ull), st));
    for (uint64_t c0 = 0; c0 < H; c0 += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, H - c0);
        hipLaunchKernelGGL(lookup_make_reqs, dim3((m + LIST_THREADS - 1) / LIST_THREADS), dim3(LIST_THREADS), 0, st,
                           (const uint32_t*)d_cand, (const uint64_t*)d_qoff, n, (const LSubj*)d_subj, c0, m, d_reqs);
        HIP_OK(hipGetLastError());
        device_check_rows(S, reinterpret_cast<const keto_check_ids*>(d_reqs), m, gmd, d_dec + c0, st, /*rows_valid=*/true);
    }
    HIP_OK(hipEventRecord(ev[2], st));

    // ---- ordered compaction: items over the queries' candidates, count / scan / emit
    std::vector<uint64_t> citems((uint64_t)n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) citems[i + 1] = citems[i] + (out.candidates[i] + tile - 1) / tile;
    if (citems[n] > 0x7FFFFFF0ull) throw Error{KETO_E_RANGE, "keto_lookup_objects_batch: more than 2^31 candidate tiles"};
    const uint32_t cm = (uint32_t)citems[n];
    std::vector<LItem> cit(cm);
    std::vector<uint32_t> cioff((uint64_t)n + 1);
    for (uint32_t q = 0; q < n; ++q) {
        cioff[q] = (uint32_t)citems[q];
        for (uint64_t t = 0; t < citems[q + 1] - citems[q]; ++t) cit[citems[q] + t] = LItem{q, (uint32_t)t};
    }
    cioff[n] = cm;
    LItem* d_items = L.items.get<LItem>(cm);
    uint32_t* d_ioff = L.ioff.get<uint32_t>((uint64_t)n + 1);
    uint32_t* d_cnt = L.cnt.get<uint32_t>((uint64_t)cm + 1);
    uint32_t* d_wcnt = L.wcnt.get<uint32_t>((uint64_t)cm * LIST_WAVES);
    uint64_t* d_base = L.base.get<uint64_t>((uint64_t)cm + 1);
    unsigned long long* d_und = L.lk_und.get<unsigned long long>(n);
    HIP_OK(hipMemcpyAsync(d_items, cit.data(), (uint64_t)cm * sizeof(LItem), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_ioff, cioff.data(), ((uint64_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_cnt + cm, 0, sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(d_und, 0, (uint64_t)n * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(lookup_count, dim3(cm), dim3(LIST_THREADS), 0, st, (const uint8_t*)d_dec, (const uint64_t*)d_qoff,
                       (const LItem*)d_items, tile, d_cnt, d_wcnt, d_und);
    HIP_OK(hipGetLastError());
    scan_counts(L, d_cnt, d_base, cm);
    hipLaunchKernelGGL(list_totals, dim3((n + 255) / 256), dim3(256), 0, st, d_base, d_ioff, 0u, n, d_tot);
    HIP_OK(hipGetLastError());

    // ---- the second host sync: totals -> statuses, tokens, windows, the pinned block's size
    std::vector<uint64_t> tot(n);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the undecided counters are 64-bit");
    HIP_OK(hipMemcpyAsync(tot.data(), d_tot, (uint64_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(out.undecided.data(), d_und, (uint64_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    uint64_t total_out = 0;
    for (uint32_t i = 0; i < n; ++i) {
        wins[i] = LWindow{0, 0, total_out};
        out.offsets[i] = total_out;
        if (out.status[i] != KETO_LOOKUP_OK) continue;
        if (out.undecided[i]) {
            out.status[i] = KETO_LOOKUP_UNDECIDED;
            continue;
        }
        const uint64_t size = reqs[i].page_size ? reqs[i].page_size : S.page_size;
        const uint64_t page = std::max<uint32_t>(reqs[i].page, 1u);
        const uint64_t first = (page - 1) * size;                       // < 2^63
        const uint64_t k = tot[i] > first ? std::min(size, tot[i] - first) : 0;
        out.totals[i] = tot[i];
        out.next_page[i] = page >= (tot[i] + size - 1) / size ? 0 : page + 1;
        wins[i].wlo = first;
        wins[i].whi = first + k;
        total_out += k;
    }
    out.offsets[n] = total_out;
    struct Block {                                          // the result's pinned block until it is handed over
        void* p = nullptr;
        ~Block() { pinned_give(p); }
    } block;
    if (total_out) {
        uint32_t* d_out = L.out.get<uint32_t>(total_out);
        HIP_OK(hipMemcpyAsync(d_wins, wins.data(), (uint64_t)n * sizeof(LWindow), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(lookup_emit, dim3(cm), dim3(LIST_THREADS), 0, st, (const uint8_t*)d_dec, (const uint32_t*)d_cand,
                           (const uint64_t*)d_qoff, (const LItem*)d_items, tile, (const uint32_t*)d_cnt,
                           (const uint32_t*)d_wcnt, (const uint64_t*)d_base, (const uint32_t*)d_ioff,
                           (const LWindow*)d_wins, d_out, total_out);
        HIP_OK(hipGetLastError());
        block.p = pinned_take(total_out * sizeof(uint32_t));
        HIP_OK(hipMemcpyAsync(block.p, d_out, total_out * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipEventRecord(ev[3], st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipEventElapsedTime(&out.candidates_ms, ev[0], ev[1]));
    HIP_OK(hipEventElapsedTime(&out.check_ms, ev[1], ev[2]));
    HIP_OK(hipEventElapsedTime(&out.emit_ms, ev[2], ev[3]));
    out.rows = static_cast<uint32_t*>(block.p);
    block.p = nullptr;
}

}  // namespace keto
