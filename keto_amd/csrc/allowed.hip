// keto_allowed_subjects_batch: the SubjectIDs a check allows on an object (MI355X, gfx950).
//
// The mirror of keto_lookup_objects_batch (list.hip): take a complete candidate set on the device,
// decide every candidate forwards with the check kernels, compact the allowed ones in order, and let
// nothing but the page leave device memory.  The answer is by construction the set this engine's check
// allows, visited-map quirks included.
//
// Why the candidates are complete (the argument at the head of reach.hip): a check at clamped depth d
// says yes only when a row it enters holds the requested id (engine.go:54), and it enters only rows
// within d - 1 subject-set hops of the request's row (engine.go:88-91).  So every id that can be allowed
// is an id edge of a row within d - 1 hops of the query's row over the stored effective subject-set
// edges.  The generator below gathers exactly those id edges: a superset (the visited map can only
// remove answers), which the check then decides one by one.  Being a superset it reproduces no quirk --
// it reads ROW_SEQ rows word by word, ignores closure filters and poison flags -- and when in doubt it
// emits; what it never does is miss a row at hop d - 1.
//
//   plan        host: the query's row id through the check path's resolver, the depth clamped as a
//               check request's (engine.go:118-120), the statuses that need no device work
//   BFS         level-synchronous over all queries at once.  A frontier entry is the 64-bit key
//               query << 32 | handle; all levels lie one after another in vis[] (the visited set).
//               Per level: al_count (a lane per slot of the level's bound; the level's size is read
//               on the device: it is what the emit before appended) gives tiles of AL_TILE edges per row
//               and the level's id-edge and set-edge totals, a 64-bit exclusive scan of the tiles, then
//               the level's ONE host sync: what the emit before appended and whether it must run again,
//               and this level's totals, which size the buffers, the table and the grid.  al_emit (a
//               block per (entry, tile)): id edges are appended to the candidate keys as query << 32 | id,
//               set edges claim query << 32 | target in an open-addressing table of 64-bit keys by
//               atomicCAS, the winner appends the key to the next level; the next level's count and
//               scan follow it on the stream.  Atomics decide membership and a place in a bag, never an
//               order: the candidates are sorted next, the frontier's order changes nothing that is kept.
//               The table is kept at most half full and sized ahead of a level (for its bound, or a
//               fourfold step); a claim looks at AL_PROBES slots at most and at none once the level has
//               reported that it outgrew the table; the host then sizes the table for the level's whole
//               bound, re-inserts vis[] and runs that emit again: at most once per level
//   dedupe      hipcub radix sort of the candidate keys over bits [0, 32 + bits(n)), hipcub unique,
//               al_split: cand[] = the low words, qoff[] by lower bound
//   check       chunks of KETO_ALLOWED_CHUNK: al_make_reqs writes {the query's row id, id, 0, max_depth},
//               device_check_rows decides them into dec[] next to cand[]
//   page        a 64-bit exclusive scan of the allowed flags (the rank of every candidate), al_totals,
//               one host sync (totals, undecided counts -> statuses, tokens, windows), al_page stores
//               the candidates whose rank falls in the window; one DMA brings the page back
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "allowed.hpp"
#include "hip_check.hpp"
#include "snapshot.hpp"

namespace keto {

namespace {

inline std::string_view sv(const keto_str& s) { return std::string_view(s.p ? s.p : "", s.n); }

constexpr uint32_t AL_THREADS = 256;
constexpr uint32_t AL_TILE = 1024;              // edges of a row per block of al_emit (4 per lane)
constexpr unsigned long long AL_EMPTY = ~0ull;           // no key: a query index never reaches 2^32 - 1
constexpr uint32_t AL_PAD = 0xFFFFFFFFu;        // the padding behind a row's edges
constexpr uint32_t AL_PROBES = 128;             // slots a claim looks at (the table is kept at most half full)
constexpr uint64_t AL_TABLE_FLOOR = 1ull << 16; // visited keys the table is sized for without being asked

struct ABuf {            // a grow-only device buffer
    void* p = nullptr;
    uint64_t cap = 0;
    hipStream_t st = nullptr;        // the stream whose work may still use the block: drained before it is freed
    ABuf() = default;
    ABuf(const ABuf&) = delete;
    ABuf& operator=(const ABuf&) = delete;
    template <class T>
    T* get(uint64_t n) {
        const uint64_t want = std::max<uint64_t>(16, n * sizeof(T));
        if (want > cap) {
            if (p && st) HIP_OK(hipStreamSynchronize(st));   // (explicit: hipFree would wait for the device anyway)
            release();
            alloc(want + want / 8);
        }
        return (T*)p;
    }
    // the same, keeping the first `keep` entries (a copy on `st`, which is drained before the old block goes)
    template <class T>
    T* grow(uint64_t n, uint64_t keep, hipStream_t st) {
        const uint64_t want = std::max<uint64_t>(16, n * sizeof(T));
        if (want > cap) {
            ABuf nb;
            nb.alloc(want + want / 2);
            if (keep) {
                HIP_OK(hipMemcpyAsync(nb.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st));
                HIP_OK(hipStreamSynchronize(st));
            }
            std::swap(p, nb.p);
            std::swap(cap, nb.cap);
        }
        return (T*)p;
    }
    void alloc(uint64_t bytes) {
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            throw Error{KETO_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)};
        }
        cap = bytes;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    ~ABuf() { release(); }
};

struct AQuery {          // a query on the device: its row id, the request's depth and the clamped one
    uint32_t row;
    int32_t max_depth, depth;
    uint32_t pad;
};
struct AWindow {         // ranks [wlo, whi) of the query's allowed ids go to out[off ...)
    uint64_t wlo, whi, off;
};
struct ASeed {
    uint32_t q, row;
};

// the level's counters: id edges and set edges its rows hold (bounds of what al_emit appends), the
// candidate keys and next-level keys appended, the table's overflow flag; over the call, the forwarded rows
// the count passes met
enum { AC_IDS = 0, AC_SETS = 1, AC_CAND = 2, AC_NEXT = 3, AC_OVER = 4, AC_FWD = 5, AC_N = 8 };

__host__ __device__ inline uint64_t amix(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// a row's header, forwards followed (row_at of reach.hip): n = its effective edge words, e0 = the first
// of them this level reads (a row whose sets are not followed starts at its ids), beg = the arena word
// of edge 0.  false: the handle lies outside the arena (never, for a handle an edge or the map holds).
struct ARow {
    uint64_t beg;
    uint32_t e0, n, n_sets, n_ids;
    bool seq, fwd;                   // fwd: the identity header was a forward
};
__device__ inline bool al_row(const uint32_t* __restrict__ a, uint64_t words, uint32_t h, uint32_t g, bool follow, ARow& r) {
    uint64_t w = hword(h, g);
    if (w + HDR_WORDS > words) return false;
    uint4 h0 = *reinterpret_cast<const uint4*>(a + w);
    r.fwd = (h0.z & HDR_FWD) != 0;
    for (uint32_t hops = 0; (h0.z & HDR_FWD) && hops < 64; ++hops) {
        w = hword(h0.x, g);
        if (w + HDR_WORDS > words) return false;
        h0 = *reinterpret_cast<const uint4*>(a + w);
    }
    if (h0.z & (HDR_FWD | HDR_REMOTE)) return false;
    r.seq = (h0.z & HDR_SEQ) != 0;
    r.n_sets = h0.x;
    r.n_ids = r.seq ? 0u : h0.y;
    r.beg = w + HDR_WORDS;
    const uint64_t n = (uint64_t)r.n_sets + r.n_ids;
    if (r.beg + n > words) return false;
    r.n = (uint32_t)n;
    r.e0 = (follow || r.seq) ? 0u : r.n_sets;
    return true;
}

// vis[k] = q << 32 | the handle of the query's row, and the key into the table (the keys are distinct)
__global__ void __launch_bounds__(AL_THREADS)
al_seed(const ASeed* __restrict__ seeds, uint32_t m, const uint32_t* __restrict__ row_handle, uint32_t n_rows,
        uint64_t* __restrict__ vis, uint64_t* __restrict__ table, uint64_t mask) {
    const uint32_t i = blockIdx.x * AL_THREADS + threadIdx.x;
    if (i >= m) return;
    const ASeed s = seeds[i];
    const uint32_t h = s.row < n_rows ? row_handle[s.row] : NO_UNIT;
    const uint64_t key = ((uint64_t)s.q << 32) | h;       // NO_UNIT (never on an unpartitioned snapshot): al_row refuses it
    vis[i] = key;
    unsigned long long* t = reinterpret_cast<unsigned long long*>(table);
    for (uint64_t s0 = amix(key) & mask, k = 0; k <= mask; s0 = (s0 + 1) & mask, ++k)
        if (atomicCAS(t + s0, AL_EMPTY, (unsigned long long)key) == AL_EMPTY) break;
}

// the visited keys into a table that was just doubled
__global__ void __launch_bounds__(AL_THREADS)
al_reinsert(const uint64_t* __restrict__ vis, uint64_t m, uint64_t* __restrict__ table, uint64_t mask) {
    const uint64_t i = (uint64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (i >= m) return;
    const uint64_t key = vis[i];
    unsigned long long* t = reinterpret_cast<unsigned long long*>(table);
    for (uint64_t s0 = amix(key) & mask, k = 0; k <= mask; s0 = (s0 + 1) & mask, ++k)
        if (atomicCAS(t + s0, AL_EMPTY, (unsigned long long)key) == AL_EMPTY) break;
}

// a lane per slot of the level's bound: tiles[i] = the blocks al_emit spends on frontier entry i's row, 0 for
// the slots past the level's size m (tiles[bound] included: the scan's total).  m comes from the host
// (level 0) or is what the emit before appended (m_dev, at most bound): the host has not seen it yet.  Also
// the level's id-edge and set-edge totals (counts, no order hangs on them), one atomic per block each.
__global__ void __launch_bounds__(AL_THREADS)
al_count(const uint32_t* __restrict__ arena, uint64_t words, uint32_t g, const uint64_t* __restrict__ fr,
         const unsigned long long* __restrict__ m_dev, uint64_t m_host, uint64_t bound, const AQuery* __restrict__ qs,
         uint32_t level, uint32_t* __restrict__ tiles, unsigned long long* __restrict__ ctr) {
    __shared__ unsigned long long sh[2];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t m = m_dev ? min((uint64_t)*m_dev, bound) : m_host;
    const uint64_t i = (uint64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (i <= bound) {
        uint32_t t = 0;
        if (i < m) {
            const uint64_t key = fr[i];
            const bool follow = (int64_t)level + 2 <= (int64_t)qs[key >> 32].depth;
            ARow r;
            if (al_row(arena, words, (uint32_t)key, g, follow, r)) {
                t = (r.n - r.e0 + AL_TILE - 1) / AL_TILE;
                const uint32_t ids = r.seq ? r.n_sets : r.n_ids, sets = follow ? r.n_sets : 0u;
                if (ids) atomicAdd(&sh[0], (unsigned long long)ids);
                if (sets) atomicAdd(&sh[1], (unsigned long long)sets);
                if (r.fwd) atomicAdd(ctr + AC_FWD, 1ull);                // (rare: rows a write moved)
            }
        }
        tiles[i] = t;
    }
    __syncthreads();
    if (threadIdx.x < 2 && sh[threadIdx.x]) atomicAdd(ctr + (threadIdx.x == 0 ? AC_IDS : AC_SETS), sh[threadIdx.x]);
}

struct Widen {           // a tile count widened for the scan
    __host__ __device__ uint64_t operator()(uint32_t x) const { return x; }
};

// a block per (entry, tile): the entry is the last one whose first tile tbase[i] is at or before the
// block (entries without tiles share their successor's and are passed over).  An id edge goes to the
// candidate keys, the wave's ids behind one another from one atomicAdd; a set edge claims its key, and
// the winner appends it to the next level.  cand_cap / next_cap: the room the level's totals promised.
__global__ void __launch_bounds__(AL_THREADS)
al_emit(const uint32_t* __restrict__ arena, uint64_t words, uint32_t g, const uint64_t* __restrict__ fr, uint64_t m,
        const AQuery* __restrict__ qs, uint32_t level, const uint64_t* __restrict__ tbase, uint64_t* __restrict__ ckeys,
        uint64_t cand_cap, uint64_t* __restrict__ next, uint64_t next_cap, uint64_t* __restrict__ table, uint64_t mask,
        uint64_t visited, uint64_t fill_limit, unsigned long long* __restrict__ ctr) {
    const uint64_t b = blockIdx.x;
    uint64_t lo = 0, hi = m;                                // tbase[lo] <= b; tbase[hi] > b or hi == m
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (tbase[mid] <= b) lo = mid;
        else hi = mid;
    }
    const uint64_t key = fr[lo];
    const uint64_t qhi = key & 0xFFFFFFFF00000000ull;
    const bool follow = (int64_t)level + 2 <= (int64_t)qs[key >> 32].depth;
    ARow r;
    if (!al_row(arena, words, (uint32_t)key, g, follow, r)) return;      // (block-uniform)
    const uint64_t t0 = (uint64_t)r.e0 + (b - tbase[lo]) * AL_TILE;
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long* tb = reinterpret_cast<unsigned long long*>(table);
    for (uint32_t k = 0; k < AL_TILE / AL_THREADS; ++k) {                // (block-uniform trip count)
        const uint64_t e = t0 + (uint64_t)k * AL_THREADS + threadIdx.x;
        uint32_t w = AL_PAD;
        if (e < r.n) w = arena[r.beg + e];
        const bool skip = w == AL_PAD || w == EDGE_POISON;
        const bool is_id = !skip && !(w & EDGE_SET);
        const uint64_t ids = __ballot(is_id);
        if (ids) {
            unsigned long long at = 0;
            if (lane == (uint32_t)(__ffsll((long long)ids) - 1)) at = atomicAdd(ctr + AC_CAND, (unsigned long long)__popcll(ids));
            at = __shfl(at, __ffsll((long long)ids) - 1);
            at += __popcll(ids & ((1ull << lane) - 1ull));
            if (is_id && at < cand_cap) ckeys[at] = qhi | w;
        }
        if (follow && !skip && (w & EDGE_SET)) {
            const uint64_t nk = qhi | (w & EDGE_VAL);
            bool won = false;
            // at most AL_PROBES slots are looked at, and none once the level is known to run again: a
            // table too small for the level costs a bounded pass, not a scan of the table per key
            if (*reinterpret_cast<volatile unsigned long long*>(ctr + AC_OVER) == 0ull) {
                bool done = false;
                uint64_t s0 = amix(nk) & mask;
                for (uint32_t p = 0; p < AL_PROBES && p <= mask; s0 = (s0 + 1) & mask, ++p) {
                    const unsigned long long old = atomicCAS(tb + s0, AL_EMPTY, (unsigned long long)nk);
                    if (old == AL_EMPTY) won = true;
                    if (old == AL_EMPTY || old == nk) {
                        done = true;
                        break;
                    }
                }
                if (!done) ctr[AC_OVER] = 1;                             // no place found: the level runs again
            }
            if (won) {
                const unsigned long long at = atomicAdd(ctr + AC_NEXT, 1ull);
                if (visited + at + 1 > fill_limit) ctr[AC_OVER] = 1;
                if (at < next_cap) next[at] = nk;
            }
        }
    }
}

// sorted distinct keys -> cand[] (the low words) and, for q <= n, qoff[q] = the first key of query q or later
__global__ void __launch_bounds__(AL_THREADS)
al_split(const uint64_t* __restrict__ keys, uint64_t m, uint32_t n, uint32_t* __restrict__ cand, uint64_t* __restrict__ qoff) {
    const uint64_t i = (uint64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (i < m) cand[i] = (uint32_t)keys[i];
    if (i <= n) {
        const uint64_t want = i << 32;
        uint64_t lo = 0, hi = m;                            // keys[lo - 1] < want <= keys[hi]
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        qoff[i] = lo;
    }
}

// the query of candidate g: the last one whose first candidate qoff[q] is at or before it
__device__ inline uint32_t al_query_of(const uint64_t* __restrict__ qoff, uint32_t nq, uint64_t g) {
    uint32_t lo = 0, hi = nq;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (qoff[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the 16-B check requests of candidates [c0, c0 + m): one 16-B store per lane
__global__ void __launch_bounds__(AL_THREADS)
al_make_reqs(const uint32_t* __restrict__ cand, const uint64_t* __restrict__ qoff, uint32_t nq,
             const AQuery* __restrict__ qs, uint64_t c0, uint32_t m, uint4* __restrict__ reqs) {
    const uint32_t i = blockIdx.x * AL_THREADS + threadIdx.x;
    if (i >= m) return;
    const uint64_t g = c0 + i;
    const AQuery q = qs[al_query_of(qoff, nq, g)];
    reqs[i] = make_uint4(q.row, cand[g], 0u, (uint32_t)q.max_depth);
}

struct IsAllowed {       // a decision byte's allowed flag, widened for the scan
    __host__ __device__ uint64_t operator()(uint8_t d) const { return d == 1 ? 1ull : 0ull; }
};

// tot[q] = the allowed candidates of query q (rank[] holds H + 1 entries); the undecided ones are
// counted per query by al_undecided (a count, no order hangs on it)
__global__ void __launch_bounds__(AL_THREADS)
al_totals(const uint64_t* __restrict__ rank, const uint64_t* __restrict__ qoff, uint32_t n, uint64_t* __restrict__ tot) {
    const uint32_t q = blockIdx.x * AL_THREADS + threadIdx.x;
    if (q < n) tot[q] = rank[qoff[q + 1]] - rank[qoff[q]];
}
__global__ void __launch_bounds__(AL_THREADS)
al_undecided(const uint8_t* __restrict__ dec, uint64_t H, const uint64_t* __restrict__ qoff, uint32_t n,
             unsigned long long* __restrict__ und) {
    const uint64_t i = (uint64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (i < H && dec[i] == KETO_UNDECIDED) atomicAdd(und + al_query_of(qoff, n, i), 1ull);
}

// an allowed candidate whose rank within its query falls in the query's window goes to the page
__global__ void __launch_bounds__(AL_THREADS)
al_page(const uint8_t* __restrict__ dec, const uint32_t* __restrict__ cand, uint64_t H, const uint64_t* __restrict__ rank,
        const uint64_t* __restrict__ qoff, uint32_t n, const AWindow* __restrict__ wins, uint32_t* __restrict__ out,
        uint64_t out_n) {
    const uint64_t i = (uint64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (i >= H || dec[i] != 1) return;
    const uint32_t q = al_query_of(qoff, n, i);
    const AWindow W = wins[q];
    const uint64_t r = rank[i] - rank[qoff[q]];
    if (r < W.wlo || r >= W.whi) return;
    const uint64_t at = W.off + (r - W.wlo);
    if (at < out_n) out[at] = cand[i];
}

uint64_t allowed_env(const char* name, uint64_t def, uint64_t lo, uint64_t hi) {
    const char* e = getenv(name);
    if (!e) return def;
    const long long v = atoll(e);
    if (v < (long long)lo || (uint64_t)v > hi)
        throw Error{KETO_E_INVALID, std::string(name) + " must lie in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]"};
    return (uint64_t)v;
}

uint64_t pow2_at_least(uint64_t v) {
    uint64_t p = 64;
    while (p < v) p <<= 1;
    return p;
}

unsigned grid_of(uint64_t items) {
    const uint64_t b = (items + AL_THREADS - 1) / AL_THREADS;
    if (b > 0x7FFFFFF0ull) throw Error{KETO_E_RANGE, "keto_allowed_subjects_batch: more than 2^31 blocks in one pass"};
    return (unsigned)std::max<uint64_t>(b, 1);
}

}  // namespace

struct AllowedState {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // the BFS: visited keys (8 B each; every level's frontier), the claim table (8 B a slot), a level's
    // tile counts (4 B) and their scan (8 B), the counters, the seeds (8 B a query)
    // (tiles and their scan twice: a level's emit may have to run again after the next level was counted)
    ABuf vis, table, tiles[2], tbase[2], ctr, seeds, qs, tmp;
    // candidate keys (8 B each, twice: the sort is out of place; the second holds the ranks later),
    // candidates (4 B), decisions (1 B), a chunk's requests (16 B)
    ABuf keys_in, keys_out, cand, dec, reqs, sel;
    ABuf qoff, tot, und, wins, out;
    std::vector<ABuf*> all() {
        return {&vis, &table, &tiles[0], &tiles[1], &tbase[0], &tbase[1], &ctr, &seeds, &qs, &tmp, &keys_in, &keys_out,
                &cand, &dec, &reqs, &sel, &qoff, &tot, &und, &wins, &out};
    }
    // big workspaces do not linger, the per-query ones included
    void trim() {
        for (ABuf* b : all())
            if (b->cap > (256ull << 20)) b->release();
    }
    ~AllowedState() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

void AllowedStateDeleter::operator()(AllowedState* s) const { delete s; }

void allowed_subjects(Snapshot& S, AllowedCache& C, const keto_allowed_req* reqs, uint32_t n, int32_t gmd, AllowedResult& out) {
    if (S.n_parts > 1)
        throw Error{KETO_E_INVALID, "keto_allowed_subjects_batch: a part of a partitioned snapshot holds only some rows"};
    const DevView V = device_view(S);                        // KETO_E_HIP on a host-only snapshot
    out.status.assign(n, KETO_ALLOWED_OK);
    out.offsets.assign((uint64_t)n + 1, 0);
    out.next_page.assign(n, 0);
    out.totals.assign(n, 0);
    out.candidates.assign(n, 0);
    out.undecided.assign(n, 0);
    out.ids = nullptr;
    out.bfs_ms = out.dedupe_ms = out.check_ms = out.emit_ms = 0;
    out.visited = out.slots = out.forwards = 0;
    out.levels = out.regrows = out.reruns = 0;
    if (n == 0) return;
    if (n > 0x7FFFFFF0u) throw Error{KETO_E_RANGE, "keto_allowed_subjects_batch: more than 2^31 queries"};
    const uint64_t chunk = allowed_env("KETO_ALLOWED_CHUNK", 1ull << 22, 64, 1ull << 30);
    const uint64_t max_cand = allowed_env("KETO_ALLOWED_MAX_CANDIDATES", 1ull << 28, 0, 1ull << 40);
    const uint64_t slots0 = allowed_env("KETO_ALLOWED_VISITED_SLOTS", 0, 0, 1ull << 36);

    // ---- plan (host): the row through the check path's resolver, the depth clamped as a check request's
    std::vector<AQuery> qs(n);
    std::vector<ASeed> seeds;
    int32_t levels = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const keto_allowed_req& rq = reqs[i];
        int32_t d = rq.max_depth;
        if (d <= 0 || gmd < d) d = gmd;                      // engine.go:118-120
        qs[i] = AQuery{KETO_NO_ROW, rq.max_depth, d, 0};
        if (!rq.namespace_.n || !rq.object.n || !rq.relation.n) {
            out.status[i] = KETO_ALLOWED_UNSUPPORTED;
            continue;
        }
        const int64_t row = S.resolve_query(sv(rq.namespace_), sv(rq.object), sv(rq.relation));
        if (row == -2) {
            out.status[i] = KETO_ALLOWED_UNKNOWN_NAMESPACE;
            continue;
        }
        if (row < 0 || d <= 0) continue;                     // no row, or no depth: nothing can be allowed
        qs[i].row = (uint32_t)row;
        seeds.push_back(ASeed{i, (uint32_t)row});
        levels = std::max(levels, d);
    }
    if (seeds.empty()) return;                               // every total is 0

    const uint32_t* row_handle = device_row_handle_map(S);   // takes and drops the device lock
    std::lock_guard<std::mutex> lk(C.mu);                    // one call at a time per snapshot
    HIP_OK(hipSetDevice(V.device));
    if (!C.state) C.state.reset(new AllowedState());
    AllowedState& W = *C.state;
    if (W.device != V.device) {
        if (W.device >= 0) throw Error{KETO_E_INVALID, "keto_allowed_subjects_batch: the snapshot moved to another device"};
        W.device = V.device;
    }
    if (!W.stream) {
        HIP_OK(hipStreamCreateWithFlags(&W.stream, hipStreamNonBlocking));
        for (ABuf* b : W.all()) b->st = W.stream;
    }
    for (hipEvent_t& x : W.ev)                               // made once, kept with the workspace
        if (!x) HIP_OK(hipEventCreate(&x));
    hipStream_t st = W.stream;
    // whatever happens below, nothing of this call is in flight when its buffers go or the lock is dropped
    struct Drain {
        AllowedState& w;
        ~Drain() {
            (void)hipStreamSynchronize(w.stream);
            w.trim();
        }
    } drain{W};

    const uint32_t g = S.root_g;
    const uint64_t m0 = seeds.size();
    AQuery* d_qs = W.qs.get<AQuery>(n);
    ASeed* d_seeds = W.seeds.get<ASeed>(m0);
    unsigned long long* d_ctr = W.ctr.get<unsigned long long>(AC_N);
    HIP_OK(hipEventRecord(W.ev[0], st));
    HIP_OK(hipMemcpyAsync(d_qs, qs.data(), (uint64_t)n * sizeof(AQuery), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_seeds, seeds.data(), m0 * sizeof(ASeed), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_ctr, 0, AC_N * sizeof(unsigned long long), st));

    // ---- BFS
    const uint64_t floor_keys = slots0 ? slots0 : AL_TABLE_FLOOR;
    uint64_t slots = pow2_at_least(slots0 ? slots0 : 8 * m0);
    while (slots < 2 * m0) slots <<= 1;                      // the seeds alone stay under half
    uint64_t* d_table = W.table.get<uint64_t>(slots);
    HIP_OK(hipMemsetAsync(d_table, 0xFF, slots * sizeof(uint64_t), st));
    uint64_t* d_vis = W.vis.get<uint64_t>(m0);
    hipLaunchKernelGGL(al_seed, dim3(grid_of(m0)), dim3(AL_THREADS), 0, st, (const ASeed*)d_seeds, (uint32_t)m0, row_handle,
                       (uint32_t)S.n_rows(), d_vis, d_table, slots - 1);
    HIP_OK(hipGetLastError());
    uint64_t lv_begin = 0, lv_end = m0, n_keys = 0;          // the level's frontier = vis[lv_begin, lv_end)
    uint64_t* d_keys = W.keys_in.get<uint64_t>(1);
    unsigned long long ctr[AC_N];

    // a table of `want` slots holding the visited keys vis[0, lv_end)
    auto table_of = [&](uint64_t want) {
        if (want > (1ull << 40)) throw Error{KETO_E_RANGE, "keto_allowed_subjects_batch: the visited table outgrew 2^40 slots"};
        slots = want;
        d_table = W.table.get<uint64_t>(slots);
        HIP_OK(hipMemsetAsync(d_table, 0xFF, slots * sizeof(uint64_t), st));
        hipLaunchKernelGGL(al_reinsert, dim3(grid_of(lv_end)), dim3(AL_THREADS), 0, st, (const uint64_t*)d_vis, lv_end, d_table,
                           slots - 1);
        HIP_OK(hipGetLastError());
    };
    // count + scan of level `lvl`, whose frontier starts at vis[at] and has m_host entries, or as many as
    // the emit before it appends (at most `bound`; the host learns the number at the level's sync)
    uint64_t bound = 0;
    auto count_level = [&](uint32_t lvl, uint64_t at, bool from_dev, uint64_t m_host, uint64_t bnd) {
        if (bnd + 1 > 0x7FFFFFF0ull) throw Error{KETO_E_RANGE, "keto_allowed_subjects_batch: more than 2^31 rows in a level"};
        bound = bnd;
        uint32_t* d_tiles = W.tiles[lvl & 1].get<uint32_t>(bnd + 1);
        uint64_t* d_tbase = W.tbase[lvl & 1].get<uint64_t>(bnd + 1);
        HIP_OK(hipMemsetAsync(d_ctr + AC_IDS, 0, 2 * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(al_count, dim3(grid_of(bnd + 1)), dim3(AL_THREADS), 0, st, V.arena, V.arena_words, g,
                           (const uint64_t*)(d_vis + at), from_dev ? (const unsigned long long*)(d_ctr + AC_NEXT) : nullptr, m_host,
                           bnd, (const AQuery*)d_qs, lvl, d_tiles, d_ctr);
        HIP_OK(hipGetLastError());
        hipcub::TransformInputIterator<uint64_t, Widen, const uint32_t*> in(d_tiles, Widen{});
        size_t tb = 0;
        HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, d_tbase, (int)(bnd + 1), st));
        void* tmp = W.tmp.get<uint8_t>(tb);
        HIP_OK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, d_tbase, (int)(bnd + 1), st));
    };
    struct Emit {                                            // the emit in flight: what running it again takes
        bool valid = false;
        uint32_t level = 0;
        uint64_t F = 0, n_tiles = 0, ids = 0, sets = 0;
    } em;
    // emit of level em.level over vis[lv_begin, lv_end), then the count of the level it appends
    auto emit_level = [&] {
        HIP_OK(hipMemsetAsync(d_ctr + AC_NEXT, 0, 2 * sizeof(unsigned long long), st));
        HIP_OK(hipMemcpyAsync(d_ctr + AC_CAND, &n_keys, sizeof(uint64_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(al_emit, dim3((unsigned)em.n_tiles), dim3(AL_THREADS), 0, st, V.arena, V.arena_words, g,
                           (const uint64_t*)(d_vis + lv_begin), em.F, (const AQuery*)d_qs, em.level,
                           (const uint64_t*)W.tbase[em.level & 1].p, d_keys, n_keys + em.ids, d_vis + lv_end, em.sets, d_table,
                           slots - 1, lv_end, slots / 2, d_ctr);
        HIP_OK(hipGetLastError());
        count_level(em.level + 1, lv_end, /*from_dev=*/true, 0, em.sets);
    };
    out.regrows = out.reruns = 0;
    count_level(0, 0, /*from_dev=*/false, m0, m0);
    for (uint32_t level = 0;;) {
        // the level's one host sync: what the emit before appended (and whether it must run again), and
        // this level's totals, which size the buffers and the grid
        uint64_t n_tiles = 0;
        HIP_OK(hipMemcpyAsync(ctr, d_ctr, AC_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(&n_tiles, (const uint64_t*)W.tbase[level & 1].p + bound, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (em.valid && ctr[AC_OVER]) {
            // the table was too small for the level: size it for the level's bound (every set edge a new
            // key), put the visited keys back and run the emit again -- it appends the same ids behind
            // n_keys and claims the level's targets afresh.  At most once per level, but for a claim that
            // found no place in a table under half full (AL_PROBES), which doubles it
            const uint64_t need = pow2_at_least(2 * (lv_end + em.sets));
            table_of(need > slots ? need : slots * 2);
            ++out.reruns;
            emit_level();
            continue;
        }
        if (em.valid) {
            n_keys = std::min<uint64_t>(ctr[AC_CAND], n_keys + em.ids);
            lv_begin = lv_end;
            lv_end += std::min<uint64_t>(ctr[AC_NEXT], em.sets);
            em.valid = false;
        }
        const uint64_t F = lv_end - lv_begin;
        if (F == 0 || level >= (uint32_t)levels) break;
        const uint64_t ids = ctr[AC_IDS], sets = ctr[AC_SETS];
        if (n_keys + ids > max_cand)
            throw Error{KETO_E_INVALID, "keto_allowed_subjects_batch: " + std::to_string(n_keys + ids) +
                                            " id edges gathered, more than KETO_ALLOWED_MAX_CANDIDATES (" +
                                            std::to_string(max_cand) + ")"};
        if (n_tiles == 0) {
            lv_begin = lv_end;
            break;
        }
        if (n_tiles > 0x7FFFFFF0ull) throw Error{KETO_E_RANGE, "keto_allowed_subjects_batch: more than 2^31 edge tiles in a level"};
        d_keys = W.keys_in.grow<uint64_t>(n_keys + ids + 1, n_keys, st);
        d_vis = W.vis.grow<uint64_t>(lv_end + sets, lv_end, st);
        // the table ahead of the level: room for the level's bound, but for no more than four times the
        // keys visited so far (or the floor) -- a level whose set edges mostly name visited rows need not pay
        // for all of them; one that does outgrow it reports that and runs again (above)
        const uint64_t target = std::min<uint64_t>(lv_end + sets, std::max<uint64_t>(4 * lv_end, floor_keys));
        if (2 * target > slots) {
            table_of(pow2_at_least(2 * target));
            ++out.regrows;
        }
        em.valid = true;
        em.level = level;
        em.F = F;
        em.n_tiles = n_tiles;
        em.ids = ids;
        em.sets = sets;
        emit_level();
        ++level;
        out.levels = level;
    }
    out.visited = lv_end;
    out.slots = slots;
    out.forwards = ctr[AC_FWD];
    HIP_OK(hipEventRecord(W.ev[1], st));
    if (n_keys == 0) {
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipEventElapsedTime(&out.bfs_ms, W.ev[0], W.ev[1]));
        return;                                              // every total is 0
    }
    if (n_keys > 0x7FFFFFF0ull) throw Error{KETO_E_RANGE, "keto_allowed_subjects_batch: more than 2^31 id edges"};

    // ---- distinct candidates: sort, unique, split
    uint32_t qbits = 0;
    while (qbits < 32 && (1ull << qbits) < n) ++qbits;
    uint64_t* d_sorted = W.keys_out.get<uint64_t>(n_keys + 1);
    uint64_t* d_sel = W.sel.get<uint64_t>(1);
    {
        size_t tb = 0;
        HIP_OK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, (const uint64_t*)d_keys, d_sorted, (int)n_keys, 0, (int)(32 + qbits), st));
        void* tmp = W.tmp.get<uint8_t>(tb);
        HIP_OK(hipcub::DeviceRadixSort::SortKeys(tmp, tb, (const uint64_t*)d_keys, d_sorted, (int)n_keys, 0, (int)(32 + qbits), st));
        tb = 0;
        HIP_OK(hipcub::DeviceSelect::Unique(nullptr, tb, (const uint64_t*)d_sorted, d_keys, d_sel, (int)n_keys, st));
        tmp = W.tmp.get<uint8_t>(tb);
        HIP_OK(hipcub::DeviceSelect::Unique(tmp, tb, (const uint64_t*)d_sorted, d_keys, d_sel, (int)n_keys, st));
    }
    uint64_t H = 0;
    HIP_OK(hipMemcpyAsync(&H, d_sel, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (H == 0 || H > n_keys) throw Error{KETO_E_HIP, "keto_allowed_subjects_batch: the unique pass returned no count"};
    uint32_t* d_cand = W.cand.get<uint32_t>(H);
    uint64_t* d_qoff = W.qoff.get<uint64_t>((uint64_t)n + 1);
    hipLaunchKernelGGL(al_split, dim3(grid_of(std::max<uint64_t>(H, (uint64_t)n + 1))), dim3(AL_THREADS), 0, st,
                       (const uint64_t*)d_keys, H, n, d_cand, d_qoff);
    HIP_OK(hipGetLastError());
    std::vector<uint64_t> qoff((uint64_t)n + 1);
    HIP_OK(hipMemcpyAsync(qoff.data(), d_qoff, ((uint64_t)n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipEventRecord(W.ev[2], st));

    // ---- check, in chunks: requests made on the device, decisions written straight into dec[]
    uint8_t* d_dec = W.dec.get<uint8_t>(H + 1);
    uint4* d_reqs = W.reqs.get<uint4>(std::min(chunk, H));
    HIP_OK(hipMemsetAsync(d_dec + H, 0, 1, st));             // the scan reads H + 1 flags
    for (uint64_t c0 = 0; c0 < H; c0 += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, H - c0);
        hipLaunchKernelGGL(al_make_reqs, dim3(grid_of(m)), dim3(AL_THREADS), 0, st, (const uint32_t*)d_cand,
                           (const uint64_t*)d_qoff, n, (const AQuery*)d_qs, c0, m, d_reqs);
        HIP_OK(hipGetLastError());
        device_check_rows(S, reinterpret_cast<const keto_check_ids*>(d_reqs), m, gmd, d_dec + c0, st, /*rows_valid=*/true);
    }
    HIP_OK(hipEventRecord(W.ev[3], st));

    // ---- ordered compaction: the rank of every candidate among the allowed ones, totals, the page
    uint64_t* d_rank = d_sorted;                             // (the sorted keys are done with: H + 1 <= n_keys + 1)
    uint64_t* d_tot = W.tot.get<uint64_t>(n);
    unsigned long long* d_und = W.und.get<unsigned long long>(n);
    {
        hipcub::TransformInputIterator<uint64_t, IsAllowed, const uint8_t*> in(d_dec, IsAllowed{});
        size_t tb = 0;
        HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, d_rank, (int)(H + 1), st));
        void* tmp = W.tmp.get<uint8_t>(tb);
        HIP_OK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, d_rank, (int)(H + 1), st));
    }
    HIP_OK(hipMemsetAsync(d_und, 0, (uint64_t)n * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(al_totals, dim3(grid_of(n)), dim3(AL_THREADS), 0, st, (const uint64_t*)d_rank, (const uint64_t*)d_qoff, n,
                       d_tot);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(al_undecided, dim3(grid_of(H)), dim3(AL_THREADS), 0, st, (const uint8_t*)d_dec, H,
                       (const uint64_t*)d_qoff, n, d_und);
    HIP_OK(hipGetLastError());
    std::vector<uint64_t> tot(n);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the undecided counters are 64-bit");
    HIP_OK(hipMemcpyAsync(tot.data(), d_tot, (uint64_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(out.undecided.data(), d_und, (uint64_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    std::vector<AWindow> wins(n);
    uint64_t total_out = 0;
    for (uint32_t i = 0; i < n; ++i) {
        wins[i] = AWindow{0, 0, total_out};
        out.offsets[i] = total_out;
        out.candidates[i] = qoff[i + 1] - qoff[i];
        if (out.status[i] != KETO_ALLOWED_OK) continue;
        if (out.undecided[i]) {
            out.status[i] = KETO_ALLOWED_UNDECIDED;
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
        uint32_t* d_out = W.out.get<uint32_t>(total_out);
        AWindow* d_wins = W.wins.get<AWindow>(n);
        HIP_OK(hipMemcpyAsync(d_wins, wins.data(), (uint64_t)n * sizeof(AWindow), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(al_page, dim3(grid_of(H)), dim3(AL_THREADS), 0, st, (const uint8_t*)d_dec, (const uint32_t*)d_cand, H,
                           (const uint64_t*)d_rank, (const uint64_t*)d_qoff, n, (const AWindow*)d_wins, d_out, total_out);
        HIP_OK(hipGetLastError());
        block.p = pinned_take(total_out * sizeof(uint32_t));
        HIP_OK(hipMemcpyAsync(block.p, d_out, total_out * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipEventRecord(W.ev[4], st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipEventElapsedTime(&out.bfs_ms, W.ev[0], W.ev[1]));
    HIP_OK(hipEventElapsedTime(&out.dedupe_ms, W.ev[1], W.ev[2]));
    HIP_OK(hipEventElapsedTime(&out.check_ms, W.ev[2], W.ev[3]));
    HIP_OK(hipEventElapsedTime(&out.emit_ms, W.ev[3], W.ev[4]));
    out.ids = static_cast<uint32_t*>(block.p);
    block.p = nullptr;
}

}  // namespace keto
