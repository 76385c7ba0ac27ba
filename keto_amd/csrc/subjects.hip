// keto_subjects_batch: which subjects have a relation on an object -- Expand's answer flattened on the
// device.  device_expand (its `keep` form) leaves the finished node arena of the batch in the
// snapshot's device buffers; this unit is that arena's third consumer, next to the two encoders of
// proto.hip, and returns 4 B per distinct SubjectID leaf of the requested page instead of every node.
//
//   scan        hipcub exclusive sum (64-bit) over the nodes' id-leaf flags, read through a transform
//               iterator (no flag array); id-leaf = info bit31 set, subject bit31 clear
//   compact     subj_compact: the id-leaf words to leaf[scan[i]]; the set leaves (both bits set: depth
//               cut, revisited or empty sets) are counted per tree, one atomic per wave and tree
//   segments    subj_segments: tree t's leaves are leaf[loff[t], loff[t+1]), loff[t] = scan[toff[t]];
//               the trees are put in a class by their leaf count L (two compacted lists)
//   -- the arena is not read after this; one small D2H (the class counts) and the host drops the
//      device state's mutex
//   sort+unique L <= 64: subj_sort_wave, a wave per segment, a bitonic network over the lanes;
//               L <= KETO_SUBJECTS_LDS: subj_sort_block, a block per segment, a bitonic sort in LDS;
//               beyond: subj_global_keys + hipcub::DeviceRadixSort over 64-bit (segment start << 32 |
//               word) keys + subj_unique_stream, a block per segment streaming over the sorted keys.
//               Every class leaves the segment's distinct words, ascending, at leaf[loff[t] ...) and
//               their count in ucount[t]
//   page        ucount / leaves / set_leaves D2H in one copy; the host applies the list rule and sizes
//               the pinned block; subj_emit copies each window to the output, one DMA brings it back
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_check.hpp"
#include "snapshot.hpp"
#include "subjects.hpp"

namespace keto {

namespace {

constexpr uint32_t SJ_THREADS = 256;
constexpr uint32_t SJ_WAVES = SJ_THREADS / 64;
constexpr uint32_t SJ_WAVE_MAX = 64;            // the wave class: a segment per wave, a word per lane
constexpr uint32_t SJ_PAD = 0xFFFFFFFFu;        // sorts behind every string id (bit 31 clear)
constexpr uint32_t SJ_STREAM_ITEMS = 16;        // sorted keys per thread and tile of subj_unique_stream
constexpr uint32_t SJ_KEY_CHUNKS = 256;         // blocks a global segment's key pass is spread over, at most

struct SBuf {            // a grow-only device buffer
    void* p = nullptr;
    uint64_t cap = 0;
    SBuf() = default;
    SBuf(const SBuf&) = delete;
    SBuf& operator=(const SBuf&) = delete;
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
    ~SBuf() { release(); }
};

struct IdLeaf {          // a node's id-leaf flag, widened for the scan
    __host__ __device__ uint64_t operator()(const keto_tree_node& x) const {
        return ((x.info & EDGE_SET) && !(x.subject & EDGE_SET)) ? 1ull : 0ull;
    }
};

struct SWindow {         // ranks [first, ...) of the query's distinct words go to out[off ...)
    uint64_t first, off;
};

// the counters behind the per-tree counts: block-class segments, global-class segments, their leaves
enum { CTR_BLOCK = 0, CTR_GLOBAL = 1, CTR_GITEMS = 2, CTR_N = 4 };

// the scan at position p <= n_nodes (the scan holds n_nodes entries: its end is the last entry plus
// the last node's flag)
__device__ inline uint64_t scan_at(const uint64_t* __restrict__ scan, const keto_tree_node* __restrict__ nodes,
                                   uint64_t n_nodes, uint64_t p) {
    if (p < n_nodes) return scan[p];
    return n_nodes ? scan[n_nodes - 1] + IdLeaf{}(nodes[n_nodes - 1]) : 0;
}

// leaf[scan[i]] = the id leaf i's word; set_leaves[t] += the set leaves of tree t.  A wave's set leaves
// of one tree make one atomic (a depth-cut tree is a run of them).
__global__ void __launch_bounds__(SJ_THREADS)
subj_compact(const keto_tree_node* __restrict__ nodes, uint64_t n_nodes, const uint64_t* __restrict__ scan,
             const uint64_t* __restrict__ toff, uint32_t n_trees, uint32_t* __restrict__ leaf,
             unsigned long long* __restrict__ set_leaves) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t b = (uint64_t)blockIdx.x * SJ_THREADS; b < n_nodes; b += (uint64_t)gridDim.x * SJ_THREADS) {
        const uint64_t i = b + threadIdx.x;
        bool is_set = false;
        uint32_t t = 0xFFFFFFFFu;
        if (i < n_nodes) {
            const keto_tree_node x = nodes[i];
            if (x.info & EDGE_SET) {
                if (!(x.subject & EDGE_SET)) {
                    leaf[scan[i]] = x.subject;
                } else {
                    is_set = true;
                    uint32_t lo = 0, hi = n_trees;          // the last tree starting at or before i
                    while (hi - lo > 1) {
                        const uint32_t mid = lo + (hi - lo) / 2;
                        if (toff[mid] <= i) lo = mid;
                        else hi = mid;
                    }
                    t = lo;
                }
            }
        }
        unsigned long long m = __ballot(is_set);
        while (m) {                                         // (wave-uniform)
            const int leader = __ffsll((long long)m) - 1;
            const uint32_t t0 = __shfl(t, leader);
            const unsigned long long same = __ballot(is_set && t == t0);
            if (lane == (uint32_t)leader) atomicAdd(&set_leaves[t0], (unsigned long long)__popcll(same));
            m &= ~same;
        }
    }
}

// loff[t] = scan[toff[t]] for t <= n; leaves[t]; the tree's class
__global__ void __launch_bounds__(SJ_THREADS)
subj_segments(const keto_tree_node* __restrict__ nodes, uint64_t n_nodes, const uint64_t* __restrict__ scan,
              const uint64_t* __restrict__ toff, uint32_t n, uint32_t lds_limit, uint64_t* __restrict__ loff,
              unsigned long long* __restrict__ cnt, uint32_t* __restrict__ blist, uint32_t* __restrict__ glist,
              unsigned long long* __restrict__ gstart, unsigned long long* __restrict__ ctr) {
    const uint32_t t = blockIdx.x * SJ_THREADS + threadIdx.x;
    if (t > n) return;
    const uint64_t a = scan_at(scan, nodes, n_nodes, toff[t]);
    loff[t] = a;
    if (t == n) return;
    const uint64_t L = scan_at(scan, nodes, n_nodes, toff[t + 1]) - a;
    cnt[(uint64_t)n + t] = L;
    if (L > lds_limit) {
        const unsigned long long k = atomicAdd(&ctr[CTR_GLOBAL], 1ull);
        glist[k] = t;
        gstart[k] = atomicAdd(&ctr[CTR_GITEMS], (unsigned long long)L);
    } else if (L > SJ_WAVE_MAX) {
        blist[atomicAdd(&ctr[CTR_BLOCK], 1ull)] = t;
    }
}

// L <= 64: a wave per segment, the words in the lanes (padded), a bitonic network of cross-lane moves,
// heads by comparing with the lane below, compacted by ballot and popcount.  The wave has read the
// whole segment before it writes, so the distinct words go back in place.
__global__ void __launch_bounds__(SJ_THREADS)
subj_sort_wave(uint32_t* __restrict__ leaf, const uint64_t* __restrict__ loff, unsigned long long* __restrict__ cnt,
               uint32_t n) {
    const uint32_t t = blockIdx.x * SJ_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (t >= n) return;
    const uint64_t L = cnt[(uint64_t)n + t];
    if (L == 0 || L > SJ_WAVE_MAX) return;                  // (ucount[t] is 0 already; the other classes)
    const uint64_t base = loff[t];
    uint32_t v = lane < L ? leaf[base + lane] : SJ_PAD;
    for (uint32_t k = 2; k <= 64; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t p = __shfl_xor(v, (int)j);
            const bool up = (lane & k) == 0, lower = (lane & j) == 0;
            v = (lower == up) ? min(v, p) : max(v, p);
        }
    const uint32_t below = __shfl_up(v, 1);
    const bool head = lane < L && (lane == 0 || v != below);
    const unsigned long long m = __ballot(head);
    if (head) leaf[base + __popcll(m & ((1ull << lane) - 1))] = v;
    if (lane == 0) cnt[t] = (unsigned long long)__popcll(m);
}

// exclusive prefix of c over the block's threads, and the block's total (wtot: SJ_WAVES words of LDS)
__device__ inline uint32_t block_exclusive(uint32_t c, uint32_t* wtot, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = c;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d);
        if (lane >= d) inc += y;
    }
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    uint32_t pre = 0;
    total = 0;
    for (uint32_t k = 0; k < SJ_WAVES; ++k) {
        if (k < w) pre += wtot[k];
        total += wtot[k];
    }
    __syncthreads();                                        // (wtot is free again)
    return pre + inc - c;
}

// 64 < L <= lds_limit: a block per segment of blist; the segment in LDS, padded to a power of two, a
// bitonic sort, heads, a block scan per 256 words.  The whole segment is in LDS before anything is
// written, so the distinct words go back in place.
__global__ void __launch_bounds__(SJ_THREADS)
subj_sort_block(uint32_t* __restrict__ leaf, const uint64_t* __restrict__ loff, unsigned long long* __restrict__ cnt,
                uint32_t n, const uint32_t* __restrict__ blist, uint32_t lds_limit) {
    extern __shared__ uint32_t s[];                         // lds_limit words
    __shared__ uint32_t wtot[SJ_WAVES];
    const uint32_t t = blist[blockIdx.x];
    const uint32_t L = (uint32_t)min((unsigned long long)lds_limit, cnt[(uint64_t)n + t]);
    const uint64_t base = loff[t];
    uint32_t P = 128;
    while (P < L) P <<= 1;                                  // <= lds_limit, itself a power of two >= 128
    for (uint32_t i = threadIdx.x; i < P; i += SJ_THREADS) s[i] = i < L ? leaf[base + i] : SJ_PAD;
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += SJ_THREADS) {
                const uint32_t o = i ^ j;
                if (o > i) {
                    const uint32_t a = s[i], b = s[o];
                    if ((a > b) == ((i & k) == 0)) {
                        s[i] = b;
                        s[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    uint32_t run = 0;
    for (uint32_t tb = 0; tb < L; tb += SJ_THREADS) {       // (block-uniform)
        const uint32_t i = tb + threadIdx.x;
        const uint32_t v = i < L ? s[i] : SJ_PAD;
        const bool head = i < L && (i == 0 || v != s[i - 1]);
        uint32_t total;
        const uint32_t pre = block_exclusive(head ? 1u : 0u, wtot, total);
        if (head) leaf[base + run + pre] = v;
        run += total;
    }
    if (threadIdx.x == 0) cnt[t] = run;
}

// the global class: key = the segment's start in the key buffer << 32 | word, so that one radix sort
// leaves every segment sorted in its own range [gstart, gstart + L).  Blocks (k, 0 .. gridDim.y) share
// segment k.
__global__ void __launch_bounds__(SJ_THREADS)
subj_global_keys(const uint32_t* __restrict__ leaf, const uint64_t* __restrict__ loff,
                 const unsigned long long* __restrict__ cnt, uint32_t n, const uint32_t* __restrict__ glist,
                 const unsigned long long* __restrict__ gstart, uint64_t gitems, uint64_t* __restrict__ keys) {
    const uint32_t t = glist[blockIdx.x];
    const uint64_t L = cnt[(uint64_t)n + t], base = loff[t], g = gstart[blockIdx.x];
    if (g + L > gitems) return;                             // (never: the starts were handed out of gitems)
    for (uint64_t i = (uint64_t)blockIdx.y * SJ_THREADS + threadIdx.x; i < L; i += (uint64_t)gridDim.y * SJ_THREADS)
        keys[g + i] = (g << 32) | leaf[base + i];
}

// a block per global segment streams over its sorted keys, a tile of 256 x SJ_STREAM_ITEMS at a time
// (a thread's keys are consecutive, read into registers before the tile's writes), and appends the
// tile's distinct words at leaf[loff[t] ...).  It reads the sort's output and writes leaf[], and never
// writes more words than it has read.
__global__ void __launch_bounds__(SJ_THREADS)
subj_unique_stream(const uint64_t* __restrict__ sorted, const unsigned long long* __restrict__ gstart,
                   const uint32_t* __restrict__ glist, const uint64_t* __restrict__ loff, uint64_t gitems,
                   unsigned long long* __restrict__ cnt, uint32_t n, uint32_t* __restrict__ leaf) {
    __shared__ uint32_t wtot[SJ_WAVES];
    const uint32_t t = glist[blockIdx.x];
    const uint64_t L = cnt[(uint64_t)n + t], base = loff[t], g = gstart[blockIdx.x];
    if (g + L > gitems) return;                             // (never, as above)
    uint64_t run = 0;
    for (uint64_t tb = 0; tb < L; tb += (uint64_t)SJ_THREADS * SJ_STREAM_ITEMS) {    // (block-uniform)
        const uint64_t i0 = tb + (uint64_t)threadIdx.x * SJ_STREAM_ITEMS;
        uint32_t v[SJ_STREAM_ITEMS];
        uint32_t heads = 0, c = 0;
        uint32_t below = (i0 > 0 && i0 < L) ? (uint32_t)sorted[g + i0 - 1] : SJ_PAD;
#pragma unroll
        for (uint32_t e = 0; e < SJ_STREAM_ITEMS; ++e) {
            v[e] = SJ_PAD;
            if (i0 + e < L) {
                v[e] = (uint32_t)sorted[g + i0 + e];
                if (i0 + e == 0 || v[e] != below) {
                    heads |= 1u << e;
                    ++c;
                }
                below = v[e];
            }
        }
        uint32_t total;
        uint64_t o = base + run + block_exclusive(c, wtot, total);
#pragma unroll
        for (uint32_t e = 0; e < SJ_STREAM_ITEMS; ++e)
            if (heads & (1u << e)) leaf[o++] = v[e];
        run += total;
    }
    if (threadIdx.x == 0) cnt[t] = run;
}

// out[j] for j < total: the query whose output range holds j (the last one starting at or before j:
// the queries without output before it share its start), then the word of its window
__global__ void __launch_bounds__(SJ_THREADS)
subj_emit(const uint32_t* __restrict__ leaf, const uint64_t* __restrict__ loff, const SWindow* __restrict__ wins,
          uint32_t n, uint64_t total, uint32_t* __restrict__ out) {
    for (uint64_t j = (uint64_t)blockIdx.x * SJ_THREADS + threadIdx.x; j < total; j += (uint64_t)gridDim.x * SJ_THREADS) {
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (wins[mid].off <= j) lo = mid;
            else hi = mid;
        }
        const SWindow w = wins[lo];
        out[j] = leaf[loff[lo] + w.first + (j - w.off)];
    }
}

}  // namespace

struct SubjectsState {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev[SUBJECTS_STAGES + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // per node: the scan (8 B) and the compacted id-leaf words (4 B, sized for the bound: every node)
    SBuf scan, leaf, tmp;
    // per tree: loff (8 B), ucount / leaves / set_leaves and the class counters (8 B each), the class
    // lists (4 B each), the global segments' starts (8 B), the windows (16 B)
    SBuf loff, cnt, blist, glist, gstart, wins;
    SBuf keys_in, keys_out;          // the global class: 8 B per leaf, twice (the sort is out of place)
    SBuf out;                        // 4 B per emitted id
    // big workspaces do not linger
    void trim() {
        for (SBuf* b : {&scan, &leaf, &tmp, &keys_in, &keys_out, &out, &loff, &cnt, &blist, &glist, &gstart, &wins})
            if (b->cap > (256ull << 20)) b->release();
    }
    ~SubjectsState() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

void SubjectsStateDeleter::operator()(SubjectsState* s) const { delete s; }

uint32_t subjects_lds_limit() {
    const char* e = getenv("KETO_SUBJECTS_LDS");
    if (!e) return 2048;
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end == e || *end || v < 128 || v > 8192 || (v & (v - 1)) != 0)
        throw Error{KETO_E_INVALID, "KETO_SUBJECTS_LDS must be a power of two in [128, 8192]"};
    return (uint32_t)v;
}

void subjects_flatten(Snapshot& S, SubjectsCache& C, ExpandOnDevice& keep, const ExpandResult& ex,
                      const uint32_t* page_size, const uint32_t* page, uint32_t n, SubjectsResult& out) {
    const uint32_t lds_limit = subjects_lds_limit();
    const DevView V = device_view(S);                        // KETO_E_HIP on a host-only snapshot
    out.status.assign(n, KETO_SUBJECTS_OK);
    out.offsets.assign((uint64_t)n + 1, 0);
    out.next_page.assign(n, 0);
    out.totals.assign(n, 0);
    out.leaves.assign(n, 0);
    out.set_leaves.assign(n, 0);
    out.ids = nullptr;
    for (uint32_t i = 0; i < n; ++i)
        out.status[i] = ex.status[i] == KETO_EXPAND_NOT_FOUND   ? KETO_SUBJECTS_NOT_FOUND
                        : ex.status[i] == KETO_EXPAND_UNDECIDED ? KETO_SUBJECTS_UNDECIDED
                                                                : KETO_SUBJECTS_OK;
    const ResidentArena& A = keep.arena;
    if (n == 0 || A.n_nodes == 0) {                          // no tree has a node: every count is 0
        if (keep.hold.owns_lock()) keep.hold.unlock();
        return;
    }
    std::lock_guard<std::mutex> lk(C.mu);                    // after D.mu (keep.hold)
    HIP_OK(hipSetDevice(V.device));
    if (!C.state) C.state.reset(new SubjectsState());
    SubjectsState& W = *C.state;
    if (W.device != V.device) {
        if (W.device >= 0) throw Error{KETO_E_INVALID, "keto_subjects_batch: the snapshot moved to another device"};
        W.device = V.device;
    }
    if (!W.stream) HIP_OK(hipStreamCreateWithFlags(&W.stream, hipStreamNonBlocking));
    for (hipEvent_t& x : W.ev)
        if (!x) HIP_OK(hipEventCreate(&x));
    hipStream_t st = W.stream;
    // whatever happens below, nothing of this call is still in flight when the caller lets go of the
    // arena (a kernel reading an arena that the next expand overwrites would index with garbage)
    struct Drain {
        hipStream_t st;
        ~Drain() { (void)hipStreamSynchronize(st); }
    } drain{st};

    const uint64_t N = A.n_nodes;
    uint64_t* d_scan = W.scan.get<uint64_t>(N);
    uint32_t* d_leaf = W.leaf.get<uint32_t>(N);
    uint64_t* d_loff = W.loff.get<uint64_t>((uint64_t)n + 1);
    unsigned long long* d_cnt = W.cnt.get<unsigned long long>(3ull * n + CTR_N);
    unsigned long long* d_ctr = d_cnt + 3ull * n;
    uint32_t* d_blist = W.blist.get<uint32_t>(n);
    uint32_t* d_glist = W.glist.get<uint32_t>(n);
    unsigned long long* d_gstart = W.gstart.get<unsigned long long>(n);

    // ---- the passes over the arena
    HIP_OK(hipEventRecord(W.ev[0], st));
    HIP_OK(hipMemsetAsync(d_cnt, 0, (3ull * n + CTR_N) * sizeof(unsigned long long), st));
    {
        hipcub::TransformInputIterator<uint64_t, IdLeaf, const keto_tree_node*> flags(A.d_nodes, IdLeaf{});
        size_t tb = 0;
        HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flags, d_scan, N, st));
        void* tmp = W.tmp.get<uint8_t>(tb);
        HIP_OK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, flags, d_scan, N, st));
    }
    hipLaunchKernelGGL(subj_compact, dim3((unsigned)std::min<uint64_t>((N + SJ_THREADS - 1) / SJ_THREADS, 16384)),
                       dim3(SJ_THREADS), 0, st, A.d_nodes, N, (const uint64_t*)d_scan, A.d_toff, n, d_leaf, d_cnt + 2ull * n);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(subj_segments, dim3(n / SJ_THREADS + 1), dim3(SJ_THREADS), 0, st, A.d_nodes, N,
                       (const uint64_t*)d_scan, A.d_toff, n, lds_limit, d_loff, d_cnt, d_blist, d_glist, d_gstart, d_ctr);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(W.ev[1], st));
    unsigned long long ctr[CTR_N] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    keep.hold.unlock();                                      // the arena is no longer read

    // ---- sort and unique per segment, by class
    hipLaunchKernelGGL(subj_sort_wave, dim3((n + SJ_WAVES - 1) / SJ_WAVES), dim3(SJ_THREADS), 0, st, d_leaf,
                       (const uint64_t*)d_loff, d_cnt, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(W.ev[2], st));
    if (ctr[CTR_BLOCK]) {
        hipLaunchKernelGGL(subj_sort_block, dim3((unsigned)ctr[CTR_BLOCK]), dim3(SJ_THREADS), lds_limit * sizeof(uint32_t), st,
                           d_leaf, (const uint64_t*)d_loff, d_cnt, n, (const uint32_t*)d_blist, lds_limit);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(W.ev[3], st));
    if (ctr[CTR_GLOBAL]) {
        const uint64_t G = ctr[CTR_GITEMS];
        if (G > (uint64_t)INT_MAX)
            throw Error{KETO_E_RANGE, "keto_subjects_batch: more than 2^31 leaves in segments past KETO_SUBJECTS_LDS"};
        uint64_t* d_kin = W.keys_in.get<uint64_t>(G);
        uint64_t* d_kout = W.keys_out.get<uint64_t>(G);
        const unsigned chunks = (unsigned)std::min<uint64_t>(SJ_KEY_CHUNKS, (G + SJ_THREADS - 1) / SJ_THREADS);
        hipLaunchKernelGGL(subj_global_keys, dim3((unsigned)ctr[CTR_GLOBAL], chunks), dim3(SJ_THREADS), 0, st,
                           (const uint32_t*)d_leaf, (const uint64_t*)d_loff, (const unsigned long long*)d_cnt, n,
                           (const uint32_t*)d_glist, (const unsigned long long*)d_gstart, G, d_kin);
        HIP_OK(hipGetLastError());
        int end_bit = 32;                                    // the words, then the bits of the segment starts
        while (end_bit < 64 && ((G - 1) >> (end_bit - 32))) ++end_bit;
        size_t tb = 0;
        HIP_OK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, (const uint64_t*)d_kin, d_kout, (int)G, 0, end_bit, st));
        void* tmp = W.tmp.get<uint8_t>(tb);
        HIP_OK(hipcub::DeviceRadixSort::SortKeys(tmp, tb, (const uint64_t*)d_kin, d_kout, (int)G, 0, end_bit, st));
        hipLaunchKernelGGL(subj_unique_stream, dim3((unsigned)ctr[CTR_GLOBAL]), dim3(SJ_THREADS), 0, st, (const uint64_t*)d_kout,
                           (const unsigned long long*)d_gstart, (const uint32_t*)d_glist, (const uint64_t*)d_loff, G, d_cnt,
                           n, d_leaf);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(W.ev[4], st));

    // ---- the counts -> totals, tokens, windows, the pinned block's size
    struct Block {
        void* p = nullptr;
        ~Block() { pinned_give(p); }
    } counts, block;
    counts.p = pinned_take(3ull * n * sizeof(uint64_t));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are 64-bit");
    HIP_OK(hipMemcpyAsync(counts.p, d_cnt, 3ull * n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const uint64_t* ucount = static_cast<const uint64_t*>(counts.p);
    std::vector<SWindow> wins(n);
    uint64_t total_out = 0;
    for (uint32_t i = 0; i < n; ++i) {
        wins[i] = SWindow{0, total_out};
        out.offsets[i] = total_out;
        out.leaves[i] = ucount[(uint64_t)n + i];
        out.set_leaves[i] = ucount[2ull * n + i];
        const uint64_t tot = ucount[i];
        const uint64_t size = page_size[i] ? page_size[i] : S.page_size;
        const uint64_t pg = std::max<uint32_t>(page[i], 1u);
        const uint64_t first = (pg - 1) * size;              // < 2^63
        const uint64_t k = tot > first ? std::min(size, tot - first) : 0;
        out.totals[i] = tot;
        out.next_page[i] = pg >= (tot + size - 1) / size ? 0 : pg + 1;
        wins[i].first = first;
        total_out += k;
    }
    out.offsets[n] = total_out;
    if (total_out) {
        uint32_t* d_out = W.out.get<uint32_t>(total_out);
        SWindow* d_wins = W.wins.get<SWindow>(n);
        HIP_OK(hipMemcpyAsync(d_wins, wins.data(), (uint64_t)n * sizeof(SWindow), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(subj_emit, dim3((unsigned)std::min<uint64_t>((total_out + SJ_THREADS - 1) / SJ_THREADS, 16384)),
                           dim3(SJ_THREADS), 0, st, (const uint32_t*)d_leaf, (const uint64_t*)d_loff, (const SWindow*)d_wins, n,
                           total_out, d_out);
        HIP_OK(hipGetLastError());
        block.p = pinned_take(total_out * sizeof(uint32_t));
        HIP_OK(hipMemcpyAsync(block.p, d_out, total_out * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipEventRecord(W.ev[5], st));
    HIP_OK(hipStreamSynchronize(st));
    for (uint32_t k = 0; k < SUBJECTS_STAGES; ++k) HIP_OK(hipEventElapsedTime(&out.stage_ms[k], W.ev[k], W.ev[k + 1]));
    HIP_OK(hipEventElapsedTime(&out.flatten_ms, W.ev[0], W.ev[5]));
    out.ids = static_cast<uint32_t*>(block.p);
    block.p = nullptr;
    W.trim();
}

}  // namespace keto
