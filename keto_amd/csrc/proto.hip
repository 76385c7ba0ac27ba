// acl.SubjectTree protobuf encoding of expand trees on the GPU (keto_tree_proto_all_device): the
// bytes proto.Marshal gives for Tree.ToProto() (internal/expand/tree.go:165-188;
// proto/ory/keto/acl/v1alpha1/expand_service.proto, acl.proto), the same bytes as the host encoder
// keto_tree_proto_all (capi.cpp), from the node arena and the snapshot's strings resident on the
// device.  SURVEY.md 8(f) row 3: "expand tree materialization to proto directly from the GPU".
//
// A tree is pre-order nodes {subject, leaf | n_children}.  Its encoding is every node's header in
// pre-order -- [children tag 0x1A + varint(subtree size), except the root] [node_type 0x08, 1 union |
// 4 leaf] [subject tag 0x12 + varint(subject size)] [subject] -- so
//   1. per node (parallel): the subject's encoded size;
//   2. per tree (one lane, reverse pre-order with a stack kept in the tree's own slice of a
//      scratch array): every union node's subtree size.  Leaves (most nodes: a group's members)
//      are sized in parallel; a run of consecutive leaves is one step and one stack entry of the
//      serial pass, its children-field bytes a difference of prefix sums -- so a hub tree costs
//      its union nodes and leaf runs, not its leaves;
//   3. per node: its header length; one exclusive scan over all nodes gives every node's byte
//      offset, the trees' offsets included;
//   4. per node (parallel): write the header and the subject's strings.
//
// keto_tree_json_all_device (the "json_" kernels below) encodes the same trees as Tree.MarshalJSON
// text from the same tables, with the same leaf-run serial pass: it finds where every union closes
// instead of how large it is.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_check.hpp"
#include "json_runs.hpp"
#include "list.hpp"
#include "parallel.hpp"
#include "snapshot.hpp"

namespace keto {

namespace {

constexpr uint32_t NONE_STR = 0xFFFFFFFFu;     // an absent (empty) field of a subject

template <class T>
T* palloc(uint64_t n) {
    void* p = nullptr;
    if (n == 0) n = 1;
    const hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) throw Error{KETO_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)};
    return (T*)p;
}
struct PBuf {                     // a grow-only device buffer, freed with its owner
    void* p = nullptr;
    uint64_t cap = 0;
    PBuf() = default;
    PBuf(const PBuf&) = delete;
    PBuf& operator=(const PBuf&) = delete;
    template <class T>
    T* get(uint64_t n) {
        const uint64_t want = std::max<uint64_t>(1, n * sizeof(T));
        if (want > cap) {
            release();
            const uint64_t c = std::max<uint64_t>(want, cap + cap / 4);   // some headroom for the next call
            p = palloc<uint8_t>(c);
            cap = c;
        }
        return (T*)p;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    ~PBuf() { release(); }
};

// the strings a subject can name: snapshot strings, namespace names, the arena's extra strings
struct StrTab {
    const uint8_t* bytes;
    const uint64_t* off;          // n + 1
    uint32_t n;
};
struct Tables {
    StrTab strs, ns, extra;
    const int32_t* row_ns;        // namespace config index of a row, -1 = none ("")
    const uint32_t* row_obj;      // string id or ANY
    const uint32_t* row_rel;
    uint32_t n_rows;
    const int32_t* ov_ns;         // the arena's overlay rows (batch-local wildcard roots)
    const uint32_t* ov_obj;
    const uint32_t* ov_rel;
    uint32_t ov_base, n_ov;
    uint32_t extra_base;
};

struct Sub {                      // a subject's strings: (table, index) pairs; index NONE = ""
    bool set;
    const StrTab* t[3];
    uint32_t i[3];
};

__device__ inline uint32_t slen_of(const StrTab* t, uint32_t i) {
    return (t && i < t->n) ? (uint32_t)(t->off[i + 1] - t->off[i]) : 0u;
}

__device__ inline Sub subject_of(const Tables& T, uint32_t ref) {
    Sub s;
    s.set = (ref & EDGE_SET) != 0;
    const uint32_t v = ref & EDGE_VAL;
    if (!s.set) {
        s.t[0] = (v >= T.extra_base && v - T.extra_base < T.extra.n) ? &T.extra : &T.strs;
        s.i[0] = (v >= T.extra_base && v - T.extra_base < T.extra.n) ? v - T.extra_base : v;
        s.t[1] = s.t[2] = nullptr;
        s.i[1] = s.i[2] = NONE_STR;
        return s;
    }
    int32_t ns;
    uint32_t obj, rel;
    if (v >= T.ov_base && v - T.ov_base < T.n_ov) {
        ns = T.ov_ns[v - T.ov_base];
        obj = T.ov_obj[v - T.ov_base];
        rel = T.ov_rel[v - T.ov_base];
    } else if (v < T.n_rows) {
        ns = T.row_ns[v];
        obj = T.row_obj[v];
        rel = T.row_rel[v];
    } else {
        ns = -1;
        obj = rel = ANY;
    }
    s.t[0] = &T.ns;
    s.i[0] = ns < 0 ? NONE_STR : (uint32_t)ns;
    s.t[1] = &T.strs;
    s.i[1] = obj == ANY ? NONE_STR : obj;
    s.t[2] = &T.strs;
    s.i[2] = rel == ANY ? NONE_STR : rel;
    return s;
}

__host__ __device__ inline uint32_t vlen(uint64_t v) {
    uint32_t k = 1;
    while (v >= 0x80) {
        v >>= 7;
        ++k;
    }
    return k;
}
__host__ __device__ inline uint64_t flen(uint64_t n) { return 1 + vlen(n) + n; }

// bytes of the Subject message (oneof id, present even when "" | set {namespace, object, relation;
// empty strings omitted})
__device__ inline uint64_t subject_len(const Sub& s) {
    if (!s.set) return flen(slen_of(s.t[0], s.i[0]));
    uint64_t in = 0;
    for (int f = 0; f < 3; ++f) {
        const uint32_t l = slen_of(s.t[f], s.i[f]);
        if (l) in += flen(l);
    }
    return flen(in);
}

// per node: the subject's size; a leaf's subtree size and its children-field bytes (leafw); the
// node's own position if it is a union node, else -1 (max-scanned into "last union at or before")
__global__ void __launch_bounds__(256) proto_slen(const keto_tree_node* __restrict__ nd, uint64_t n, Tables T,
                                                  uint64_t* __restrict__ slen, uint64_t* __restrict__ size,
                                                  uint64_t* __restrict__ leafw, int64_t* __restrict__ uni) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t l = subject_len(subject_of(T, nd[k].subject));
    slen[k] = l;
    const bool leaf = (nd[k].info & 0x80000000u) != 0;
    const uint64_t z = 2 + flen(l);
    size[k] = z;                                          // final for leaves; unions: proto_sizes
    leafw[k] = leaf ? flen(z) : 0;
    uni[k] = leaf ? -1 : (int64_t)k;
}

// one lane per tree: union nodes' subtree sizes in reverse pre-order.  Stack entries (2 words in
// the tree's slice of `st`): a finished union child {UNION, size}, or a run of leaf children
// {first, end} whose children-field bytes are lp[end] - lp[first] (lp = exclusive prefix of leafw);
// last_union[j] = the last union node at or before j (runs end there)
constexpr uint64_t ST_UNION = ~0ull;
__global__ void __launch_bounds__(256) proto_sizes(const keto_tree_node* __restrict__ nd,
                                                   const uint64_t* __restrict__ toff, uint32_t n_trees,
                                                   const uint64_t* __restrict__ lp,
                                                   const int64_t* __restrict__ last_union,
                                                   uint64_t* __restrict__ size, uint64_t* __restrict__ st) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_trees) return;
    const uint64_t b = toff[t], e = toff[t + 1];
    uint64_t* const stack = st + 2 * b;
    uint64_t sp = 0;
    uint64_t k = e;
    while (k > b) {
        --k;
        if (nd[k].info & 0x80000000u) {                   // the run of leaves ending at k
            const int64_t u = last_union[k];
            const uint64_t first = (u < 0 || (uint64_t)u < b) ? b : (uint64_t)u + 1;
            stack[2 * sp] = first;
            stack[2 * sp + 1] = k + 1;
            ++sp;
            k = first;
            continue;
        }
        uint32_t need = nd[k].info & 0x7FFFFFFFu;
        uint64_t z = size[k];                             // 2 + the subject field
        while (need > 0 && sp > 0) {
            uint64_t* top = stack + 2 * (sp - 1);
            if (top[0] == ST_UNION) {
                z += flen(top[1]);
                --need;
                --sp;
                continue;
            }
            const uint64_t m = top[1] - top[0], take = m < need ? m : need;   // the first `take` leaves
            z += lp[top[0] + take] - lp[top[0]];
            need -= (uint32_t)take;
            top[0] += take;
            if (top[0] == top[1]) --sp;
        }
        size[k] = z;
        stack[2 * sp] = ST_UNION;
        stack[2 * sp + 1] = z;
        ++sp;
    }
}

// header bytes of every node (tree roots have no children-field prefix)
__global__ void __launch_bounds__(256) proto_hdr(const uint64_t* __restrict__ slen, const uint64_t* __restrict__ size,
                                                 const uint8_t* __restrict__ is_root, uint64_t n,
                                                 uint64_t* __restrict__ hdr) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    hdr[k] = (is_root[k] ? 0u : 1u + vlen(size[k])) + 2u + flen(slen[k]);
}

__global__ void __launch_bounds__(256) proto_roots(const uint64_t* __restrict__ toff, uint32_t n_trees,
                                                   uint8_t* __restrict__ is_root) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_trees && toff[t] < toff[t + 1]) is_root[toff[t]] = 1;
}

__device__ inline uint8_t* put_varint(uint8_t* p, uint64_t v) {
    while (v >= 0x80) {
        *p++ = (uint8_t)(v | 0x80);
        v >>= 7;
    }
    *p++ = (uint8_t)v;
    return p;
}
__device__ inline uint8_t* put_str(uint8_t* p, uint8_t tag, const StrTab* t, uint32_t i) {
    const uint32_t l = slen_of(t, i);
    *p++ = tag;
    p = put_varint(p, l);
    if (l) {
        const uint8_t* s = t->bytes + t->off[i];
        for (uint32_t c = 0; c < l; ++c) p[c] = s[c];
    }
    return p + l;
}

__global__ void __launch_bounds__(256) proto_write(const keto_tree_node* __restrict__ nd, uint64_t n, Tables T,
                                                   const uint64_t* __restrict__ slen, const uint64_t* __restrict__ size,
                                                   const uint8_t* __restrict__ is_root, const uint64_t* __restrict__ pos,
                                                   uint8_t* __restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint8_t* p = out + pos[k];
    if (!is_root[k]) {
        *p++ = 0x1A;
        p = put_varint(p, size[k]);
    }
    *p++ = 0x08;
    *p++ = (nd[k].info & 0x80000000u) ? 4 : 1;
    *p++ = 0x12;
    p = put_varint(p, slen[k]);
    const Sub s = subject_of(T, nd[k].subject);
    if (!s.set) {
        put_str(p, 0x0A, s.t[0], s.i[0]);
        return;
    }
    uint64_t in = 0;
    for (int f = 0; f < 3; ++f) {
        const uint32_t l = slen_of(s.t[f], s.i[f]);
        if (l) in += flen(l);
    }
    *p++ = 0x12;
    p = put_varint(p, in);
    const uint8_t tags[3] = {0x0A, 0x12, 0x1A};
    for (int f = 0; f < 3; ++f)
        if (slen_of(s.t[f], s.i[f])) p = put_str(p, tags[f], s.t[f], s.i[f]);
}

__global__ void __launch_bounds__(256) proto_tree_offsets(const uint64_t* __restrict__ toff, uint32_t n_trees,
                                                          const uint64_t* __restrict__ pos, uint64_t total,
                                                          uint64_t n_nodes, uint64_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_trees) return;
    out[t] = toff[t] < n_nodes ? pos[toff[t]] : total;
}

// ---- Tree.MarshalJSON text (keto_tree_json_all_device): tree_json / subject_json / json_escape of
// capi.cpp, byte for byte.  A node's text is not contiguous -- a union with children opens before
// its first child and closes behind its last -- so the output is laid out as, for every node k in
// pre-order: [the closes of the unions whose subtree ends right before k, innermost first]
// [the "null"s of the nil trees in front of a tree root] [a comma unless k is a first child or a
// root] [k's own text: everything for a leaf or a childless union, the open text for a union with
// children].  One exclusive scan of these per-node byte counts places everything.

// json_escape's classification of the sequence starting at s[i]: the bytes it consumes (1 for an
// invalid one) and the bytes it emits; raw = copy the consumed bytes unchanged
struct Esc {
    uint32_t take, emit;
    bool raw;
    uint32_t cp;                  // the code point of an escaped multi-byte sequence, 0xFFFD if invalid
};
__device__ inline Esc esc_at(const uint8_t* s, uint32_t i, uint32_t l) {
    const uint8_t c = s[i];
    if (c < 0x80) {
        if (c == '"' || c == '\\' || c == '\n' || c == '\r' || c == '\t') return Esc{1, 2, false, c};
        if (c < 0x20 || c == '<' || c == '>' || c == '&') return Esc{1, 6, false, c};
        return Esc{1, 1, true, c};
    }
    const uint32_t len = (c >> 5) == 6 ? 2 : (c >> 4) == 14 ? 3 : (c >> 3) == 30 ? 4 : 0;
    bool ok = len != 0 && (uint64_t)i + len <= l;
    uint32_t cp = 0;
    if (ok) {
        cp = c & (0x7Fu >> len);
        for (uint32_t k = 1; k < len; ++k) {
            const uint8_t cc = s[i + k];
            if ((cc >> 6) != 2) {
                ok = false;
                break;
            }
            cp = (cp << 6) | (cc & 0x3Fu);
        }
        if (ok && ((len == 2 && cp < 0x80) || (len == 3 && cp < 0x800) || (len == 4 && (cp < 0x10000 || cp > 0x10FFFF)) ||
                   (cp >= 0xD800 && cp <= 0xDFFF)))
            ok = false;
    }
    if (!ok) return Esc{1, 6, false, 0xFFFDu};
    if (cp == 0x2028 || cp == 0x2029) return Esc{len, 6, false, cp};
    return Esc{len, len, true, cp};
}
// bytes of json_escape's output for a string of the tables, the quotes included
__device__ inline uint64_t esc_len(const StrTab* t, uint32_t i) {
    const uint32_t l = slen_of(t, i);
    uint64_t n = 2;
    if (!l) return n;
    const uint8_t* s = t->bytes + t->off[i];
    for (uint32_t c = 0; c < l;) {
        const Esc e = esc_at(s, c, l);
        n += e.emit;
        c += e.take;
    }
    return n;
}
__device__ inline uint8_t* put_lit(uint8_t* p, const char* s, uint32_t n) {
    for (uint32_t c = 0; c < n; ++c) p[c] = (uint8_t)s[c];
    return p + n;
}
#define PUT_LIT(p, s) put_lit((p), (s), (uint32_t)sizeof(s) - 1)
__device__ inline uint8_t* put_esc(uint8_t* p, const StrTab* t, uint32_t i) {
    const uint32_t l = slen_of(t, i);
    *p++ = '"';
    if (l) {
        const uint8_t* s = t->bytes + t->off[i];
        for (uint32_t c = 0; c < l;) {
            const Esc e = esc_at(s, c, l);
            if (e.raw) {
                for (uint32_t k = 0; k < e.take; ++k) *p++ = s[c + k];
            } else if (e.emit == 2) {
                *p++ = '\\';
                *p++ = e.cp == '\n' ? 'n' : e.cp == '\r' ? 'r' : e.cp == '\t' ? 't' : (uint8_t)e.cp;
            } else {
                *p++ = '\\';
                *p++ = 'u';
                for (int sh = 12; sh >= 0; sh -= 4) {
                    const uint32_t h = (e.cp >> sh) & 15u;
                    *p++ = (uint8_t)(h < 10 ? '0' + h : 'a' + (h - 10));
                }
            }
            c += e.take;
        }
    }
    *p++ = '"';
    return p;
}

// subject_json: ,"subject_id":"..."} | ,"subject_set":{"namespace":"...","object":"...","relation":"..."}}
__device__ inline uint64_t subject_json_len(const Sub& s) {
    if (!s.set) return 14 + esc_len(s.t[0], s.i[0]) + 1;
    return 28 + esc_len(s.t[0], s.i[0]) + 10 + esc_len(s.t[1], s.i[1]) + 12 + esc_len(s.t[2], s.i[2]) + 2;
}
__device__ inline uint8_t* put_subject_json(uint8_t* p, const Sub& s) {
    if (!s.set) {
        p = PUT_LIT(p, ",\"subject_id\":");
        p = put_esc(p, s.t[0], s.i[0]);
    } else {
        p = PUT_LIT(p, ",\"subject_set\":{\"namespace\":");
        p = put_esc(p, s.t[0], s.i[0]);
        p = PUT_LIT(p, ",\"object\":");
        p = put_esc(p, s.t[1], s.i[1]);
        p = PUT_LIT(p, ",\"relation\":");
        p = put_esc(p, s.t[2], s.i[2]);
        *p++ = '}';
    }
    *p++ = '}';
    return p;
}
__device__ inline bool json_open_union(const keto_tree_node& x) {     // a union with children: closes later
    return (x.info & 0x80000000u) == 0 && (x.info & 0x7FFFFFFFu) != 0;
}

// per node: own = the text at the node's place (all of a leaf's or a childless union's, the open
// text of a union with children), clen = the close text a union with children writes behind its
// last child; uni as in proto_slen
__global__ void __launch_bounds__(256) json_own(const keto_tree_node* __restrict__ nd, uint64_t n, Tables T,
                                                uint64_t* __restrict__ own, uint64_t* __restrict__ clen,
                                                int64_t* __restrict__ uni) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const keto_tree_node x = nd[k];
    const uint64_t sl = subject_json_len(subject_of(T, x.subject));
    const bool leaf = (x.info & 0x80000000u) != 0;
    if (json_open_union(x)) {
        own[k] = 28;                                      // {"type":"union","children":[
        clen[k] = 1 + sl;                                 // ] and the subject
    } else {
        own[k] = (leaf ? 14 : 15) + sl;                   // {"type":"leaf" | {"type":"union"
        clen[k] = 0;
    }
    uni[k] = leaf ? -1 : (int64_t)k;
}

// pre[k] = the "null" bytes in front of tree root k, -1 for every other node; pre[n_nodes] = the
// ones behind the last node.  run[t] = the "null" bytes of the node-less trees right before tree t
// (t = n_trees: at the end).
__global__ void __launch_bounds__(256) json_roots(const uint64_t* __restrict__ toff, uint32_t n_trees,
                                                  const uint64_t* __restrict__ run, uint64_t n_nodes,
                                                  int64_t* __restrict__ pre) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_trees && toff[t] < toff[t + 1]) pre[toff[t]] = (int64_t)run[t];
    if (t == n_trees) pre[n_nodes] = (int64_t)run[n_trees];
}

// one lane per tree, reverse pre-order with leaf runs as single steps (proto_sizes): where every
// union with children closes.  Stack entries (2 words in the tree's slice of `st`): a finished
// union {ST_UNION, end of its subtree} or a run of leaves {first, end}.  Union u closes right before
// node cend[u] = the end of its last child; the unions that close there are reached innermost
// first, so close_at[cend[u]] before u's add is u's byte offset in that group (coff[u]).  A lane
// writes close_at in (b, e] only: no two trees share an entry.  A node list cut short closes what
// is open at its end, as tree_json does.
__global__ void __launch_bounds__(256) json_closes(const keto_tree_node* __restrict__ nd,
                                                   const uint64_t* __restrict__ toff, uint32_t n_trees,
                                                   const int64_t* __restrict__ last_union,
                                                   const uint64_t* __restrict__ clen, uint64_t* __restrict__ close_at,
                                                   uint64_t* __restrict__ cend, uint64_t* __restrict__ coff,
                                                   uint64_t* __restrict__ st) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_trees) return;
    const uint64_t b = toff[t], e = toff[t + 1];
    uint64_t* const stack = st + 2 * b;
    uint64_t sp = 0;
    uint64_t k = e;
    while (k > b) {
        --k;
        if (nd[k].info & 0x80000000u) {                   // the run of leaves ending at k
            const int64_t u = last_union[k];
            const uint64_t first = (u < 0 || (uint64_t)u < b) ? b : (uint64_t)u + 1;
            stack[2 * sp] = first;
            stack[2 * sp + 1] = k + 1;
            ++sp;
            k = first;
            continue;
        }
        uint32_t need = nd[k].info & 0x7FFFFFFFu;
        const bool open = need != 0;
        uint64_t end = k + 1;
        while (need > 0 && sp > 0) {
            uint64_t* top = stack + 2 * (sp - 1);
            if (top[0] == ST_UNION) {
                end = top[1];
                --need;
                --sp;
                continue;
            }
            const uint64_t m = top[1] - top[0], take = m < need ? m : need;   // the first `take` leaves
            need -= (uint32_t)take;
            top[0] += take;
            end = top[0];
            if (top[0] == top[1]) --sp;
        }
        if (open) {
            const uint64_t at = close_at[end];
            coff[k] = at;
            cend[k] = end;
            close_at[end] = at + clen[k];
        }
        stack[2 * sp] = ST_UNION;
        stack[2 * sp + 1] = end;
        ++sp;
    }
}

// the bytes laid out at node k (k = n_nodes: behind the last node)
__global__ void __launch_bounds__(256) json_term(const keto_tree_node* __restrict__ nd, uint64_t n,
                                                 const uint64_t* __restrict__ own, const uint64_t* __restrict__ close_at,
                                                 const int64_t* __restrict__ pre, uint64_t* __restrict__ term) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n) return;
    const int64_t pr = pre[k];
    uint64_t z = close_at[k] + (pr < 0 ? 0 : (uint64_t)pr);
    if (k < n) z += own[k] + ((pr < 0 && k > 0 && !json_open_union(nd[k - 1])) ? 1 : 0);
    term[k] = z;
}

__global__ void __launch_bounds__(256) json_write(const keto_tree_node* __restrict__ nd, uint64_t n, Tables T,
                                                  const uint64_t* __restrict__ close_at, const int64_t* __restrict__ pre,
                                                  const uint64_t* __restrict__ cend, const uint64_t* __restrict__ coff,
                                                  const uint64_t* __restrict__ pos, uint8_t* __restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const keto_tree_node x = nd[k];
    const int64_t pr = pre[k];
    uint8_t* p = out + pos[k] + close_at[k] + (pr < 0 ? 0 : (uint64_t)pr);
    if (pr < 0 && k > 0 && !json_open_union(nd[k - 1])) *p++ = ',';
    const Sub s = subject_of(T, x.subject);
    if (json_open_union(x)) {
        PUT_LIT(p, "{\"type\":\"union\",\"children\":[");
        p = out + pos[cend[k]] + coff[k];
        *p++ = ']';
    } else if (x.info & 0x80000000u) {
        p = PUT_LIT(p, "{\"type\":\"leaf\"");
    } else {
        p = PUT_LIT(p, "{\"type\":\"union\"");
    }
    put_subject_json(p, s);
}

// per tree: its offset; a nil tree's "null".  A tree without nodes (nil, error) lies run[t] bytes
// into the "null"s in front of the next root.
__global__ void __launch_bounds__(256) json_trees(const uint64_t* __restrict__ toff, uint32_t n_trees,
                                                  const uint64_t* __restrict__ run, const uint8_t* __restrict__ nil,
                                                  const uint64_t* __restrict__ close_at, const uint64_t* __restrict__ pos,
                                                  uint64_t n_nodes, uint8_t* __restrict__ out,
                                                  uint64_t* __restrict__ offs) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_trees) return;
    if (t == n_trees) {
        if (offs) offs[t] = pos[n_nodes + 1];
        return;
    }
    const uint64_t b = toff[t];
    const uint64_t at = pos[b] + close_at[b] + run[t];
    if (offs) offs[t] = at;
    if (out && nil[t]) PUT_LIT(out + at, "null");
}

// a string table on the device from host strings (its buffers are reused by the next upload)
struct DevStrs {
    PBuf b_bytes, b_off;
    uint8_t* bytes = nullptr;
    uint64_t* off = nullptr;
    uint32_t n = 0;
    template <class Get>
    void upload(uint32_t count, Get get) {
        std::vector<uint64_t> o(count + 1, 0);
        for (uint32_t i = 0; i < count; ++i) o[i + 1] = o[i] + get(i).size();
        std::vector<uint8_t> b(std::max<uint64_t>(1, o[count]));
        for (uint32_t i = 0; i < count; ++i) {
            const std::string_view s = get(i);
            if (!s.empty()) std::memcpy(b.data() + o[i], s.data(), s.size());
        }
        bytes = b_bytes.get<uint8_t>(b.size());
        off = b_off.get<uint64_t>(o.size());
        HIP_OK(hipMemcpy(bytes, b.data(), b.size(), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(off, o.data(), o.size() * 8, hipMemcpyHostToDevice));
        n = count;
    }
    void release() {
        b_bytes.release();
        b_off.release();
        bytes = nullptr;
        off = nullptr;
        n = 0;
    }
    StrTab view() const { return StrTab{bytes, off, n}; }
};

// device_tree_proto's per-call buffers, kept across calls (one call at a time: the snapshot lock)
struct ProtoWork {
    DevStrs ex;
    PBuf ons, oobj, orel, nodes, toff, slen, size, st, root, hdr, pos, out, to, tmp, tmp3, lw, lp, uni, lu;
    PBuf jown, jclen, jcat, jpre, jcend, jcoff, jterm, jrun, jnil;      // device_tree_json's
};
// device_list_encode's, kept across calls likewise: 16 B per item (size, position), the bodies
struct ListEncWork {
    PBuf meta, sz, pos, res, tmp, out;
};

}  // namespace

// The snapshot's strings and row keys on the device (uploaded on first use, again after a write).
struct ProtoState {
    int device = 0;
    uint64_t version = ~0ull;
    DevStrs strs, ns;
    int32_t* row_ns = nullptr;
    uint32_t* row_obj = nullptr;
    uint32_t* row_rel = nullptr;
    uint32_t n_rows = 0;
    // two pinned bounce chunks for the output's D2H (d2h_staged)
    uint8_t* pin[2] = {nullptr, nullptr};
    uint64_t pin_bytes = 0;
    ProtoWork work;
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    ListEncWork list_work;
    hipEvent_t list_ev = nullptr;     // orders the list stream behind a refresh (device_list_encode)
    void release_rows() {
        if (row_ns) (void)hipFree(row_ns);
        if (row_obj) (void)hipFree(row_obj);
        if (row_rel) (void)hipFree(row_rel);
        row_ns = nullptr;
        row_obj = row_rel = nullptr;
    }
    ~ProtoState() {
        (void)hipSetDevice(device);
        strs.release();
        ns.release();
        release_rows();
        for (int i = 0; i < 2; ++i) {
            if (pin[i]) (void)hipHostFree(pin[i]);
            if (pin_ev[i]) (void)hipEventDestroy(pin_ev[i]);
        }
        if (list_ev) (void)hipEventDestroy(list_ev);
    }
};

void ProtoStateDeleter::operator()(ProtoState* p) const { delete p; }

namespace {
ProtoState& proto_state(Snapshot& S, int device) {
    if (!S.proto) {
        S.proto.reset(new ProtoState);
        S.proto->device = device;
    }
    ProtoState& P = *S.proto;
    if (P.version == S.version) return P;
    P.strs.upload((uint32_t)S.strs.size(), [&](uint32_t i) { return std::string_view(S.strs[i]); });
    P.ns.upload((uint32_t)S.ns_names.size(), [&](uint32_t i) { return std::string_view(S.ns_names[i]); });
    const uint32_t R = S.n_rows();
    std::vector<int32_t> rns(R);
    std::vector<uint32_t> robj(R), rrel(R);
    for (uint32_t r = 0; r < R; ++r) {
        const RowKey& k = S.row_key[r];
        int32_t ci = -1;
        if (k.ns != ANY_NS) {
            auto it = S.ns_by_id.find((int32_t)k.ns);
            if (it != S.ns_by_id.end()) ci = it->second;
        }
        rns[r] = ci;
        robj[r] = k.obj;
        rrel[r] = k.rel;
    }
    P.release_rows();
    P.row_ns = palloc<int32_t>(R);
    P.row_obj = palloc<uint32_t>(R);
    P.row_rel = palloc<uint32_t>(R);
    HIP_OK(hipMemcpy(P.row_ns, rns.data(), (uint64_t)R * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(P.row_obj, robj.data(), (uint64_t)R * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(P.row_rel, rrel.data(), (uint64_t)R * 4, hipMemcpyHostToDevice));
    P.n_rows = R;
    P.version = S.version;
    return P;
}
}  // namespace

// D2H of the encoded bytes into the caller's buffer.  A pinned buffer takes one DMA.  A pageable
// one (the usual case: a fresh numpy / std::vector buffer) goes through two pinned bounce chunks:
// the DMA of chunk i + 1 overlaps the host threads' copy of chunk i out of its bounce buffer, which
// also takes the first-touch page faults of the caller's buffer in parallel (a plain pageable
// hipMemcpy ran at 16.8 GB/s on config #5's 36 MB).
// KETO_PROTO_PIN_CHUNK (bytes, tests): a smaller chunk, so small outputs take the staged path.
static void d2h_staged(ProtoState& P, uint8_t* buf, const uint8_t* d_src, uint64_t total, hipStream_t st) {
    uint64_t PIN_CHUNK = 8ull << 20;
    if (const char* e = getenv("KETO_PROTO_PIN_CHUNK")) PIN_CHUNK = std::max(1ll, atoll(e));
    hipPointerAttribute_t at{};
    const bool pinned = hipPointerGetAttributes(&at, buf) == hipSuccess && at.type == hipMemoryTypeHost;
    (void)hipGetLastError();                       // pageable pointers report an error here
    if (pinned || total <= std::min<uint64_t>(1ull << 20, PIN_CHUNK)) {
        HIP_OK(hipMemcpyAsync(buf, d_src, total, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return;
    }
    if (P.pin_bytes != PIN_CHUNK) {
        for (int i = 0; i < 2; ++i) {
            if (P.pin[i]) HIP_OK(hipHostFree(P.pin[i]));
            P.pin[i] = nullptr;
        }
        P.pin_bytes = PIN_CHUNK;
    }
    for (int i = 0; i < 2; ++i) {
        if (!P.pin[i]) HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&P.pin[i]), PIN_CHUNK, hipHostMallocDefault));
        if (!P.pin_ev[i]) HIP_OK(hipEventCreateWithFlags(&P.pin_ev[i], hipEventDisableTiming));
    }
    const uint64_t n_ch = (total + PIN_CHUNK - 1) / PIN_CHUNK;
    auto issue = [&](uint64_t c) {
        const uint64_t off = c * PIN_CHUNK, len = std::min(PIN_CHUNK, total - off);
        HIP_OK(hipMemcpyAsync(P.pin[c & 1], d_src + off, len, hipMemcpyDeviceToHost, st));
        HIP_OK(hipEventRecord(P.pin_ev[c & 1], st));
    };
    issue(0);
    if (n_ch > 1) issue(1);
    const unsigned th = std::min(8u, build_threads());
    for (uint64_t c = 0; c < n_ch; ++c) {
        HIP_OK(hipEventSynchronize(P.pin_ev[c & 1]));
        const uint64_t off = c * PIN_CHUNK, len = std::min(PIN_CHUNK, total - off);
        const uint8_t* src = P.pin[c & 1];
        par_chunks(len, th, 1ull << 20, [&](uint64_t b, uint64_t e, unsigned) { memcpy(buf + off + b, src + b, e - b); });
        if (c + 2 < n_ch) issue(c + 2);
    }
}

// the arena on the device for one encoder call: its overlay rows and extra strings next to the
// snapshot's tables, its nodes and tree offsets
namespace {
struct Arena {
    Tables T;
    const keto_tree_node* nodes;
    const uint64_t* toff;
};
// res != NULL: the nodes and tree offsets are on the device already (device_expand's arena, kept
// there); only the call's tables are uploaded
Arena upload_arena(Snapshot& S, ProtoState& P, const keto_tree_node* nodes, uint64_t n_nodes, const uint64_t* tree_off,
                   uint32_t n_trees, uint32_t ov_base, const std::vector<RowKey>& ov_keys, uint32_t extra_base,
                   const std::vector<std::string>& extra, const ResidentArena* res) {
    ProtoWork& W = P.work;
    DevStrs& ex = W.ex;
    ex.upload((uint32_t)extra.size(), [&](uint32_t i) { return std::string_view(extra[i]); });
    const uint32_t n_ov = (uint32_t)ov_keys.size();
    std::vector<int32_t> ons(n_ov);
    std::vector<uint32_t> oobj(n_ov), orel(n_ov);
    for (uint32_t i = 0; i < n_ov; ++i) {
        int32_t ci = -1;
        if (ov_keys[i].ns != ANY_NS) {
            auto it = S.ns_by_id.find((int32_t)ov_keys[i].ns);
            if (it != S.ns_by_id.end()) ci = it->second;
        }
        ons[i] = ci;
        oobj[i] = ov_keys[i].obj;
        orel[i] = ov_keys[i].rel;
    }
    int32_t* d_ons = W.ons.get<int32_t>(n_ov);
    uint32_t* d_oobj = W.oobj.get<uint32_t>(n_ov);
    uint32_t* d_orel = W.orel.get<uint32_t>(n_ov);
    if (n_ov) {
        HIP_OK(hipMemcpy(d_ons, ons.data(), n_ov * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_oobj, oobj.data(), n_ov * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_orel, orel.data(), n_ov * 4, hipMemcpyHostToDevice));
    }
    Arena A;
    A.T = Tables{P.strs.view(), P.ns.view(), ex.view(), P.row_ns, P.row_obj, P.row_rel, P.n_rows, d_ons, d_oobj, d_orel,
                 ov_base, n_ov, extra_base};
    if (res) {
        A.nodes = res->d_nodes;
        A.toff = res->d_toff;
        return A;
    }
    keto_tree_node* d_nodes = W.nodes.get<keto_tree_node>(n_nodes);
    uint64_t* d_toff = W.toff.get<uint64_t>(n_trees + 1ull);
    HIP_OK(hipMemcpy(d_nodes, nodes, n_nodes * sizeof(keto_tree_node), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_toff, tree_off, (n_trees + 1ull) * 8, hipMemcpyHostToDevice));
    A.nodes = d_nodes;
    A.toff = d_toff;
    return A;
}

// Where an encoder's bytes go once their total is known: the caller's buf when it can take them
// (cap >= total), or -- `take` -- a block of that size from the pinned pool (pinned_take), handed to
// the caller through *take before anything is written to it, so that a call that fails later leaves
// the block with its owner.  NULL: nothing is written (a sizing call, or no bytes).
struct Sink {
    uint8_t* buf;
    uint64_t cap;
    uint8_t** take;
    uint8_t* at(uint64_t total) const {
        if (total == 0) return nullptr;
        if (take) return *take = static_cast<uint8_t*>(pinned_take(total));
        return buf && cap >= total ? buf : nullptr;
    }
};
}  // namespace

static uint64_t encode_proto(Snapshot& S, const keto_tree_node* nodes, const ResidentArena* res, uint64_t n_nodes,
                           const uint64_t* tree_off, uint32_t n_trees, uint32_t ov_base,
                           const std::vector<RowKey>& ov_keys, uint32_t extra_base,
                           const std::vector<std::string>& extra, const Sink& sink, uint64_t* offsets) {
    const DevView dv = device_view(S);
    HIP_OK(hipSetDevice(dv.device));
    std::lock_guard<std::mutex> lk(S.mu);
    // KETO_PROTO_TRACE=1: phase times on stderr (tooling)
    const bool trace = getenv("KETO_PROTO_TRACE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!trace) return;
        (void)hipDeviceSynchronize();
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[proto] %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
        t_last = t;
    };
    ProtoState& P = proto_state(S, dv.device);
    const hipStream_t st = 0;
    ProtoWork& W = P.work;
    const Arena A = upload_arena(S, P, nodes, n_nodes, tree_off, n_trees, ov_base, ov_keys, extra_base, extra, res);
    const Tables& T = A.T;
    const keto_tree_node* const d_nodes = A.nodes;
    const uint64_t* const d_toff = A.toff;
    lap(res ? "tables" : "upload");
    uint64_t* d_slen = W.slen.get<uint64_t>(n_nodes);
    uint64_t* d_size = W.size.get<uint64_t>(n_nodes);
    uint64_t* d_st = W.st.get<uint64_t>(2 * n_nodes);
    uint64_t* d_lw = W.lw.get<uint64_t>(n_nodes + 1);
    uint64_t* d_lp = W.lp.get<uint64_t>(n_nodes + 1);
    int64_t* d_uni = W.uni.get<int64_t>(n_nodes);
    int64_t* d_lu = W.lu.get<int64_t>(n_nodes);
    uint8_t* d_root = W.root.get<uint8_t>(n_nodes);
    uint64_t* d_hdr = W.hdr.get<uint64_t>(n_nodes + 1);
    uint64_t* d_pos = W.pos.get<uint64_t>(n_nodes + 1);
    uint64_t* d_to = W.to.get<uint64_t>(n_trees + 1ull);
    const auto g = [](uint64_t n) { return dim3((unsigned)std::max<uint64_t>(1, (n + 255) / 256)); };
    lap("alloc");
    HIP_OK(hipMemsetAsync(d_root, 0, std::max<uint64_t>(1, n_nodes), st));
    HIP_OK(hipMemsetAsync(d_hdr + n_nodes, 0, 8, st));
    HIP_OK(hipMemsetAsync(d_lw + n_nodes, 0, 8, st));
    size_t tmp_bytes = 0, tb2 = 0;
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_lw, d_lp, n_nodes + 1, st));
    HIP_OK(hipcub::DeviceScan::InclusiveScan(nullptr, tb2, d_uni, d_lu, hipcub::Max(), std::max<uint64_t>(1, n_nodes), st));
    tmp_bytes = std::max(tmp_bytes, tb2);
    if (n_nodes) {
        hipLaunchKernelGGL(proto_slen, g(n_nodes), dim3(256), 0, st, d_nodes, n_nodes, T, d_slen, d_size, d_lw, d_uni);
        lap("slen");
        void* d_t0 = W.tmp.get<uint8_t>(tmp_bytes);
        HIP_OK(hipcub::DeviceScan::ExclusiveSum(d_t0, tmp_bytes, d_lw, d_lp, n_nodes + 1, st));
        HIP_OK(hipcub::DeviceScan::InclusiveScan(d_t0, tb2, d_uni, d_lu, hipcub::Max(), n_nodes, st));
        hipLaunchKernelGGL(proto_sizes, g(n_trees), dim3(256), 0, st, d_nodes, d_toff, n_trees, d_lp, d_lu, d_size, d_st);
        lap("sizes");
        hipLaunchKernelGGL(proto_roots, g(n_trees), dim3(256), 0, st, d_toff, n_trees, d_root);
        hipLaunchKernelGGL(proto_hdr, g(n_nodes), dim3(256), 0, st, d_slen, d_size, d_root, n_nodes, d_hdr);
        HIP_OK(hipGetLastError());
    }
    lap("hdr");
    // exclusive scan over n_nodes + 1 entries (the last is 0): pos[n_nodes] = total
    size_t tb3 = 0;
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb3, d_hdr, d_pos, n_nodes + 1, st));
    void* d_tmp = W.tmp3.get<uint8_t>(tb3);
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb3, d_hdr, d_pos, n_nodes + 1, st));
    uint64_t total = 0;
    HIP_OK(hipMemcpyAsync(&total, d_pos + n_nodes, 8, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(proto_tree_offsets, g(n_trees + 1ull), dim3(256), 0, st, d_toff, n_trees, d_pos, total, n_nodes,
                       d_to);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    // proto_tree_offsets ran before total was known on the device side: fix the tail entries
    HIP_OK(hipMemcpy(offsets, d_to, (n_trees + 1ull) * 8, hipMemcpyDeviceToHost));
    for (uint32_t t = 0; t <= n_trees; ++t)
        if (tree_off[t] >= n_nodes) offsets[t] = total;
    lap("scan");
    uint8_t* const buf = sink.at(total);
    if (!buf) return total;
    uint8_t* d_out = W.out.get<uint8_t>(total);
    hipLaunchKernelGGL(proto_write, g(n_nodes), dim3(256), 0, st, d_nodes, n_nodes, T, d_slen, d_size, d_root, d_pos,
                       d_out);
    HIP_OK(hipGetLastError());
    lap("write");
    d2h_staged(P, buf, d_out, total, st);
    lap("d2h");
    return total;
}

uint64_t device_tree_proto(Snapshot& S, const keto_tree_node* nodes, uint64_t n_nodes, const uint64_t* tree_off,
                           uint32_t n_trees, uint32_t ov_base, const std::vector<RowKey>& ov_keys, uint32_t extra_base,
                           const std::vector<std::string>& extra, uint8_t* buf, uint64_t cap, uint64_t* offsets) {
    return encode_proto(S, nodes, nullptr, n_nodes, tree_off, n_trees, ov_base, ov_keys, extra_base, extra,
                      Sink{buf, cap, nullptr}, offsets);
}

uint64_t device_tree_proto_resident(Snapshot& S, const ResidentArena& res, const uint64_t* tree_off, uint32_t n_trees,
                                    uint32_t ov_base, const std::vector<RowKey>& ov_keys, uint32_t extra_base,
                                    const std::vector<std::string>& extra, uint8_t** bytes_out, uint64_t* offsets) {
    return encode_proto(S, nullptr, &res, res.n_nodes, tree_off, n_trees, ov_base, ov_keys, extra_base, extra,
                      Sink{nullptr, 0, bytes_out}, offsets);
}

// Tree.MarshalJSON text of the same trees (the kernels above "json_"): nil[t] != 0 marks a nil tree
// ("null"); a tree without nodes that is not nil (an error root) is empty.
static uint64_t encode_json(Snapshot& S, const keto_tree_node* nodes, const ResidentArena* res, uint64_t n_nodes,
                          const uint64_t* tree_off, const uint8_t* nil, uint32_t n_trees, uint32_t ov_base,
                          const std::vector<RowKey>& ov_keys, uint32_t extra_base, const std::vector<std::string>& extra,
                          const Sink& sink, uint64_t* offsets) {
    const DevView dv = device_view(S);
    HIP_OK(hipSetDevice(dv.device));
    std::lock_guard<std::mutex> lk(S.mu);
    // KETO_JSON_TRACE=1: phase times on stderr (tooling)
    const bool trace = getenv("KETO_JSON_TRACE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!trace) return;
        (void)hipDeviceSynchronize();
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[json] %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
        t_last = t;
    };
    ProtoState& P = proto_state(S, dv.device);
    const hipStream_t st = 0;
    ProtoWork& W = P.work;
    const Arena A = upload_arena(S, P, nodes, n_nodes, tree_off, n_trees, ov_base, ov_keys, extra_base, extra, res);
    // run[t]: the "null" bytes of the node-less trees right before tree t, back to the last tree
    // with nodes (several such trees in a row share one node index: they need a term per tree)
    std::vector<uint64_t> run(n_trees + 1ull);
    json_null_runs(tree_off, nil, n_trees, run.data());
    uint64_t* d_run = W.jrun.get<uint64_t>(n_trees + 1ull);
    uint8_t* d_nil = W.jnil.get<uint8_t>(n_trees);
    HIP_OK(hipMemcpy(d_run, run.data(), (n_trees + 1ull) * 8, hipMemcpyHostToDevice));
    if (n_trees) HIP_OK(hipMemcpy(d_nil, nil, n_trees, hipMemcpyHostToDevice));
    lap(res ? "tables" : "upload");
    uint64_t* d_own = W.jown.get<uint64_t>(n_nodes);
    uint64_t* d_clen = W.jclen.get<uint64_t>(n_nodes);
    uint64_t* d_cat = W.jcat.get<uint64_t>(n_nodes + 1);
    int64_t* d_pre = W.jpre.get<int64_t>(n_nodes + 1);
    uint64_t* d_cend = W.jcend.get<uint64_t>(n_nodes);
    uint64_t* d_coff = W.jcoff.get<uint64_t>(n_nodes);
    uint64_t* d_term = W.jterm.get<uint64_t>(n_nodes + 2);
    uint64_t* d_pos = W.pos.get<uint64_t>(n_nodes + 2);
    uint64_t* d_st = W.st.get<uint64_t>(2 * n_nodes);
    int64_t* d_uni = W.uni.get<int64_t>(n_nodes);
    int64_t* d_lu = W.lu.get<int64_t>(n_nodes);
    uint64_t* d_to = W.to.get<uint64_t>(n_trees + 1ull);
    const auto g = [](uint64_t n) { return dim3((unsigned)std::max<uint64_t>(1, (n + 255) / 256)); };
    size_t tb_max = 0, tb_sum = 0;
    HIP_OK(hipcub::DeviceScan::InclusiveScan(nullptr, tb_max, d_uni, d_lu, hipcub::Max(), std::max<uint64_t>(1, n_nodes), st));
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_sum, d_term, d_pos, n_nodes + 2, st));
    void* d_tmp = W.tmp.get<uint8_t>(std::max(tb_max, tb_sum));
    HIP_OK(hipMemsetAsync(d_cat, 0, (n_nodes + 1) * 8, st));
    HIP_OK(hipMemsetAsync(d_pre, 0xFF, (n_nodes + 1) * 8, st));          // -1: not a root
    HIP_OK(hipMemsetAsync(d_term + n_nodes + 1, 0, 8, st));
    hipLaunchKernelGGL(json_roots, g(n_trees + 1ull), dim3(256), 0, st, A.toff, n_trees, d_run, n_nodes, d_pre);
    if (n_nodes) {
        hipLaunchKernelGGL(json_own, g(n_nodes), dim3(256), 0, st, A.nodes, n_nodes, A.T, d_own, d_clen, d_uni);
        HIP_OK(hipGetLastError());
        lap("sizes");
        HIP_OK(hipcub::DeviceScan::InclusiveScan(d_tmp, tb_max, d_uni, d_lu, hipcub::Max(), n_nodes, st));
        hipLaunchKernelGGL(json_closes, g(n_trees), dim3(256), 0, st, A.nodes, A.toff, n_trees, d_lu, d_clen, d_cat, d_cend,
                           d_coff, d_st);
        HIP_OK(hipGetLastError());
        lap("closes");
    }
    // exclusive scan over n_nodes + 2 entries (node n_nodes: what follows the last node; the last
    // is 0): pos[n_nodes + 1] = total
    hipLaunchKernelGGL(json_term, g(n_nodes + 1), dim3(256), 0, st, A.nodes, n_nodes, d_own, d_cat, d_pre, d_term);
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb_sum, d_term, d_pos, n_nodes + 2, st));
    hipLaunchKernelGGL(json_trees, g(n_trees + 1ull), dim3(256), 0, st, A.toff, n_trees, d_run, d_nil, d_cat, d_pos,
                       n_nodes, (uint8_t*)nullptr, d_to);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(offsets, d_to, (n_trees + 1ull) * 8, hipMemcpyDeviceToHost));
    const uint64_t total = offsets[n_trees];
    lap("scan");
    uint8_t* const buf = sink.at(total);
    if (!buf) return total;
    uint8_t* d_out = W.out.get<uint8_t>(total);
    if (n_nodes)
        hipLaunchKernelGGL(json_write, g(n_nodes), dim3(256), 0, st, A.nodes, n_nodes, A.T, d_cat, d_pre, d_cend, d_coff,
                           d_pos, d_out);
    hipLaunchKernelGGL(json_trees, g(n_trees + 1ull), dim3(256), 0, st, A.toff, n_trees, d_run, d_nil, d_cat, d_pos,
                       n_nodes, d_out, (uint64_t*)nullptr);
    HIP_OK(hipGetLastError());
    lap("write");
    d2h_staged(P, buf, d_out, total, st);
    lap("d2h");
    return total;
}

uint64_t device_tree_json(Snapshot& S, const keto_tree_node* nodes, uint64_t n_nodes, const uint64_t* tree_off,
                          const uint8_t* nil, uint32_t n_trees, uint32_t ov_base, const std::vector<RowKey>& ov_keys,
                          uint32_t extra_base, const std::vector<std::string>& extra, uint8_t* buf, uint64_t cap,
                          uint64_t* offsets) {
    return encode_json(S, nodes, nullptr, n_nodes, tree_off, nil, n_trees, ov_base, ov_keys, extra_base, extra,
                     Sink{buf, cap, nullptr}, offsets);
}

uint64_t device_tree_json_resident(Snapshot& S, const ResidentArena& res, const uint64_t* tree_off, const uint8_t* nil,
                                   uint32_t n_trees, uint32_t ov_base, const std::vector<RowKey>& ov_keys,
                                   uint32_t extra_base, const std::vector<std::string>& extra, uint8_t** bytes_out,
                                   uint64_t* offsets) {
    return encode_json(S, nullptr, &res, res.n_nodes, tree_off, nil, n_trees, ov_base, ov_keys, extra_base, extra,
                     Sink{nullptr, 0, bytes_out}, offsets);
}

// ---- keto_list_encode_batch: the ListRelationTuples response bodies of a batch of list queries, from
// the page's entries where list_emit left them (list.hip) and the tables above.  Paths relative to the
// reference tree: json.Marshal of GetResponse (internal/relationtuple/handler.go:23-29), whose tuples
// marshal as their RelationQuery (definitions.go:340-342,367-375: MarshalJSON is ToQuery(); :45-65: the
// field order, omitempty on the two subject fields), or proto.Marshal of ListRelationTuplesResponse
// (read_server.go:39-45,148-151; ToProto, definitions.go:231-250,358-365; acl.proto:14-52,
// read_service.proto:85-91).  An empty page is [] (persistence/sql/relationtuples.go:267), never null.
//
// The output is flat: query q owns the items [off_q + 2 q, off_q + 2 q + k_q + 2) -- a head frame, its
// k_q tuples (off_q = its window's offset into the entries), a tail frame -- and every item's bytes
// follow the item before it, so one exclusive scan of the item sizes places everything:
//   list_enc_sizes    a thread per item: its query by binary search over off_q + 2 q (strictly
//                     ascending, so empty queries need no care); nothing for a query that is not OK on the
//                     host's side or whose page holds a poisoned entry (the device flag: no host sync)
//   scan              hipcub exclusive sum, 64-bit, over n_items + 1 sizes
//   list_enc_offsets  a thread per query: body offset, tuples encoded, the poison flag -- one D2H
//   list_enc_write    a wave per 64 consecutive items.  Staged: when their bytes fit the wave's LDS
//                     window each lane assembles its item there, at the byte offset it has in the output
//                     (the window starts at the output's offset mod 16), and the wave streams the window
//                     out with 16-B stores between a byte-wise head and tail.  Direct: a lane per item
//                     straight to global memory, field by field in lockstep, so that a string longer
//                     than LE_COOP_MIN is written by the whole wave (list_wave_raw / list_wave_esc).
namespace {

constexpr uint32_t LE_THREADS = 256, LE_WAVES = LE_THREADS / 64;
constexpr uint32_t LE_WINDOW = 16384;        // bytes of LDS per wave
constexpr uint32_t LE_COOP_MIN = 256;        // the direct path: a longer string is the wave's work

struct LEnc {
    const uint2* slots;
    uint64_t n_slots;
    const uint64_t* wins;                    // per query {wlo, whi, off}
    const uint32_t* qpage;
    const uint64_t* meta;                    // per query: the next page's number, or LIST_ENC_FAILED
    uint32_t n;
    uint32_t json;
    uint64_t n_items;                        // n_slots + 2 n
};

constexpr uint32_t LE_NONE = 0, LE_TUPLE = 1, LE_HEAD = 2, LE_TAIL = 3;
struct LEItem {
    uint32_t kind;
    bool first;                              // a tuple: the first of its body
    uint2 e;
    uint64_t token;
};

__device__ inline LEItem list_enc_item(const LEnc& A, uint64_t i) {
    LEItem it{LE_NONE, false, make_uint2(0, 0), 0};
    if (i >= A.n_items || A.n == 0) return it;
    uint32_t lo = 0, hi = A.n;                             // base(lo) <= i; base(hi) > i or hi == n
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (A.wins[3ull * mid + 2] + 2ull * mid <= i) lo = mid;
        else hi = mid;
    }
    const uint64_t m = A.meta[lo];
    if (m == LIST_ENC_FAILED) return it;
    const uint64_t k = A.wins[3ull * lo + 1] - A.wins[3ull * lo], off = A.wins[3ull * lo + 2];
    if (k && A.qpage[lo]) return it;                       // toInternal fails over the page: no body
    const uint64_t local = i - (off + 2ull * lo);
    if (local == 0) {
        it.kind = LE_HEAD;
    } else if (local == k + 1) {
        it.kind = LE_TAIL;
        it.token = m;
    } else if (local <= k && off + local - 1 < A.n_slots) {
        it.kind = LE_TUPLE;
        it.first = local == 1;
        it.e = A.slots[off + local - 1];
    }
    return it;
}

__device__ inline uint32_t dec_digits(uint64_t v) {        // 0: the empty token
    uint32_t d = 0;
    while (v) {
        v /= 10;
        ++d;
    }
    return d;
}
__device__ inline uint8_t* put_dec(uint8_t* p, uint64_t v) {
    const uint32_t d = dec_digits(v);
    for (uint32_t k = d; k > 0; --k) {
        p[k - 1] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
    return p + d;
}

// the RelationTuple message without its own tag and length
__device__ inline uint64_t list_msg_len(const Sub& key, const Sub& sub) {
    uint64_t m = flen(subject_len(sub));
    for (int f = 0; f < 3; ++f) {
        const uint32_t l = slen_of(key.t[f], key.i[f]);
        if (l) m += flen(l);
    }
    return m;
}

__device__ inline uint64_t list_enc_size(const Tables& T, const LEItem& it, bool json) {
    if (it.kind == LE_NONE) return 0;
    if (it.kind == LE_HEAD) return json ? 20 : 0;          // {"relation_tuples":[
    if (it.kind == LE_TAIL) {
        const uint32_t d = dec_digits(it.token);
        return json ? 23 + d : (d ? flen(d) : 0);          // ],"next_page_token":"..."}
    }
    const Sub key = subject_of(T, EDGE_SET | it.e.x), sub = subject_of(T, it.e.y);
    if (json)
        return (it.first ? 0 : 1) + 13 + esc_len(key.t[0], key.i[0]) + 10 + esc_len(key.t[1], key.i[1]) + 12 +
               esc_len(key.t[2], key.i[2]) + subject_json_len(sub);
    return flen(list_msg_len(key, sub));
}

__global__ void __launch_bounds__(256) list_enc_sizes(LEnc A, Tables T, uint64_t* __restrict__ sz) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n_items) return;
    sz[i] = list_enc_size(T, list_enc_item(A, i), A.json != 0);
}

// res: [0, n] the body offsets, [n + 1, 2 n + 1) the tuples encoded, [2 n + 1, 3 n + 1) the poison flags
__global__ void __launch_bounds__(256) list_enc_offsets(LEnc A, const uint64_t* __restrict__ pos,
                                                        uint64_t* __restrict__ res) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > A.n) return;
    if (q == A.n) {
        res[q] = pos[A.n_items];
        return;
    }
    const uint64_t k = A.wins[3ull * q + 1] - A.wins[3ull * q], off = A.wins[3ull * q + 2];
    const uint32_t poisoned = k && A.qpage[q] ? 1u : 0u;
    res[q] = pos[off + 2ull * q];
    res[A.n + 1ull + q] = (A.meta[q] == LIST_ENC_FAILED || poisoned) ? 0 : k;
    res[2ull * A.n + 1 + q] = poisoned;
}

// one sequence of put_esc: the bytes esc_at's e stands for, at p
__device__ inline void put_seq(uint8_t* p, const uint8_t* s, uint32_t c, const Esc& e) {
    if (e.raw) {
        for (uint32_t k = 0; k < e.take; ++k) p[k] = s[c + k];
    } else if (e.emit == 2) {
        p[0] = '\\';
        p[1] = e.cp == '\n' ? 'n' : e.cp == '\r' ? 'r' : e.cp == '\t' ? 't' : (uint8_t)e.cp;
    } else {
        p[0] = '\\';
        p[1] = 'u';
        for (int k = 0; k < 4; ++k) {
            const uint32_t h = (e.cp >> (12 - 4 * k)) & 15u;
            p[2 + k] = (uint8_t)(h < 10 ? '0' + h : 'a' + (h - 10));
        }
    }
}

// The whole wave copies s[0, l) to p; returns the end.  Every lane calls it with the same arguments.
__device__ inline uint8_t* list_wave_raw(uint8_t* p, const uint8_t* s, uint32_t l, uint32_t lane) {
    for (uint32_t c = lane; c < l; c += 64) p[c] = s[c];
    return p + l;
}

// The whole wave writes put_esc's text of s[0, l), without the quotes, to p; returns the end.  A lane
// per byte, 64 bytes a step.  A byte starts a sequence of esc_at's walk unless it is a continuation
// byte that a valid multi-byte sequence in front of it consumes; such a sequence starts at a lead byte
// at most three bytes back with only continuation bytes between, and a lead byte -- never a
// continuation byte itself -- always starts a sequence.  So every lane can tell locally whether its
// byte starts one and what esc_at emits for it; a prefix sum over the wave places the sequences, and
// a run without escapes is a plain 64-byte copy.  Every lane calls it with the same arguments.
__device__ inline uint8_t* list_wave_esc(uint8_t* p, const uint8_t* s, uint32_t l, uint32_t lane) {
    for (uint32_t c0 = 0; c0 < l; c0 += 64) {
        const uint32_t i = c0 + lane;
        Esc e{0, 0, true, 0};
        if (i < l) {
            bool covered = false;
            if ((s[i] >> 6) == 2) {
                for (uint32_t k = 1; k <= 3 && k <= i; ++k) {
                    const uint8_t b = s[i - k];
                    if (b >= 0xC0) {
                        covered = esc_at(s, i - k, l).take > k;
                        break;
                    }
                    if ((b >> 6) != 2) break;
                }
            }
            if (!covered) e = esc_at(s, i, l);
        }
        uint32_t x = e.emit;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (e.emit) put_seq(p + (x - e.emit), s, i, e);
        p += __shfl(x, 63);
    }
    return p;
}

__device__ inline uint8_t* bcast_ptr(const uint8_t* p, int src) {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
    return (uint8_t*)(((uint64_t)hi << 32) | lo);
}

// One item's bytes at p.  COOP (the direct path): all 64 lanes of the wave are in the call, each with
// its own item (or none), and walk the six string fields of a tuple in lockstep -- row namespace,
// object, relation, then the subject's one or three -- each lane writing the literal in front of its
// field and the field itself when it is short, the wave together every field longer than LE_COOP_MIN.
template <bool COOP>
__device__ __forceinline__ void list_enc_put(const Tables& T, const LEItem& it, bool json, uint8_t* p, uint32_t lane) {
    if (it.kind == LE_HEAD) {
        if (json) PUT_LIT(p, "{\"relation_tuples\":[");
    } else if (it.kind == LE_TAIL) {
        if (json) {
            p = PUT_LIT(p, "],\"next_page_token\":\"");
            p = put_dec(p, it.token);
            PUT_LIT(p, "\"}");
        } else if (it.token) {
            *p++ = 0x12;
            *p++ = (uint8_t)dec_digits(it.token);           // at most 20 digits: one length byte
            put_dec(p, it.token);
        }
    }
    const bool tup = it.kind == LE_TUPLE;
    Sub key, sub;
    key.set = sub.set = false;
    if (tup) {
        key = subject_of(T, EDGE_SET | it.e.x);
        sub = subject_of(T, it.e.y);
        if (!json) {
            *p++ = 0x0A;
            p = put_varint(p, list_msg_len(key, sub));
        } else if (!it.first) {
            *p++ = ',';
        }
    }
    const uint8_t tags[3] = {0x0A, 0x12, 0x1A};
#pragma unroll 1
    for (int f = 0; f < 6; ++f) {
        const StrTab* t = nullptr;
        uint32_t si = NONE_STR, l = 0;
        bool has = false;                                   // a string is written at this step
        if (tup && (f < 4 || sub.set)) {
            const Sub& from = f < 3 ? key : sub;
            t = from.t[f % 3];
            si = from.i[f % 3];
            l = slen_of(t, si);
            if (json) {
                has = true;
                switch (f) {
                    case 0: p = PUT_LIT(p, "{\"namespace\":"); break;
                    case 1: p = PUT_LIT(p, ",\"object\":"); break;
                    case 2: p = PUT_LIT(p, ",\"relation\":"); break;
                    case 3:
                        p = sub.set ? PUT_LIT(p, ",\"subject_set\":{\"namespace\":") : PUT_LIT(p, ",\"subject_id\":");
                        break;
                    case 4: p = PUT_LIT(p, ",\"object\":"); break;
                    default: p = PUT_LIT(p, ",\"relation\":"); break;
                }
            } else {
                if (f == 3) {
                    *p++ = 0x22;
                    p = put_varint(p, subject_len(sub));
                    if (sub.set) {
                        uint64_t in = 0;
                        for (int g = 0; g < 3; ++g) {
                            const uint32_t gl = slen_of(sub.t[g], sub.i[g]);
                            if (gl) in += flen(gl);
                        }
                        *p++ = 0x12;
                        p = put_varint(p, in);
                    }
                }
                has = l != 0 || (f == 3 && !sub.set);       // empty strings are omitted, but for the id
            }
        }
        const bool coop = COOP && has && l > LE_COOP_MIN;
        if (has && !coop) p = json ? put_esc(p, t, si) : put_str(p, tags[f % 3], t, si);
        if constexpr (COOP) {
            const uint8_t* s = nullptr;
            if (coop) {
                s = t->bytes + t->off[si];
                if (json) {
                    *p++ = '"';
                } else {
                    *p++ = tags[f % 3];
                    p = put_varint(p, l);
                }
            }
            uint64_t mask = __ballot(coop);
            while (mask) {
                const int src = __ffsll((unsigned long long)mask) - 1;
                mask &= mask - 1;
                const uint8_t* cs = bcast_ptr(s, src);
                uint8_t* cp = bcast_ptr(p, src);
                const uint32_t cl = __shfl(l, src);
                uint8_t* end = json ? list_wave_esc(cp, cs, cl, lane) : list_wave_raw(cp, cs, cl, lane);
                if ((int)lane == src) p = end;
            }
            if (coop && json) *p++ = '"';
        }
    }
    if (tup && json) {
        if (sub.set) *p++ = '}';
        *p++ = '}';
    }
}

__global__ void __launch_bounds__(LE_THREADS)
list_enc_write(LEnc A, Tables T, const uint64_t* __restrict__ pos, uint8_t* __restrict__ out, uint32_t use_lds) {
    // LE_WAVES windows when use_lds, nothing otherwise (the direct path's occupancy is not bound by LDS)
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t i0 = ((uint64_t)blockIdx.x * LE_WAVES + wave) * 64, i = i0 + lane;
    const bool json = A.json != 0;
    const bool live = i0 < A.n_items;                       // the same for the whole wave
    uint64_t b0 = 0, b1 = 0;
    if (live) {
        b0 = pos[i0];
        b1 = pos[min(i0 + 64, A.n_items)];
    }
    const uint32_t a = (uint32_t)(b0 & 15u);                // the window starts at the output's offset mod 16
    const bool staged = live && use_lds && b1 > b0 && a + (b1 - b0) <= LE_WINDOW;
    const LEItem it = live ? list_enc_item(A, i) : LEItem{LE_NONE, false, make_uint2(0, 0), 0};
    uint8_t* const w = lds + wave * LE_WINDOW;
    if (staged) {
        if (it.kind != LE_NONE) list_enc_put<false>(T, it, json, w + a + (uint32_t)(pos[i] - b0), lane);
    } else if (live && b1 > b0) {
        list_enc_put<true>(T, it, json, out + (it.kind != LE_NONE ? pos[i] : b0), lane);
    }
    __syncthreads();
    if (staged) {
        const uint32_t len = (uint32_t)(b1 - b0);
        uint8_t* const g = out + b0;
        const uint32_t head = min(len, (16u - a) & 15u), nvec = (len - head) / 16, tail = head + nvec * 16;
        if (lane < head) g[lane] = w[a + lane];
        for (uint32_t v = lane; v < nvec; v += 64)
            *reinterpret_cast<uint4*>(g + head + 16 * v) = *reinterpret_cast<const uint4*>(w + a + head + 16 * v);
        if (tail + lane < len) g[tail + lane] = w[a + tail + lane];
    }
}

struct ListEncEvents {
    hipEvent_t a = nullptr, b = nullptr;
    ListEncEvents() {
        HIP_OK(hipEventCreate(&a));
        if (hipEventCreate(&b) != hipSuccess) {
            (void)hipEventDestroy(a);
            throw Error{KETO_E_HIP, "hipEventCreate"};
        }
    }
    ~ListEncEvents() {
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
    }
};

}  // namespace

void device_list_encode(Snapshot& S, const ListEncodeIn& in, uint32_t encoding, ListEncoded& out,
                        std::vector<uint32_t>& qpage) {
    const DevView dv = device_view(S);
    HIP_OK(hipSetDevice(dv.device));
    const hipStream_t st = static_cast<hipStream_t>(in.stream);
    const uint32_t n = in.n;
    const uint64_t n_items = in.n_slots + 2ull * n;
    if (n_items >= (1ull << 31)) throw Error{KETO_E_RANGE, "keto_list_encode_batch: more than 2^31 tuples in one call"};
    // KETO_LIST_ENC_LDS=0: every wave writes straight to global memory (tests, the A/B of the two paths)
    const char* env = getenv("KETO_LIST_ENC_LDS");
    const uint32_t use_lds = env ? (atol(env) != 0 ? 1u : 0u) : 1u;
    ListEncEvents ev;
    std::lock_guard<std::mutex> lk(S.mu);
    const bool current = S.proto && S.proto->version == S.version;
    ProtoState& P = proto_state(S, dv.device);
    if (!current) {
        // the refresh copied on the null stream: the list stream, which does not synchronize with it,
        // waits for it explicitly
        if (!P.list_ev) HIP_OK(hipEventCreateWithFlags(&P.list_ev, hipEventDisableTiming));
        HIP_OK(hipEventRecord(P.list_ev, 0));
        HIP_OK(hipStreamWaitEvent(st, P.list_ev, 0));
    }
    ListEncWork& W = P.list_work;
    const Tables T{P.strs.view(), P.ns.view(), StrTab{nullptr, nullptr, 0}, P.row_ns, P.row_obj, P.row_rel, P.n_rows,
                   nullptr, nullptr, nullptr, 0, 0, 0};
    uint64_t* d_meta = W.meta.get<uint64_t>(n);
    uint64_t* d_sz = W.sz.get<uint64_t>(n_items + 1);
    uint64_t* d_pos = W.pos.get<uint64_t>(n_items + 1);
    uint64_t* d_res = W.res.get<uint64_t>(3ull * n + 1);
    size_t tb = 0;
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_sz, d_pos, n_items + 1, st));
    void* d_tmp = W.tmp.get<uint8_t>(tb);
    const LEnc A{static_cast<const uint2*>(in.d_slots), in.n_slots, in.d_wins, in.d_qpage, d_meta, n,
                 encoding == KETO_ENC_JSON ? 1u : 0u, n_items};
    const auto g = [](uint64_t k) { return dim3((unsigned)std::max<uint64_t>(1, (k + 255) / 256)); };
    HIP_OK(hipEventRecord(ev.a, st));
    HIP_OK(hipMemcpyAsync(d_meta, in.meta, (uint64_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_sz + n_items, 0, 8, st));
    hipLaunchKernelGGL(list_enc_sizes, g(n_items), dim3(256), 0, st, A, T, d_sz);
    HIP_OK(hipGetLastError());
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_sz, d_pos, n_items + 1, st));
    hipLaunchKernelGGL(list_enc_offsets, g(n + 1ull), dim3(256), 0, st, A, d_pos, d_res);
    HIP_OK(hipGetLastError());
    // ---- the one host sync before the write: offsets, tuple counts, poison flags, and with them the total
    std::vector<uint64_t> res(3ull * n + 1);
    HIP_OK(hipMemcpyAsync(res.data(), d_res, res.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    out.offsets.assign(res.begin(), res.begin() + n + 1);
    out.tuples.assign(res.begin() + n + 1, res.begin() + 2ull * n + 1);
    qpage.resize(n);
    for (uint32_t q = 0; q < n; ++q) qpage[q] = (uint32_t)res[2ull * n + 1 + q];
    const uint64_t total = res[n];
    if (total) {
        out.bytes = static_cast<uint8_t*>(pinned_take(total));   // the caller's from here on
        out.total = total;
        uint8_t* d_out = W.out.get<uint8_t>(total + 16);
        const uint64_t waves = (n_items + 63) / 64;
        hipLaunchKernelGGL(list_enc_write, dim3((unsigned)((waves + LE_WAVES - 1) / LE_WAVES)), dim3(LE_THREADS),
                           use_lds ? LE_WAVES * LE_WINDOW : 0, st, A, T, d_pos, d_out, use_lds);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(out.bytes, d_out, total, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipEventRecord(ev.b, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipEventElapsedTime(&out.encode_ms, ev.a, ev.b));
}

}  // namespace keto
