// ListRelationTuples from the snapshot (list.hip; keto_list_batch / keto_list_plan): what the C-ABI
// layer needs of it.  The list index lives with the snapshot's handle (capi_internal.hpp), not in
// keto::Snapshot: it is built on the first list call of a snapshot version and freed with the handle,
// before the snapshot's device state.
#pragma once

#include <memory>
#include <mutex>
#include <vector>

#include "snapshot.hpp"

namespace keto {

struct ListState;        // list.hip
struct ListStateDeleter {
    void operator()(ListState* l) const;
};
struct ListCache {
    std::unique_ptr<ListState, ListStateDeleter> state;
    std::mutex mu;       // builds the index; held for the whole of a list_batch (one at a time per snapshot)
};

struct ListResult {
    std::vector<uint8_t> status;                        // n x KETO_LIST_*
    std::vector<uint64_t> offsets, next_page, totals;   // n + 1, n, n
    keto_list_tuple* tuples = nullptr;                  // a block of the pinned pool (pinned_take), or NULL
    float index_ms = 0, scan_ms = 0;
};

// The callers hold the snapshot's lock shared.  list_plan resolves the queries on the host (any
// snapshot); list_batch runs them on the snapshot's device and hands out.tuples to the caller, who
// gives it back with pinned_give.
void list_plan(const Snapshot& s, ListCache& c, const keto_list_req* reqs, uint32_t n, keto_list_plan_t* out);
void list_batch(Snapshot& s, ListCache& c, const keto_list_req* reqs, uint32_t n, ListResult& out);
uint64_t list_device_bytes(ListCache& c);   // device memory of the list index (0 before the first list_batch)

// keto_list_encode_batch (list.hip, proto.hip): the response bodies of the same queries, encoded on the
// device from the page's entries where list_emit left them
struct ListEncoded {
    ListResult r;                                       // status, next_page, totals, timings; r.offsets / r.tuples unused
    std::vector<uint64_t> offsets, tuples;              // n + 1 byte offsets; n: tuples encoded into body i
    uint8_t* bytes = nullptr;                           // a block of the pinned pool (pinned_take), or NULL (total 0)
    uint64_t total = 0;
    float encode_ms = 0;
};
// The caller holds the snapshot's lock shared.  Takes c.mu, and S.mu inside it (the encoder); out.bytes
// goes to the caller, who gives it back with pinned_give -- also when the call throws.
void list_encode_batch(Snapshot& s, ListCache& c, const keto_list_req* reqs, uint32_t n, uint32_t encoding,
                       ListEncoded& out);
// What list.hip hands the encoder in proto.hip: the page's entries {row id, subject word} of all queries
// (d_slots, n_slots of them) and per query its window {wlo, whi, off} (three words: entries
// d_slots[off, off + whi - wlo)), its poison-in-page flag -- all on the device, their writes enqueued on
// `stream` -- and on the host meta[q] = the next page's number (0: none), or LIST_ENC_FAILED for a query
// that is not KETO_LIST_OK whatever its page holds.
constexpr uint64_t LIST_ENC_FAILED = ~0ull;
struct ListEncodeIn {
    const void* d_slots;
    uint64_t n_slots;
    const uint64_t* d_wins;
    const uint32_t* d_qpage;
    const uint64_t* meta;
    uint32_t n;
    void* stream;
};
// Runs on in.stream, under S.mu, after the refresh of the snapshot's strings on the device; returns with
// the stream drained.  Fills out.offsets / tuples / bytes / total / encode_ms and qpage (the flags, on the host).
void device_list_encode(Snapshot& s, const ListEncodeIn& in, uint32_t encoding, ListEncoded& out,
                        std::vector<uint32_t>& qpage);

// keto_lookup_objects_batch (list.hip): per query the tuple rows (namespace, o, relation), in key
// order, whose check against the query's subject is allowed; the page of them
struct LookupResult {
    std::vector<uint8_t> status;                        // n x KETO_LOOKUP_*
    std::vector<uint64_t> offsets, next_page, totals;   // n + 1, n, n
    std::vector<uint64_t> candidates, undecided;        // n, n
    uint32_t* rows = nullptr;                           // a block of the pinned pool (pinned_take), or NULL
    float index_ms = 0, candidates_ms = 0, check_ms = 0, emit_ms = 0;
};
// The caller holds the snapshot's lock shared, from before the call until it returns: the candidates,
// their checks and the page belong to one version.  Holds c.mu throughout, and the device lock
// (device_check_rows) inside it per chunk.  out.rows goes to the caller, who gives it back with pinned_give.
void lookup_objects(Snapshot& s, ListCache& c, const keto_lookup_req* reqs, uint32_t n, int32_t global_max_depth,
                    LookupResult& out);

// The journal of written rows.  keto_snapshot_apply, holding the snapshot's lock exclusive, after the
// commit that took the version from ver_before to ver_after: notes the rows it changed.  Nothing is
// noted without index state; past KETO_LIST_PATCH_MAX_ROWS distinct rows, with KETO_LIST_PATCH=0, or when
// a version went by unnoted the journal is invalid and the next list call rebuilds the index.
void list_note_rows(ListCache& c, const uint32_t* rows, uint64_t n, uint64_t ver_before, uint64_t ver_after) noexcept;
// keto_list_index_info: the caller holds the snapshot's lock shared; builds nothing
void list_index_info(const Snapshot& s, ListCache& c, keto_list_index_info_t* out);

// keto_snapshot_delete_query: the rows a whereQuery / whereSubject touches (list.hip)
struct DeleteScan {
    std::vector<uint32_t> rows;      // the tuple rows that lose a tuple, ascending and distinct
    uint32_t subject = ANY;          // the subject word that leaves them (ANY: every tuple of the row)
    uint64_t matches = 0;            // tuples matched (SQL: rows affected)
    uint64_t heads = 0;              // rows touched; rows is left empty when there are more than max_rows
    bool poisoned = false;           // a poisoned tuple among the tuples matching the key part
    uint32_t path = KETO_DELETE_PATH_HOST;
    float scan_ms = 0;
    // the query as the scan ran it on the list index of `version`: entries [lo, hi) and the key
    // predicates left over -- what delete_index_patch squeezes the matches out of
    uint64_t lo = 0, hi = 0, version = 0;
    uint32_t obj = ANY, rel = ANY;
};
// The caller holds the snapshot's lock shared (and not c.mu, which the scan takes and releases).  Throws
// KETO_E_INVALID for an unknown namespace.  The device pass runs when the snapshot is on a device,
// unpartitioned, its device list index is current and the query is not fully keyed; no index is built.
void delete_scan(const Snapshot& s, ListCache& c, const keto_list_req& q, uint64_t max_rows, DeleteScan& out);
// After the commit, the caller holding the snapshot's lock exclusive: patches the device list index
// that was current at scan.version (out of place: [0, lo), the kept entries of [lo, hi), [hi, N)) and
// rebuilds the host half, both stamped with the new version.  Returns true when the device index is
// current afterwards; any failure drops the index (the next list call rebuilds it) and returns false.
// Without a device index to keep, the host half is only marked stale (the next list call rebuilds it
// under the shared lock).
bool delete_index_patch(const Snapshot& s, ListCache& c, const DeleteScan& scan) noexcept;

}  // namespace keto
