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

}  // namespace keto
