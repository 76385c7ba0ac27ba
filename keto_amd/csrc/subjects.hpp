// keto_subjects_batch (subjects.hip): the distinct SubjectID leaves of expand trees, flattened on the
// device from the node arena device_expand leaves there.  What the C-ABI layer needs of it.  The
// workspace and its stream live with the snapshot's handle (capi_internal.hpp), next to the list
// index, and are freed with the handle, before the snapshot's device state.
#pragma once

#include <memory>
#include <mutex>
#include <vector>

#include "snapshot.hpp"

namespace keto {

struct SubjectsState;    // subjects.hip
struct SubjectsStateDeleter {
    void operator()(SubjectsState* s) const;
};
struct SubjectsCache {
    std::unique_ptr<SubjectsState, SubjectsStateDeleter> state;
    std::mutex mu;       // the workspace: held from the first pass over the arena to the page's copy
};

constexpr uint32_t SUBJECTS_STAGES = 5;   // compact, wave class, block class, global class, emit

struct SubjectsResult {
    std::vector<uint8_t> status;                        // n x KETO_SUBJECTS_*
    std::vector<uint64_t> offsets, next_page, totals;   // n + 1, n, n
    std::vector<uint64_t> leaves, set_leaves;           // n, n
    uint32_t* ids = nullptr;                            // a block of the pinned pool (pinned_take), or NULL
    float expand_ms = 0, flatten_ms = 0;
    float stage_ms[SUBJECTS_STAGES] = {0, 0, 0, 0, 0};
};

// The segment length up to which a segment is sorted in LDS: KETO_SUBJECTS_LDS from the environment
// (default 2048; a power of two in [128, 8192], anything else is KETO_E_INVALID).
uint32_t subjects_lds_limit();

// The caller holds the snapshot's lock shared and, in keep.hold, the device state's mutex over the
// arena keep.arena describes (device_expand's `keep` form); ex = that expand's statuses and offsets.
// Lock order: rw shared -> D.mu (keep.hold) -> c.mu.  keep.hold is dropped as soon as the passes that
// read the arena have completed; c.mu is held to the end.  page_size / page: n entries each (0 = the
// snapshot's page size / the first page).  out.ids goes to the caller, who gives it back with pinned_give.
void subjects_flatten(Snapshot& s, SubjectsCache& c, ExpandOnDevice& keep, const ExpandResult& ex,
                      const uint32_t* page_size, const uint32_t* page, uint32_t n, SubjectsResult& out);

}  // namespace keto
