// The erasure form of a transaction (delta.cpp): what keto_snapshot_delete_query commits.
#pragma once

#include <functional>

#include "snapshot.hpp"

namespace keto {

// every edge equal to `subject` leaves `row`; subject == ANY: every tuple of the row
struct RowErase {
    uint32_t row, subject;
};

// apply_writes with a third input: row-level erasures, staged after the tuple deletes; the collision,
// wildcard, poison and commit stages then run as for any transaction (apply_writes passes none)
void apply_writes_erase(Snapshot& s, const keto_tuple* ins, uint64_t n_ins, const keto_tuple* del, uint64_t n_del,
                        const RowErase* erase, uint64_t n_erase, const std::function<void()>& commit = {});

}  // namespace keto
