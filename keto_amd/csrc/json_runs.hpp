// Host side of keto_tree_json_all_device's per-tree term (proto.hip): trees without nodes (nil
// trees, which encode as "null", and error roots, which encode as nothing) have no node to hang
// their bytes on, and several in a row share one node index.
#pragma once
#include <cstdint>

namespace keto {

// run[t], t <= n_trees: the "null" bytes of the node-less trees between the last tree with nodes
// before tree t and tree t itself (t = n_trees: behind the last tree).  tree_off[n_trees + 1]: tree
// t's nodes are [tree_off[t], tree_off[t + 1]); nil[t] != 0: tree t is a nil tree.
inline void json_null_runs(const uint64_t* tree_off, const uint8_t* nil, uint32_t n_trees, uint64_t* run) {
    uint64_t acc = 0;
    for (uint32_t t = 0; t < n_trees; ++t) {
        run[t] = acc;
        if (tree_off[t] < tree_off[t + 1]) acc = 0;
        else if (nil[t]) acc += 4;
    }
    run[n_trees] = acc;
}

}  // namespace keto
