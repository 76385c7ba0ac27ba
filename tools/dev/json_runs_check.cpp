// Stand-alone check of json_null_runs (keto_amd/csrc/json_runs.hpp), the host side of
// keto_tree_json_all_device's per-tree offsets, for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan \
//       -static-libubsan -I keto_amd/csrc tools/dev/json_runs_check.cpp -o json_runs_check && ./json_runs_check
// Random batches (trees with nodes, nil trees, error roots; runs of node-less trees at the start, in
// the middle and at the end; n = 0) against the definition applied tree by tree, and the offsets a
// layout built from run[] gives against a concatenation of the per-tree texts' lengths.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "json_runs.hpp"

int main() {
    std::mt19937_64 rng(12345);
    uint64_t cases = 0;
    for (uint32_t n = 0; n <= 70; ++n) {
        for (int rep = 0; rep < 40; ++rep) {
            // kind: 0 = a tree with nodes, 1 = nil, 2 = error root
            std::vector<int> kind(n);
            const int mode = rep % 4;                     // 3: no tree has nodes
            for (uint32_t t = 0; t < n; ++t) {
                const uint64_t r = rng() % 10;
                kind[t] = mode == 3 ? 1 + (int)(r & 1) : r < (mode == 0 ? 7u : 3u) ? 0 : 1 + (int)(r & 1);
            }
            std::vector<uint64_t> toff(n + 1, 0), len(n, 0);
            std::vector<uint8_t> nil(n, 0);
            for (uint32_t t = 0; t < n; ++t) {
                const uint64_t nodes = kind[t] == 0 ? 1 + rng() % 5 : 0;
                toff[t + 1] = toff[t] + nodes;
                nil[t] = kind[t] == 1;
                len[t] = kind[t] == 0 ? 30 * nodes : kind[t] == 1 ? 4 : 0;   // bytes of tree t's text
            }
            std::vector<uint64_t> run(n + 1, ~0ull);
            keto::json_null_runs(toff.data(), nil.data(), n, run.data());
            // the definition: "null" bytes of the node-less trees between the last tree with nodes
            // before t and t
            for (uint32_t t = 0; t <= n; ++t) {
                uint64_t want = 0;
                for (uint32_t u = t; u-- > 0 && toff[u] == toff[u + 1];) want += nil[u] ? 4 : 0;
                if (run[t] != want) {
                    fprintf(stderr, "n=%u rep=%d t=%u: run %llu, want %llu\n", n, rep, t, (unsigned long long)run[t],
                            (unsigned long long)want);
                    return 1;
                }
            }
            // the layout: a tree's text starts behind the text of the trees with nodes before it
            // (what the device's scan over nodes gives) plus every "null" before it; with run[]
            // that is start(next node) - (the run's bytes from t on) for a node-less tree
            std::vector<uint64_t> want_off(n + 1, 0);
            for (uint32_t t = 0; t < n; ++t) want_off[t + 1] = want_off[t] + len[t];
            uint64_t node_bytes = 0, nulls_done = 0;      // bytes of finished trees with nodes / runs
            for (uint32_t t = 0; t <= n; ++t) {
                const uint64_t at = node_bytes + nulls_done + run[t];
                if (at != want_off[t]) {
                    fprintf(stderr, "n=%u rep=%d t=%u: offset %llu, want %llu\n", n, rep, t, (unsigned long long)at,
                            (unsigned long long)want_off[t]);
                    return 1;
                }
                if (t < n && toff[t] < toff[t + 1]) {
                    node_bytes += len[t];
                    nulls_done += run[t];
                }
            }
            ++cases;
        }
    }
    printf("json_runs_check: %llu batches ok\n", (unsigned long long)cases);
    return 0;
}
