// ThreadSanitizer run of keto_snapshot_delete_query's locking (tests/test_delete_query_tsan.py builds
// this with the library's host code under -fsanitize=thread; no GPU is touched).  On one host-only
// snapshot, at once:
//   * planners call keto_list_plan: the snapshot's lock shared, then the list index's mutex (the host
//     half of the index is built by whichever caller finds it stale);
//   * a writer alternates keto_snapshot_delete_query -- the scan under the shared lock and the index
//     mutex, the mutex released before the commit waits for the exclusive lock, the host half rebuilt
//     under the exclusive lock with the mutex taken again -- and keto_snapshot_apply.
// The run has to finish (a lock-order inversion between the snapshot's lock and the index mutex would
// leave a planner and the writer waiting for each other) and TSan has to stay silent.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <thread>
#include <vector>

#include "../../include/keto_mi355x.h"

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() {
        uint64_t x = (s += 0x9E3779B97F4A7C15ull);
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        return x ^ (x >> 31);
    }
    uint32_t pick(uint32_t n) { return (uint32_t)(next() % n); }
};

keto_str ks(const std::string& s) { return keto_str{s.data(), (uint32_t)s.size()}; }

std::atomic<int> failures{0};

void fail(const char* what, int rc) {
    std::fprintf(stderr, "FAIL %s: rc %d: %s\n", what, rc, keto_last_error());
    failures.fetch_add(1);
}

const char* NS[] = {"docs", "groups"};
const char* RELS[] = {"view", "member"};
constexpr uint32_t N_OBJ = 200, N_USER = 50;

struct Maker {
    std::deque<std::string> pool;      // stable storage behind the keto_str views
    keto_str keep(std::string s) {
        pool.push_back(std::move(s));
        return ks(pool.back());
    }
    keto_tuple tuple(Rng& r) {
        keto_tuple t;
        std::memset(&t, 0, sizeof t);
        const uint32_t ns = r.pick(2);
        t.namespace_id = (int32_t)ns + 1;
        t.object = keep("o" + std::to_string(r.pick(N_OBJ)));
        t.relation = keep(RELS[ns]);
        if (r.pick(4)) {
            t.subject_kind = 0;
            t.subject_id = keep("u" + std::to_string(r.pick(N_USER)));
        } else {
            t.subject_kind = 1;
            t.set_namespace_id = 2;
            t.set_object = keep("o" + std::to_string(r.pick(N_OBJ)));
            t.set_relation = keep(RELS[1]);
        }
        return t;
    }
    // a query of a random shape: any of namespace / object / relation, with or without a subject id
    keto_list_req query(Rng& r) {
        keto_list_req q;
        std::memset(&q, 0, sizeof q);
        const uint32_t ns = r.pick(2), shape = r.pick(8);
        if (shape & 1) q.namespace_ = keep(NS[ns]);
        if (shape & 2) q.object = keep("o" + std::to_string(r.pick(N_OBJ)));
        if (shape & 4) q.relation = keep(RELS[ns]);
        if (r.pick(3) || shape == 0) {       // the empty query would delete everything at once
            q.has_subject = 1;
            q.subject.kind = 0;
            q.subject.id = keep("u" + std::to_string(r.pick(N_USER)));
        }
        return q;
    }
};

}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 200;
    std::vector<keto_namespace> ns;
    std::deque<std::string> names;
    for (int i = 0; i < 2; ++i) {
        names.push_back(NS[i]);
        ns.push_back(keto_namespace{i + 1, ks(names.back())});
    }
    Maker base_maker;
    Rng r0{1};
    std::vector<keto_tuple> base;
    for (int i = 0; i < 6000; ++i) base.push_back(base_maker.tuple(r0));
    keto_snapshot_opts opts{};
    opts.page_size = 7;
    opts.device = -1;
    keto_snapshot* snap = nullptr;
    int rc = keto_snapshot_build(ns.data(), (uint32_t)ns.size(), base.data(), base.size(), &opts, &snap);
    if (rc != KETO_OK) {
        fail("build", rc);
        return 1;
    }
    std::atomic<bool> done{false};
    std::atomic<uint64_t> plans{0}, deleted{0};

    std::thread writer([&] {
        Maker m;
        Rng r{7};
        uint64_t version = 0;
        for (int it = 0; it < rounds; ++it) {
            const keto_list_req q = m.query(r);
            keto_delete_info info{};
            int rc = keto_snapshot_delete_query(snap, &q, &info);
            if (rc != KETO_OK) fail("delete_query", rc);
            else if (info.version != ++version || info.path != KETO_DELETE_PATH_HOST || info.index_kept)
                fail("delete_query info", (int)info.version);
            deleted.fetch_add(info.deleted);
            std::vector<keto_tuple> ins;
            for (uint32_t k = 1 + r.pick(8); k > 0; --k) ins.push_back(m.tuple(r));
            uint64_t ver = 0;
            rc = keto_snapshot_apply(snap, ins.data(), ins.size(), nullptr, 0, &ver);
            if (rc != KETO_OK || ver != ++version) fail("apply", rc);
        }
        done = true;
    });

    std::vector<std::thread> planners;
    for (int t = 0; t < 4; ++t)
        planners.emplace_back([&, t] {
            Maker m;
            Rng r{100u + (uint64_t)t};
            while (!done.load()) {
                m.pool.clear();
                std::vector<keto_list_req> q(16);
                for (auto& x : q) x = m.query(r);
                std::vector<keto_list_plan_t> p(q.size());
                const int rc = keto_list_plan(snap, q.data(), (uint32_t)q.size(), p.data());
                if (rc != KETO_OK) fail("list_plan", rc);
                for (const auto& x : p)
                    if (x.status != KETO_LIST_OK || x.hi < x.lo) fail("list_plan answer", x.status);
                plans.fetch_add(1);
            }
        });

    writer.join();
    for (auto& t : planners) t.join();
    keto_snapshot_release(snap);
    if (failures.load()) return 1;
    std::printf("tsan delete rounds ok: %d deletes, %llu tuples deleted, %llu plans\n", rounds,
                (unsigned long long)deleted.load(), (unsigned long long)plans.load());
    return 0;
}
