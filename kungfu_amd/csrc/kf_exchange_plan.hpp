// kf_exchange_plan.hpp — the arithmetic of the exchange's batch schedule (kf_exchange.hip):
// where a call's received shards and tails lie in the workspace, and how the pipelined
// all-reduce cuts its buckets into groups. Plain C++17, no HIP: tests/c/test_exchange_plan.cpp.
#pragma once
#include <cstddef>
#include <vector>

namespace kf
{
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The workspace of one call over `world` ranks, in bucket order: per bucket of q * world + t
// elements, the world received shards of q elements (all-to-all only), then the world gathered
// tails of t elements, each region at the next 256-byte step. No region: offset 0.
struct Workspace {
    std::vector<size_t> shards, tails;  // byte offsets, one per bucket
    size_t bytes = 0;
};
inline Workspace plan_workspace(const size_t *counts, int nb, size_t world, size_t elem_size,
                                bool all_to_all)
{
    Workspace w{std::vector<size_t>(nb, 0), std::vector<size_t>(nb, 0)};
    auto take = [&](size_t &off, size_t elems) {
        off = w.bytes;
        w.bytes += align_up(elems * world * elem_size, 256);
    };
    for (int b = 0; b < nb; ++b) {
        if (all_to_all && counts[b] / world) take(w.shards[b], counts[b] / world);
        if (counts[b] % world) take(w.tails[b], counts[b] % world);
    }
    return w;
}

// The pipeline's groups: nb buckets in at most min(G, nb) groups of consecutive buckets with about
// equal element counts; group g is [cut[g], cut[g + 1]). A group closes at the first bucket that
// brings the running count to its share, while every later group can still get a bucket.
inline std::vector<int> split_groups(const size_t *counts, int nb, int G)
{
    std::vector<int> cut(1, 0);
    if (nb <= 0) return cut;
    G = G < nb ? G : nb;
    size_t total = 0, acc = 0;
    for (int b = 0; b < nb; ++b) total += counts[b];
    for (int b = 0; b < nb; ++b) {
        acc += counts[b];
        const int left = nb - b - 1, want = G - static_cast<int>(cut.size());
        if (want > 0 && left >= want && acc * G >= total * cut.size()) cut.push_back(b + 1);
    }
    cut.push_back(nb);
    return cut;
}
}  // namespace kf
