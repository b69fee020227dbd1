// The arithmetic of the exchange's batch schedule
// (kungfu_amd/csrc/kf_exchange_plan.hpp), driven without HIP:
//
//   test_exchange_plan WORLD ELEM_SIZE ALL_TO_ALL G [COUNT ...]
//
// prints "ws BYTES | the shard offsets | the tail offsets" (plan_workspace)
// and "groups" followed by the cuts (split_groups). No memory but the plans'
// own is touched: the counts are plain numbers. tests/test_exchange_plan.py
// builds this with -fsanitize=address,undefined and checks the output.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kf_exchange_plan.hpp"

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const size_t world = std::strtoull(argv[1], nullptr, 0), sz = std::strtoull(argv[2], nullptr, 0);
    const bool a2a = std::atoi(argv[3]) != 0;
    const int G    = std::atoi(argv[4]);
    std::vector<size_t> counts;
    for (int i = 5; i < argc; ++i) counts.push_back(std::strtoull(argv[i], nullptr, 0));
    const int nb = static_cast<int>(counts.size());

    const kf::Workspace w = kf::plan_workspace(counts.data(), nb, world, sz, a2a);
    if (w.shards.size() != counts.size() || w.tails.size() != counts.size()) return 3;
    std::printf("ws %zu |", w.bytes);
    for (size_t off : w.shards) std::printf(" %zu", off);
    std::printf(" |");
    for (size_t off : w.tails) std::printf(" %zu", off);
    std::printf("\ngroups");
    for (int cut : kf::split_groups(counts.data(), nb, G)) std::printf(" %d", cut);
    std::printf("\n");
    return 0;
}
