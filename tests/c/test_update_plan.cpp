// The host launch planner of the optimizer-update kernels
// (kungfu_amd/csrc/kf_update_batch.hpp plan_update_batch), driven without HIP:
// a unit of 4 elements, tiles of 1024 units, tables of 32 segments, a `fill`
// that records the segment's index and a `launch` that prints the launch.
//
//   test_update_plan FAIL_AT [COUNT ...]
//
// prints one line "gx gy nseg | blk0[0..nseg] | the segments' indices" per
// launch and "rc N" at the end. Launch number FAIL_AT (from 0; -1: none)
// returns status 7 instead of KF_OK. No memory is touched: the counts are
// plain numbers. tests/test_update_plan.py builds this with
// -fsanitize=address,undefined and checks the output.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kf_update_batch.hpp"

namespace
{
struct Seg {
    int b;
};
struct Args {
    Seg seg[32];
    unsigned blk0[33];
    int nseg;
};
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const int fail_at = std::atoi(argv[1]);
    std::vector<size_t> counts;
    for (int i = 2; i < argc; ++i) counts.push_back(std::strtoull(argv[i], nullptr, 0));
    int launches = 0;
    const int rc = kf::plan_update_batch<Args>(
        counts.data(), static_cast<int>(counts.size()), 4, 1024,
        [](Seg &g, int b) { g.b = b; },
        [&](unsigned gx, unsigned gy, const Args &a) {
            std::printf("%u %u %d |", gx, gy, a.nseg);
            for (int i = 0; i <= a.nseg; ++i) std::printf(" %u", a.blk0[i]);
            std::printf(" |");
            for (int i = 0; i < a.nseg; ++i) std::printf(" %d", a.seg[i].b);
            std::printf("\n");
            return launches++ == fail_at ? 7 : KF_OK;
        });
    std::printf("rc %d\n", rc);
    return 0;
}
