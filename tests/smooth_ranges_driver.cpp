// Driver of tests/test_smooth_wide_cpu.py: the ranges of segments the posterior calls at 9..64 states cut their
// plan into for a budgeted workspace, exactly as smooth_wide.hip makes them (plan::smooth_ranges), on the host alone.
//   smooth_ranges_driver GROUP ROW_BYTES BUDGET_BYTES LEN_0 ... LEN_{S-1}
// prints one "range S0 S1 STEPS" per range.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "plan.hpp"

int main(int argc, char **argv)
{
    if (argc < 4)
        return 2;
    const int group = atoi(argv[1]);
    const int64_t row_bytes = atoll(argv[2]), budget = atoll(argv[3]);
    std::vector<int32_t> len;
    for (int i = 4; i < argc; ++i)
        len.push_back((int32_t)atoll(argv[i]));
    std::vector<bhmm::plan::SegRange> ranges;
    bhmm::plan::smooth_ranges(len, group, row_bytes, budget, ranges);
    for (const auto &r : ranges)
        printf("range %d %d %lld\n", r.s0, r.s1, (long long)r.steps);
    return 0;
}
