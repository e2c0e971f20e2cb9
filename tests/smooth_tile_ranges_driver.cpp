// Driver of tests/test_smooth_tile_cpu.py: the ranges of segments the posterior calls at 65..128 states cut their
// plan into for a budgeted workspace, with the forward and backward tile tables of every range, exactly as
// smooth_tile.hip makes them (plan::plan_segments, plan::smooth_tile_ranges), on the host alone.
//   smooth_tile_ranges_driver ROW_BYTES BUDGET_BYTES SEGLEN T_0 ... T_{K-1}
// prints one "seg TRAJ T0 LEN" per segment, one "range S0 S1 STEPS F0 NF B0 NB" per range and one "tilef ..." /
// "tileb ..." line of sixteen segment numbers per tile of the two concatenated tables.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "plan.hpp"

int main(int argc, char **argv)
{
    if (argc < 4)
        return 2;
    const int64_t row_bytes = atoll(argv[1]), budget = atoll(argv[2]), seglen = atoll(argv[3]);
    std::vector<int64_t> offsets(1, 0);
    for (int i = 4; i < argc; ++i)
        offsets.push_back(offsets.back() + atoll(argv[i]));
    const int K = (int)offsets.size() - 1;
    bhmm::plan::SegPlan s;
    bhmm::plan::plan_segments(offsets, K, seglen, 1, s);
    std::vector<bhmm::plan::TileRange> ranges;
    std::vector<int32_t> tf, tb;
    bhmm::plan::smooth_tile_ranges(s, offsets, row_bytes, budget, ranges, tf, tb);
    for (size_t i = 0; i < s.traj.size(); ++i)
        printf("seg %d %lld %d\n", s.traj[i], (long long)s.t0[i], s.len[i]);
    for (const auto &r : ranges)
        printf("range %d %d %lld %d %d %d %d\n", r.s0, r.s1, (long long)r.steps, r.f0, r.nf, r.b0, r.nb);
    for (int dir = 0; dir < 2; ++dir) {
        const std::vector<int32_t> &t = dir ? tb : tf;
        for (size_t i = 0; i < t.size(); ++i)
            printf("%s%d%s", i % 16 == 0 ? (dir ? "tileb " : "tilef ") : "", t[i], i % 16 == 15 ? "\n" : " ");
    }
    return 0;
}
