// Driver of tests/test_score_tile_cpu.py: the segment plan and the tile table of bhmm_score for 65..128 states,
// exactly as score_api.hip makes them (plan::score_tile_seglen, plan::plan_segments with mult 1, then
// plan::plan_tiles for the forward direction), on the host alone.
//   score_tile_plan_driver NUM_SIMD ASKED OFFSET_0 ... OFFSET_K
// prints "seglen L", one "seg TRAJ T0 LEN" per segment, "traj0 I_0 ... I_K" and one "tile S_0 ... S_15" per tile.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "plan.hpp"

int main(int argc, char **argv)
{
    if (argc < 5)
        return 2;
    const int num_simd = atoi(argv[1]);
    const int64_t asked = atoll(argv[2]);
    std::vector<int64_t> off;
    for (int i = 3; i < argc; ++i)
        off.push_back(atoll(argv[i]));
    const int K = (int)off.size() - 1;
    const int64_t seglen = bhmm::plan::score_tile_seglen(off[K] - off[0], num_simd, asked);
    bhmm::plan::SegPlan sp;
    bhmm::plan::plan_segments(off, K, seglen, 1, sp);
    std::vector<int32_t> tile_seg;
    bhmm::plan::plan_tiles(sp, off, false, tile_seg);
    printf("seglen %lld\n", (long long)seglen);
    for (size_t s = 0; s < sp.traj.size(); ++s)
        printf("seg %d %lld %d\n", sp.traj[s], (long long)sp.t0[s], sp.len[s]);
    printf("traj0");
    for (int k = 0; k <= K; ++k)
        printf(" %d", sp.traj0[k]);
    printf("\n");
    if (tile_seg.size() % 16 != 0)
        return 3;
    for (size_t t = 0; t < tile_seg.size(); t += 16) {
        printf("tile");
        for (int r = 0; r < 16; ++r)
            printf(" %d", tile_seg[t + r]);
        printf("\n");
    }
    return 0;
}
