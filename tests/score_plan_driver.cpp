// Driver of tests/test_score_wide_cpu.py: the segment plan of bhmm_score for 9..64 states, exactly as
// score_api.hip makes it (plan::score_seglen, then plan::plan_segments with mult 1), on the host alone.
//   score_plan_driver NP NUM_SIMD ASKED OFFSET_0 ... OFFSET_K
// prints "seglen L", one "seg TRAJ T0 LEN" per segment and "traj0 I_0 ... I_K".
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "plan.hpp"

int main(int argc, char **argv)
{
    if (argc < 6)
        return 2;
    const int np = atoi(argv[1]), num_simd = atoi(argv[2]);
    const int64_t asked = atoll(argv[3]);
    std::vector<int64_t> off;
    for (int i = 4; i < argc; ++i)
        off.push_back(atoll(argv[i]));
    const int K = (int)off.size() - 1;
    const int64_t seglen = bhmm::plan::score_seglen(off[K] - off[0], np, num_simd, asked);
    bhmm::plan::SegPlan sp;
    bhmm::plan::plan_segments(off, K, seglen, 1, sp);
    printf("seglen %lld\n", (long long)seglen);
    for (size_t s = 0; s < sp.traj.size(); ++s)
        printf("seg %d %lld %d\n", sp.traj[s], (long long)sp.t0[s], sp.len[s]);
    printf("traj0");
    for (int k = 0; k <= K; ++k)
        printf(" %d", sp.traj0[k]);
    printf("\n");
    return 0;
}
