// Driver of tests/test_probe_plan_cpu.py: the host arithmetic the verified time-parallel passes share (csrc/plan.hpp),
// on the host alone.
//   probe_plan_driver wmax MAXT                       prints "narrow W" and "wide W" (probe_wmax, probe_wmax_wide)
//   probe_plan_driver starts WMAX P OFFSET_0 ... OFFSET_K
//                                                     prints "start S" per sample position (probe_starts)
//   probe_plan_driver read WMAX TARGET BOTH [INDEX:VALUE ...]
//                                                     a curve of 2 WMAX zeros but for the given entries; prints
//                                                     "last L" (curve_last), "narrow W" (warmup_of) and "wide W"
//                                                     (warmup_wide_of)
//   probe_plan_driver plan NP NUM_SIMD ASKED OFFSET_0 ... OFFSET_K
//   probe_plan_driver tileplan NUM_SIMD ASKED OFFSET_0 ... OFFSET_K
//                                                     the plan of a forward-only pass as bhmm_score and bhmm_filter
//                                                     make it (plan_pass with score_seglen / score_tile_seglen), in the
//                                                     format of score_plan_driver / score_tile_plan_driver, then
//                                                     "ntraj N"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "plan.hpp"

using namespace bhmm::plan;

static std::vector<int64_t> offsets_from(int argc, char **argv, int first)
{
    std::vector<int64_t> off;
    for (int i = first; i < argc; ++i)
        off.push_back(atoll(argv[i]));
    return off;
}

int main(int argc, char **argv)
{
    if (argc < 3)
        return 2;
    const std::string mode = argv[1];
    if (mode == "wmax") {
        printf("narrow %d\nwide %d\n", probe_wmax(atoll(argv[2])), probe_wmax_wide(atoll(argv[2])));
        return 0;
    }
    if (mode == "starts" && argc >= 6) {
        const int Wmax = atoi(argv[2]), P = atoi(argv[3]);
        const std::vector<int64_t> off = offsets_from(argc, argv, 4);
        std::vector<int64_t> starts;
        probe_starts(off, (int)off.size() - 1, Wmax, P, starts);
        for (int64_t s : starts)
            printf("start %lld\n", (long long)s);
        return 0;
    }
    if (mode == "read" && argc >= 5) {
        const int Wmax = atoi(argv[2]);
        const float target = strtof(argv[3], nullptr);
        const bool both = atoi(argv[4]) != 0;
        std::vector<float> curve(2 * (size_t)Wmax, 0.f);
        for (int i = 5; i < argc; ++i) {
            const char *colon = strchr(argv[i], ':');
            const long at = atol(argv[i]);
            if (!colon || at < 0 || at >= 2L * Wmax)
                return 2;
            curve[at] = strtof(colon + 1, nullptr);
        }
        const int last = curve_last(curve.data(), Wmax, target, both);
        printf("last %d\nnarrow %d\nwide %d\n", last, warmup_of(last, Wmax), warmup_wide_of(last));
        return 0;
    }
    const bool tiles = mode == "tileplan";
    if ((mode != "plan" && !tiles) || argc < (tiles ? 6 : 7))
        return 2;
    const std::vector<int64_t> off = offsets_from(argc, argv, tiles ? 4 : 5);
    const int K = (int)off.size() - 1;
    const int64_t total = off[K] - off[0];
    const int64_t seglen = tiles ? score_tile_seglen(total, atoi(argv[2]), atoll(argv[3]))
                                 : score_seglen(total, atoi(argv[2]), atoi(argv[3]), atoll(argv[4]));
    PassPlan p;
    plan_pass(off, K, seglen, tiles, p);
    printf("seglen %lld\n", (long long)seglen);
    for (size_t s = 0; s < p.seg.traj.size(); ++s)
        printf("seg %d %lld %d\n", p.seg.traj[s], (long long)p.seg.t0[s], p.seg.len[s]);
    printf("traj0");
    for (int k = 0; k <= K; ++k)
        printf(" %d", p.seg.traj0[k]);
    printf("\n");
    if (p.tile_seg.size() % 16 != 0 || (!tiles && !p.tile_seg.empty()))
        return 3;
    for (size_t t = 0; t < p.tile_seg.size(); t += 16) {
        printf("tile");
        for (int r = 0; r < 16; ++r)
            printf(" %d", p.tile_seg[t + r]);
        printf("\n");
    }
    printf("ntraj %d\n", p.ntraj);
    return 0;
}
