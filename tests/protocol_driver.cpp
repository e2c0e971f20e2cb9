// Driver of tests/test_protocol_cpu.py: the acceptance protocol of a verified pass (csrc/plan.hpp: two_attempts,
// doubled), on the host alone.
//   protocol_driver run W CAP SCRIPT COUNTER
//       CAP     an integer, or "tile" for SCORE_TILE_W_MAX
//       SCRIPT  what the scripted pass answers, one letter per call: v (verified), f (failed), a (abandon), or a
//               digit 1..9 (that BHMM code, the verdict left as it was); a call past the script's end is an error
//       COUNTER the value of the fallback counter before the call
//     prints "call W" per call of the pass, then "counter C", "verified 0|1" and "rc R"
//   protocol_driver doubled W CAP      prints "doubled D"
//   protocol_driver cap                prints "tile SCORE_TILE_W_MAX"
// and the integer rules of the segment-parallel backward draw (draw_seglen, draw_next_warmup):
//   protocol_driver draw                                prints the four constants
//   protocol_driver draw_seglen TOTAL WANT              prints "seglen L"
//   protocol_driver draw_next_warmup W MISMATCH NSEG    prints "warmup W'"
// and those of the Viterbi passes (vit_*):
//   protocol_driver vit_seglen TOTAL[,TOTAL..] N NP W PER_SIMD WARMUPS NUM_SIMD
//       prints "seglen L" of the pass for N states, per TOTAL (NP: lanes per state vector up to 64 states; above 128
//       states PER_SIMD and WARMUPS are not read)
//   protocol_driver vit_w SPEC_W VIT_W TOTAL NUM_SIMD PER_SIMD MARGIN MEND
//       prints the warm-ups "estep", "wide" (9..64 states), "gen_cap" and "gen" (65..128), "rows" (129..256)
//   protocol_driver vit_next_warmup W LONGER CAP        prints "warmup W'"
//   protocol_driver vit_rows_give_up FAILS W MAXT       prints "give_up 0|1"
//   protocol_driver vit_chunk VIT_W VIT_BAD EXPLORE SPEC_W FIXED SCRIPT
//       the exploration machine of 8 states and fewer (vit_chunk_attempts) on a scripted attempt: a (accepted), c
//       (within tolerance, a close decision), f (out of tolerance) or a digit (that BHMM code); prints "call W FIRST"
//       per attempt, then "W", "bad", "explore" (the state it leaves), "accepted" (the last verdict) and "rc"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../include/bhmm_amd.h"
#include "plan.hpp"

using namespace bhmm::plan;

static_assert(BHMM_OK == 0, "two_attempts returns 0 for BHMM_OK");

static int64_t cap_of(const char *s) { return strcmp(s, "tile") == 0 ? (int64_t)SCORE_TILE_W_MAX : atoll(s); }

int main(int argc, char **argv)
{
    if (argc < 2)
        return 2;
    const std::string mode = argv[1];
    if (mode == "cap") {
        printf("tile %d\n", SCORE_TILE_W_MAX);
        return 0;
    }
    if (mode == "doubled" && argc == 4) {
        printf("doubled %d\n", doubled(atoi(argv[2]), cap_of(argv[3])));
        return 0;
    }
    if (mode == "draw") {
        printf("seglen_min %lld\nstart %d\nmax %d\nrounds %d\n", (long long)DRAW_SEGLEN_MIN, DRAW_W_START, DRAW_W_MAX,
               DRAW_MAX_ROUNDS);
        return 0;
    }
    if (mode == "draw_seglen" && argc == 4) {
        printf("seglen %lld\n", (long long)draw_seglen(atoll(argv[2]), atoll(argv[3])));
        return 0;
    }
    if (mode == "draw_next_warmup" && argc == 5) {
        printf("warmup %d\n", draw_next_warmup(atoi(argv[2]), atoll(argv[3]), atoll(argv[4])));
        return 0;
    }
    if (mode == "vit_seglen" && argc == 9) {
        const int n = atoi(argv[3]), np = atoi(argv[4]), W = atoi(argv[5]), per_simd = atoi(argv[6]), warmups = atoi(argv[7]),
                  num_simd = atoi(argv[8]);
        for (const char *p = argv[2]; p; p = strchr(p, ',') ? strchr(p, ',') + 1 : nullptr) {
            const int64_t total = atoll(p);
            const int64_t L = n <= 64    ? vit_wide_seglen(total, np, num_simd, per_simd, warmups, W)
                              : n <= 128 ? vit_gen_seglen(total, num_simd, per_simd, warmups, W)
                                         : vit_rows_seglen(vit_rows_fill(total, num_simd), W);
            printf("seglen %lld\n", (long long)L);
        }
        return 0;
    }
    if (mode == "vit_w" && argc == 9) {
        const int spec_W = atoi(argv[2]), vit_W = atoi(argv[3]), num_simd = atoi(argv[5]), per_simd = atoi(argv[6]);
        const bool margin = atoi(argv[7]) != 0, mend = atoi(argv[8]) != 0;
        const int64_t total = atoll(argv[4]);
        const int W0 = vit_w_estep(spec_W), cap = vit_gen_w_cap(W0, vit_gen_fill(total, num_simd, per_simd));
        printf("estep %d\nwide %d\ngen_cap %d\ngen %d\nrows %d\n", W0, vit_wide_w_start(vit_W, W0), cap,
               vit_gen_w_start(vit_W, W0, cap, margin, mend), vit_rows_w_start(vit_W, W0, vit_rows_fill(total, num_simd), mend));
        return 0;
    }
    if (mode == "vit_next_warmup" && argc == 5) {
        printf("warmup %d\n", vit_next_warmup(atoi(argv[2]), atoi(argv[3]) != 0, atoi(argv[4])));
        return 0;
    }
    if (mode == "vit_rows_give_up" && argc == 5) {
        printf("give_up %d\n", vit_rows_give_up(atoi(argv[2]), atoi(argv[3]), atoll(argv[4])) ? 1 : 0);
        return 0;
    }
    if (mode == "vit_chunk" && argc == 8) {
        int vit_W = atoi(argv[2]), vit_bad = atoi(argv[3]);
        bool explore = atoi(argv[4]) != 0;
        const std::string script = argv[7];
        size_t calls = 0;
        ChunkVerdict last;
        const int rc = vit_chunk_attempts(
            vit_W, vit_bad, explore, atoi(argv[5]), atoi(argv[6]) != 0,
            [&](int W, bool first, ChunkVerdict *v) {
                printf("call %d %d\n", W, first ? 1 : 0);
                if (calls >= script.size())
                    exit(3);
                const char ch = script[calls++];
                if (ch >= '1' && ch <= '9')
                    return ch - '0';
                v->accepted = ch == 'a';
                v->within = ch != 'f';
                return BHMM_OK;
            },
            &last);
        printf("W %d\nbad %d\nexplore %d\naccepted %d\nrc %d\n", vit_W, vit_bad, explore ? 1 : 0, last.accepted ? 1 : 0, rc);
        return 0;
    }
    if (mode != "run" || argc != 6)
        return 2;
    const std::string script = argv[4];
    int counter = atoi(argv[5]);
    size_t calls = 0;
    bool verified = true; // (two_attempts must clear it)
    const int rc = two_attempts(
        atoi(argv[2]), (int)cap_of(argv[3]), &counter,
        [&](int W, Verdict *v) {
            printf("call %d\n", W);
            if (calls >= script.size())
                exit(3);
            const char ch = script[calls++];
            if (ch >= '1' && ch <= '9')
                return ch - '0';
            *v = ch == 'v' ? Verdict::verified : (ch == 'a' ? Verdict::abandon : Verdict::failed);
            return BHMM_OK;
        },
        &verified);
    printf("counter %d\nverified %d\nrc %d\n", counter, verified ? 1 : 0, rc);
    return 0;
}
