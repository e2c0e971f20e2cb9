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
