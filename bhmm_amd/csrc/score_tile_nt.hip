// score_tile_nt.hip -- k_score_tile (score_tile_kernels.hpp) for ONE column-tile count
// (-DSCORE_TILE_NT_VALUE=5 .. 8; 65 .. 128 states) and its launch.  See score_api.hip for the driver (plan,
// warm-up per model, boundary check, fallbacks).
#include "score_tile_launch.hpp"

namespace bhmm {

template <int NT, int KIND>
int score_tile_launch(bhmm_ctx *c, int Sb, const ScoreTileModel *dm, const Segs &sg, const TilePlan &tp,
                      unsigned int *flags)
{
    auto &b = c->score;
    auto *kern = c->n == 16 * NT ? k_score_tile<NT, KIND, true> : k_score_tile<NT, KIND, false>;
    BHMM_HIP(launch(kern, dim3(tp.ntiles, Sb), dim3(SCORE_TILE_THREADS), 0, c->stream, dm, c->d_offsets.p, sg, tp,
                    c->d_obs_rm.p, b.logLc.p, b.aentry.p, b.aexit.p, flags));
    return BHMM_OK;
}

SCORE_TILE_LAUNCH_DECL(, SCORE_TILE_NT_VALUE)

} // namespace bhmm
