// score_tile_launch.hpp -- launch of k_score_tile (score_tile_kernels.hpp) for NT = 5 .. 8 column tiles (65 .. 128
// states).  The template is instantiated in score_tile_nt.hip, once per NT (one translation unit each, like
// tile_gen_nt.hip), and only declared for score_api.hip.
#pragma once
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "score_tile_kernels.hpp"

namespace bhmm {
// the forward pass of models [0, Sb) of the table dm over the score plan (sg, tp); flags: SCORE_TILE_FLAGS words
// per model
template <int NT, int KIND>
int score_tile_launch(bhmm_ctx *c, int Sb, const ScoreTileModel *dm, const Segs &sg, const TilePlan &tp,
                      unsigned int *flags);

#define SCORE_TILE_LAUNCH_DECL(X, NTV)                                                                            \
    X template int score_tile_launch<NTV, EMIT_GAUSS>(bhmm_ctx *, int, const ScoreTileModel *, const Segs &,     \
                                                      const TilePlan &, unsigned int *);                         \
    X template int score_tile_launch<NTV, EMIT_DISC>(bhmm_ctx *, int, const ScoreTileModel *, const Segs &,      \
                                                     const TilePlan &, unsigned int *);
} // namespace bhmm
