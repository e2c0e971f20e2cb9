// smooth_tile_launch.hpp -- launch of k_smooth_tile_bwd (smooth_tile_kernels.hpp) for NT = 5 .. 8 column tiles (65 ..
// 128 states).  The template is instantiated in smooth_tile_nt.hip, once per NT (one translation unit each, like
// filter_tile_nt.hip: 24 kernels per unit), and only declared for smooth_tile.hip.
#pragma once
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "smooth_tile_kernels.hpp"

namespace bhmm {

struct SmoothTileBwdArgs {
    const ScoreTileModel *dm; // the model's table entry on the device (its W: the warm-up of this pass)
    Segs sg;                  // the plan's segments (all of them: the tile table names them)
    TilePlan tp;              // the backward tiles of ONE range
    const double *ws;         // the filtered rows of that range, global step g at ws[(g - g_first) * n]
    int64_t g_first;
    int form;                 // SMT_*
    void *out;                // nullptr: boundary vectors only (the calibration form)
    float *conf;              // decode: [total] or nullptr
    const double *V;          // device copy of the projection, or nullptr
    int Q;
    double *bexit, *bentry;   // [nseg][n]
    uint8_t *seg_flag;        // [nseg]
};

// one launch of k_smooth_tile_bwd on c->stream
template <int NT, int KIND>
int smooth_tile_bwd_launch(bhmm_ctx *c, const SmoothTileBwdArgs &a);

#define SMOOTH_TILE_LAUNCH_DECL(X, NTV)                                                                           \
    X template int smooth_tile_bwd_launch<NTV, EMIT_GAUSS>(bhmm_ctx *, const SmoothTileBwdArgs &);               \
    X template int smooth_tile_bwd_launch<NTV, EMIT_DISC>(bhmm_ctx *, const SmoothTileBwdArgs &);
} // namespace bhmm
