// filter_tile_launch.hpp -- launch of k_filter_tile (filter_tile_kernels.hpp) for NT = 5 .. 8 column tiles (65 .. 128
// states).  The template is instantiated in filter_tile_nt.hip, once per NT (one translation unit each, like
// score_tile_nt.hip), and only declared for filter_api.hip.
#pragma once
#include "filter_tile_kernels.hpp"
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"

namespace bhmm {

struct FilterTileArgs {
    const ScoreTileModel *dm; // the model's table entry on the device (its W: the warm-up of this pass)
    Segs sg;                  // the tile filter plan
    TilePlan tp;
    void *rows, *logc;        // double / float (f32) or nullptr; both nullptr: boundary vectors only
    const double *V;          // device copy of the projection, or nullptr
    int Q;
    bool f32;
    double *aentry, *aexit;   // [nseg][n]
    uint8_t *seg_flag;        // [nseg]
};

// one launch of k_filter_tile on c->stream
template <int NT, int KIND>
int filter_tile_launch(bhmm_ctx *c, const FilterTileArgs &a);

#define FILTER_TILE_LAUNCH_DECL(X, NTV)                                                                           \
    X template int filter_tile_launch<NTV, EMIT_GAUSS>(bhmm_ctx *, const FilterTileArgs &);                      \
    X template int filter_tile_launch<NTV, EMIT_DISC>(bhmm_ctx *, const FilterTileArgs &);
} // namespace bhmm
