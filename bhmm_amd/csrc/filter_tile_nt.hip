// filter_tile_nt.hip -- k_filter_tile (filter_tile_kernels.hpp) for ONE column-tile count
// (-DFILTER_TILE_NT_VALUE=5 .. 8; 65 .. 128 states) and its launch.  See filter_api.hip for the driver (plan,
// warm-up, boundary check, redo of single trajectories, fallbacks).
#include "filter_tile_launch.hpp"

namespace bhmm {
namespace {

template <int NT, int KIND, bool FULL, typename OT>
int launch_form(bhmm_ctx *c, const FilterTileArgs &a)
{
    const bool proj = a.Q > 0 && a.rows != nullptr;
    auto *kern = proj ? (a.logc ? k_filter_tile<NT, KIND, FULL, OT, true, true>
                                : k_filter_tile<NT, KIND, FULL, OT, true, false>)
                      : (a.logc ? k_filter_tile<NT, KIND, FULL, OT, false, true>
                                : k_filter_tile<NT, KIND, FULL, OT, false, false>);
    BHMM_HIP(launch(kern, dim3(a.tp.ntiles), dim3(SCORE_TILE_THREADS), 0, c->stream, a.dm, c->d_offsets.p, a.sg, a.tp,
                    c->d_obs_rm.p, static_cast<OT *>(a.rows), a.V, a.Q, static_cast<OT *>(a.logc), a.aentry, a.aexit,
                    a.seg_flag));
    return BHMM_OK;
}

} // namespace

template <int NT, int KIND>
int filter_tile_launch(bhmm_ctx *c, const FilterTileArgs &a)
{
    if (c->n == 16 * NT)
        return a.f32 ? launch_form<NT, KIND, true, float>(c, a) : launch_form<NT, KIND, true, double>(c, a);
    return a.f32 ? launch_form<NT, KIND, false, float>(c, a) : launch_form<NT, KIND, false, double>(c, a);
}

FILTER_TILE_LAUNCH_DECL(, FILTER_TILE_NT_VALUE)

} // namespace bhmm
