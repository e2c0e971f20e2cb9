// smooth_tile_nt.hip -- k_smooth_tile_bwd (smooth_tile_kernels.hpp) for ONE column-tile count
// (-DSMOOTH_TILE_NT_VALUE=5 .. 8; 65 .. 128 states) and its launch: 2 emission kinds x 2 (all 16 NT states or fewer)
// x 6 forms = 24 kernels.  See smooth_tile.hip for the driver (plan, ranges, warm-up, boundary check, fallbacks).
#include "smooth_tile_launch.hpp"

namespace bhmm {
namespace {

template <int NT, int KIND, bool FULL, int FORM>
int launch_one(bhmm_ctx *c, const SmoothTileBwdArgs &a)
{
    BHMM_HIP(launch(k_smooth_tile_bwd<NT, KIND, FULL, FORM>, dim3(a.tp.ntiles), dim3(SCORE_TILE_THREADS), 0, c->stream,
                    a.dm, c->d_offsets.p, a.sg, a.tp, c->d_obs_rm.p, a.ws, a.g_first, a.out, a.conf, a.V, a.Q, a.bexit,
                    a.bentry, a.seg_flag));
    return BHMM_OK;
}

template <int NT, int KIND, bool FULL>
int launch_form(bhmm_ctx *c, const SmoothTileBwdArgs &a)
{
    switch (a.form) {
    case SMT_DECODE_U8:
        return launch_one<NT, KIND, FULL, SMT_DECODE_U8>(c, a);
    case SMT_DECODE_I32:
        return launch_one<NT, KIND, FULL, SMT_DECODE_I32>(c, a);
    case SMT_ROWS_F64:
        return launch_one<NT, KIND, FULL, SMT_ROWS_F64>(c, a);
    case SMT_ROWS_F32:
        return launch_one<NT, KIND, FULL, SMT_ROWS_F32>(c, a);
    case SMT_PROJ_F64:
        return launch_one<NT, KIND, FULL, SMT_PROJ_F64>(c, a);
    default:
        return launch_one<NT, KIND, FULL, SMT_PROJ_F32>(c, a);
    }
}

} // namespace

template <int NT, int KIND>
int smooth_tile_bwd_launch(bhmm_ctx *c, const SmoothTileBwdArgs &a)
{
    if (a.tp.ntiles <= 0)
        return BHMM_OK;
    return c->n == 16 * NT ? launch_form<NT, KIND, true>(c, a) : launch_form<NT, KIND, false>(c, a);
}

SMOOTH_TILE_LAUNCH_DECL(, SMOOTH_TILE_NT_VALUE)

} // namespace bhmm
