// smooth_tile_api.hpp -- what post_api.hip and marg_api.hip see of smooth_tile.hip: the matrix-core path of the two
// posterior calls for 65..128 states (post_path / marg_path 3).  The kernels compile in
// smooth_tile_nt.hip (one unit per column-tile count), the plan, the ranges, the warm-up and the protocol in
// smooth_tile.hip.  The call forms and the output description are those of the 9..64-state path.
#pragma once
#include <stdint.h>

#include "ctx.hpp"
#include "host_internal.hpp"
#include "smooth_wide_launch.hpp" // SMOOTH_FORM_*, SmoothWideOut

namespace bhmm {

// smooth_tile = -1: does a call of this form take the path by itself once the set has SMOOTH_TILE_MIN_TOTAL steps?
// Only where tools/smooth_tile_time.py measured the slowest call on path 3 faster than the fastest on the generic
// route in every shape measured (profiles/smooth/smooth_tile_time.json; the table in DESIGN.md section 18, which
// tests/test_smooth_tile_gpu.py mirrors as AUTO).
constexpr bool SMOOTH_TILE_AUTO_DECODE = false, SMOOTH_TILE_AUTO_DECODE_CONF = false, SMOOTH_TILE_AUTO_ROWS = false,
               SMOOTH_TILE_AUTO_PROJ = false;
constexpr bool smooth_tile_auto(int form)
{
    return form == SMOOTH_FORM_DECODE ? SMOOTH_TILE_AUTO_DECODE
           : form == SMOOTH_FORM_DECODE_CONF ? SMOOTH_TILE_AUTO_DECODE_CONF
           : form == SMOOTH_FORM_ROWS ? SMOOTH_TILE_AUTO_ROWS
                                      : SMOOTH_TILE_AUTO_PROJ;
}

// which path a posterior call takes: what k_filter_tile is eligible for -- 65..128 states (c->gen), gaussian or
// discrete emissions, loaded observations (explicit pobs have another kind)
inline bool smooth_tile_takes(const bhmm_ctx *c, int form)
{
    const bool emis = c->kind == BHMM_EMIT_GAUSSIAN || c->kind == BHMM_EMIT_DISCRETE;
    if (!c->gen || !emis || c->n < 65 || c->n > 128 || c->opt.smooth_tile == 0)
        return false;
    return c->opt.smooth_tile == 1 || (c->total >= SMOOTH_TILE_MIN_TOTAL && smooth_tile_auto(form));
}

// One call on the path: plan and ranges, warm-up, forward and backward launches per range of the budgeted
// workspace, the check of both directions.  *verified: the results in o stand.  Boundaries that did not verify at
// the first warm-up count one in *fallbacks and the pass runs once more with twice the warm-up; a flagged segment
// in either direction ends the call at once, nothing counted.  *verified false: the caller takes the generic path.
int smooth_tile_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                    const SmoothWideOut &o, int *fallbacks, bool *verified);

} // namespace bhmm
