// smooth_wide_launch.hpp -- what post_api.hip and marg_api.hip see of smooth_wide.hip: the time-segmented path of
// the two posterior calls for 9..64 states (post_path / marg_path 2).  The 54 instantiations of
// k_smooth_wide_bwd (smooth_wide_kernels.hpp), the plan, the warm-up and the protocol compile in that unit.
#pragma once
#include <stdint.h>

#include "ctx.hpp"
#include "host_internal.hpp"

namespace bhmm {

// the call forms the automatic rule tells apart (the columns of the table in DESIGN.md section 17)
enum { SMOOTH_FORM_DECODE = 0, SMOOTH_FORM_DECODE_CONF = 1, SMOOTH_FORM_ROWS = 2, SMOOTH_FORM_PROJ = 3 };

struct SmoothWideOut {
    int form;         // SMOOTH_FORM_*
    void *out;        // device: paths (bytes or int32, [total]) or rows (double / float, [total][Q > 0 ? Q : n])
    bool narrow;      // paths: one byte per step; rows: float
    float *conf;      // device, [total], or nullptr (decode)
    const double *V;  // device copy of the projection, or nullptr
    int Q;
};

// smooth_wide = -1: does a call of this form at np lanes per segment (16, 32, 64) take the path by itself once the
// set has SMOOTH_WIDE_MIN_TOTAL steps?  Only where tools/smooth_wide_time.py measured it faster than the generic
// route by more than the run-to-run spread (profiles/smooth/smooth_wide_time.json).
// Measured: at 128 x 1e5 steps decoding (16, 32 lanes) and projections (all classes) win, rows never do; at 128 x 1e4
// every form loses at 16 and 64 lanes.  No cell wins in every shape measured, so every class is opt-in (smooth_wide = 1).
constexpr bool smooth_wide_auto(int np, int form)
{
    (void)np;
    (void)form;
    return false;
}

// which path a posterior call takes: 9..64 states (c->wide), gaussian or discrete emissions
inline bool smooth_wide_takes(const bhmm_ctx *c, int form)
{
    const bool emis = c->kind == BHMM_EMIT_GAUSSIAN || c->kind == BHMM_EMIT_DISCRETE;
    if (!c->wide || !emis || c->n > 64 || c->opt.smooth_wide == 0)
        return false;
    return c->opt.smooth_wide == 1 || (c->total >= SMOOTH_WIDE_MIN_TOTAL && smooth_wide_auto(c->N, form));
}

// One call on the path: plan, warm-up, forward and backward launches per range of the budgeted workspace, the
// check of both directions.  *verified: the results in o stand.  Boundaries that did not verify at the first
// warm-up count one in *fallbacks and the pass runs once more with twice the warm-up; a dead or flagged segment
// ends the call at once, nothing counted.  *verified false: the caller takes the generic path.
int smooth_wide_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                    const SmoothWideOut &o, int *fallbacks, bool *verified);

} // namespace bhmm
