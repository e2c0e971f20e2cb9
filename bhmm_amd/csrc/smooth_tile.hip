// smooth_tile.hip -- the matrix-core path of bhmm_posterior_decode and bhmm_posterior_marginals for 65..128 states
// (post_path / marg_path 3): the plan, the ranges of the budgeted workspace, the warm-up and
// the pass the protocol (plan::two_attempts, plan.hpp) runs.  The kernels compile in smooth_tile_nt.hip and
// filter_tile_nt.hip.
//
// Forward half: k_filter_tile<NT, KIND, FULL, double, false, false> (filter_tile_nt.hip, not changed) through
// filter_tile_launch, with rows = the workspace, no projection, no logc.  Backward half: k_smooth_tile_bwd over the
// same segments.  The workspace holds the filtered rows of one range of segments (plan::smooth_tile_ranges; option
// smooth_ws_mb); a tile's sixteen segments are picked by length among the segments of its range, so the tiles depend
// on the budget: results are bitwise reproducible at a fixed budget, across budgets that is not promised.  Then
// k_smooth_tile_flags and k_smooth_tile_check over the flags and boundary vectors of both directions at
// BOUNDARY_TOL.  One flagged segment (probability zero, an outlier, a NaN observation, in either direction) sends
// the WHOLE call to the generic route: there is no per-trajectory redo here.  Nothing here reads or writes c->filt,
// c->smooth, c->post, c->marg, the score plans or the E-step's state: the buffers are c->smooth_tile.*, the plan's
// sizes ds.smooth_tile_*, the only other fields touched are opt.smooth_* (read) and last.smooth_segments; the
// results go where the caller (post_api.hip, marg_api.hip) says.
#include <string.h>

#include <algorithm>
#include <vector>

#include "filter_tile_launch.hpp"
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "plan.hpp"
#include "seg_host.hpp"
#include "smooth_tile_api.hpp"
#include "smooth_tile_launch.hpp"

namespace bhmm {
FILTER_TILE_LAUNCH_DECL(extern, 5)
FILTER_TILE_LAUNCH_DECL(extern, 6)
FILTER_TILE_LAUNCH_DECL(extern, 7)
FILTER_TILE_LAUNCH_DECL(extern, 8)
SMOOTH_TILE_LAUNCH_DECL(extern, 5)
SMOOTH_TILE_LAUNCH_DECL(extern, 6)
SMOOTH_TILE_LAUNCH_DECL(extern, 7)
SMOOTH_TILE_LAUNCH_DECL(extern, 8)
namespace {

// the kernel's form of a call
int form_of(const SmoothWideOut &o)
{
    if (o.form == SMOOTH_FORM_DECODE || o.form == SMOOTH_FORM_DECODE_CONF)
        return o.narrow ? SMT_DECODE_U8 : SMT_DECODE_I32;
    if (o.form == SMOOTH_FORM_ROWS)
        return o.narrow ? SMT_ROWS_F32 : SMT_ROWS_F64;
    return o.narrow ? SMT_PROJ_F32 : SMT_PROJ_F64;
}

// the segment plan of the pass on this observation set, the ranges of its workspace and their tile tables: made at
// the first eligible call (and again when smooth_seglen or smooth_ws_mb changes), never after a check.  None of the
// other plans
int smooth_tile_plan(bhmm_ctx *c)
{
    auto &d = c->ds;
    auto &b = c->smooth_tile;
    if (d.smooth_tile_nseg > 0 && d.smooth_tile_seglen_opt == c->opt.smooth_seglen &&
        d.smooth_tile_ws_mb_opt == c->opt.smooth_ws_mb)
        return BHMM_OK;
    plan::SegPlan p;
    plan::plan_segments(c->offsets, c->K, plan::score_tile_seglen(c->total, c->num_simd, c->opt.smooth_seglen), 1, p);
    std::vector<plan::TileRange> ranges;
    std::vector<int32_t> tf, tb;
    plan::smooth_tile_ranges(p, c->offsets, (int64_t)c->n * (int64_t)sizeof(double), (int64_t)c->opt.smooth_ws_mb << 20,
                             ranges, tf, tb);
    const size_t ns = p.traj.size(), ns1 = std::max<size_t>(ns, 1);
    auto &t = b.seg;
    int rc;
    if ((rc = t.seg_traj.ensure(ns1)) || (rc = t.seg_len.ensure(ns1)) || (rc = t.seg_t0.ensure(ns1)) ||
        (rc = t.seg_traj0.ensure(c->K + 1)) || (rc = t.tile_seg.ensure(std::max<size_t>(tf.size(), 16))) ||
        (rc = b.tile_segb.ensure(std::max<size_t>(tb.size(), 16))))
        return rc;
    BHMM_HIP(hipMemcpyAsync(t.seg_traj.p, p.traj.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(t.seg_len.p, p.len.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(t.seg_t0.p, p.t0.data(), ns * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(t.seg_traj0.p, p.traj0.data(), (c->K + 1) * sizeof(int32_t), hipMemcpyHostToDevice,
                            c->stream));
    BHMM_HIP(hipMemcpyAsync(t.tile_seg.p, tf.data(), tf.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(b.tile_segb.p, tb.data(), tb.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream)); // (the plan is a temporary)
    const size_t nr = ranges.size();
    b.r_s0.resize(nr), b.r_s1.resize(nr), b.r_f0.resize(nr), b.r_nf.resize(nr), b.r_b0.resize(nr), b.r_nb.resize(nr);
    b.r_steps.resize(nr), b.r_g0.resize(nr);
    for (size_t i = 0; i < nr; ++i) {
        const plan::TileRange &r = ranges[i];
        b.r_s0[i] = r.s0, b.r_s1[i] = r.s1, b.r_f0[i] = r.f0, b.r_nf[i] = r.nf, b.r_b0[i] = r.b0, b.r_nb[i] = r.nb;
        b.r_steps[i] = r.steps;
        b.r_g0[i] = c->offsets[p.traj[r.s0]] + p.t0[r.s0];
    }
    d.smooth_tile_nseg = (int)ns;
    d.smooth_tile_ntraj = 0;
    for (int k = 0; k < c->K; ++k)
        d.smooth_tile_ntraj += c->offsets[k + 1] > c->offsets[k];
    d.smooth_tile_seglen_opt = c->opt.smooth_seglen;
    d.smooth_tile_ws_mb_opt = c->opt.smooth_ws_mb;
    return BHMM_OK;
}

template <int KIND>
struct TileSmooth {
    // what a pass left
    struct Verdict {
        unsigned int fails;   // boundaries out of tolerance, both directions
        float dev_f, dev_b;   // largest boundary deviation per direction
        unsigned int flagged; // segments outside the range of either kernel
    };

    // both launches over every range at warm-up W, then the flags and the check.  o == nullptr: boundary vectors
    // only, no workspace (calibration)
    static int pass(bhmm_ctx *c, ScoreTileModel *dm, ScoreTileModel &m, int W, const SmoothWideOut *o, Verdict *v)
    {
        auto &b = c->smooth_tile;
        const int n = c->n, nseg = c->ds.smooth_tile_nseg;
        int rc;
        if (o) {
            int64_t most = 1;
            for (int64_t st : b.r_steps)
                most = std::max(most, st);
            if ((rc = b.ws.ensure((size_t)most * n)))
                return rc;
        }
        m.W = W;
        BHMM_HIP(hipMemcpyAsync(dm, &m, sizeof(ScoreTileModel), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (m changes between passes)
        BHMM_HIP(hipMemsetAsync(b.words.p, 0, SMT_WORDS * sizeof(unsigned int), c->stream));
        const Segs sg = segs_of_tables<Segs>(b.seg, nseg, W);
        for (size_t i = 0; i < b.r_s0.size(); ++i) {
            const int64_t g_first = b.r_g0[i];
            FilterTileArgs f;
            f.dm = dm;
            f.sg = sg;
            f.tp = TilePlan{b.seg.tile_seg.p + (size_t)16 * b.r_f0[i], b.r_nf[i]};
            f.rows = o ? b.ws.p - g_first * n : nullptr; // (global step g lands at ws[(g - g_first) * n])
            f.logc = nullptr;
            f.V = nullptr;
            f.Q = 0;
            f.f32 = false;
            f.aentry = b.aentry.p;
            f.aexit = b.aexit.p;
            f.seg_flag = b.fflag.p;
            SmoothTileBwdArgs a;
            a.dm = dm;
            a.sg = sg;
            a.tp = TilePlan{b.tile_segb.p + (size_t)16 * b.r_b0[i], b.r_nb[i]};
            a.ws = b.ws.p;
            a.g_first = g_first;
            a.form = o ? form_of(*o) : SMT_DECODE_I32;
            a.out = o ? o->out : nullptr;
            a.conf = o ? o->conf : nullptr;
            a.V = o ? o->V : nullptr;
            a.Q = o ? o->Q : 0;
            a.bexit = b.bexit.p;
            a.bentry = b.bentry.p;
            a.seg_flag = b.bflag.p;
            if (f.tp.ntiles > 0 &&
                (rc = n <= 80   ? filter_tile_launch<5, KIND>(c, f)
                      : n <= 96  ? filter_tile_launch<6, KIND>(c, f)
                      : n <= 112 ? filter_tile_launch<7, KIND>(c, f)
                                 : filter_tile_launch<8, KIND>(c, f)))
                return rc;
            if ((rc = n <= 80   ? smooth_tile_bwd_launch<5, KIND>(c, a)
                      : n <= 96  ? smooth_tile_bwd_launch<6, KIND>(c, a)
                      : n <= 112 ? smooth_tile_bwd_launch<7, KIND>(c, a)
                                 : smooth_tile_bwd_launch<8, KIND>(c, a)))
                return rc;
        }
        BHMM_HIP(launch(k_smooth_tile_flags, dim3((nseg + 255) / 256), dim3(256), 0, c->stream, b.fflag.p, b.bflag.p,
                        nseg, b.words.p));
        if (nseg > c->ds.smooth_tile_ntraj) // (no boundary: the exact recursions)
            BHMM_HIP(launch(k_smooth_tile_check, dim3((nseg + 15) / 16), dim3(256), 0, c->stream, sg, n, b.aentry.p,
                            b.aexit.p, b.bentry.p, b.bexit.p, BOUNDARY_TOL, b.words.p));
        unsigned int f[SMT_WORDS];
        BHMM_HIP(hipMemcpyAsync(f, b.words.p, sizeof(f), hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        v->fails = f[SMT_FAILS_F] + f[SMT_FAILS_B];
        memcpy(&v->dev_f, &f[SMT_DEV_F], sizeof(float));
        memcpy(&v->dev_b, &f[SMT_DEV_B], sizeof(float));
        v->flagged = f[SMT_FLAGGED];
        return BHMM_OK;
    }

    // warm-up by the rule of bhmm_filter's TileFilt::calibrate (filter_api.hip), in both directions: the kernels
    // themselves, without outputs, at two warm-ups; the largest boundary deviation of each direction; the decay
    // between them extrapolated; the larger of the two results
    static int calibrate(bhmm_ctx *c, ScoreTileModel *dm, ScoreTileModel &m, int *W)
    {
        Verdict v0, v1;
        int rc;
        *W = SCORE_TILE_W0;
        if ((rc = pass(c, dm, m, SCORE_TILE_W0, nullptr, &v0)))
            return rc;
        const bool ok0 = v0.fails == 0;
        const bool good0_f = ok0 && (double)v0.dev_f <= SCORE_TILE_DEV_OK;
        const bool good0_b = ok0 && (double)v0.dev_b <= SCORE_TILE_DEV_OK;
        if (good0_f && good0_b)
            return BHMM_OK;
        if ((rc = pass(c, dm, m, SCORE_TILE_W1, nullptr, &v1)))
            return rc;
        const bool ok1 = v1.fails == 0;
        auto w_of = [&](bool good0, float d0, float d1) {
            if (good0)
                return SCORE_TILE_W0;
            return ok1 && (double)d1 <= SCORE_TILE_DEV_OK ? SCORE_TILE_W1
                                                          : score_tile_extrapolate((double)d0, (double)d1);
        };
        *W = std::max(w_of(good0_f, v0.dev_f, v1.dev_f), w_of(good0_b, v0.dev_b, v1.dev_b));
        return BHMM_OK;
    }

    static int run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                   const SmoothWideOut &o, int *fallbacks, bool *verified)
    {
        auto &b = c->smooth_tile;
        const int M = c->M, n = c->n;
        *verified = false;
        int rc;
        if ((rc = smooth_tile_plan(c)))
            return rc;
        const int nseg = c->last.smooth_segments = c->ds.smooth_tile_nseg;
        const bool segmented = nseg > c->ds.smooth_tile_ntraj;
        constexpr bool disc = KIND == EMIT_DISC;
        const size_t np = wide_block_size(n, M, disc, false); // (the kernels read B^T)
        const size_t nvec = (size_t)std::max(nseg, 1) * n;
        if ((rc = b.model.ensure(sizeof(ScoreTileModel))) || (rc = b.wpar.ensure(np)) || (rc = b.aentry.ensure(nvec)) ||
            (rc = b.aexit.ensure(nvec)) || (rc = b.bexit.ensure(nvec)) || (rc = b.bentry.ensure(nvec)) ||
            (rc = b.fflag.ensure(std::max(nseg, 1))) || (rc = b.bflag.ensure(std::max(nseg, 1))) ||
            (rc = b.words.ensure(SMT_WORDS)))
            return rc;
        if (nseg == 0) { // (no trajectory has a step: nothing to write)
            *verified = true;
            return BHMM_OK;
        }
        std::vector<double> h(np, 0.0);
        ScoreTileModel m;
        m.Bt = fill_wide_block(n, M, disc, false, A, pi, par0, par1, h.data(), b.wpar.p, m.w);
        m.W = 0;
        ScoreTileModel *dm = reinterpret_cast<ScoreTileModel *>(b.model.p);
        BHMM_HIP(hipMemcpyAsync(b.wpar.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (h is a temporary)
        // W: multiples of four (the refresh of the scaling).  A plan without a boundary runs the exact recursions: no
        // calibration, no check
        int W = segmented ? (int)std::min<int64_t>(((int64_t)c->opt.smooth_W + 3) & ~(int64_t)3, SCORE_TILE_W_MAX) : 0;
        if (segmented && c->opt.smooth_W <= 0 && (rc = calibrate(c, dm, m, &W)))
            return rc;
        return plan::two_attempts(
            W, SCORE_TILE_W_MAX, fallbacks,
            [&](int w, plan::Verdict *pv) {
                Verdict v = {};
                const int rc2 = pass(c, dm, m, w, &o, &v);
                // probability zero, an outlier, a NaN observation: the generic path gives its answer (or its error);
                // nothing is counted
                *pv = v.flagged != 0 ? plan::Verdict::abandon : plan::verdict_of(v.fails);
                return rc2;
            },
            verified);
    }
};

} // namespace

int smooth_tile_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                    const SmoothWideOut &o, int *fallbacks, bool *verified)
{
    return c->kind == EMIT_GAUSS ? TileSmooth<EMIT_GAUSS>::run(c, A, pi, par0, par1, o, fallbacks, verified)
                                 : TileSmooth<EMIT_DISC>::run(c, A, pi, par0, par1, o, fallbacks, verified);
}

} // namespace bhmm
