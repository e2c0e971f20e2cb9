// smooth_wide.hip -- the time-segmented path of bhmm_posterior_decode and bhmm_posterior_marginals for 9..64 states
// (post_path / marg_path 2) in a translation unit of its own: the 54 instantiations of
// k_smooth_wide_bwd (16 / 32 / 64 lanes per segment x gaussian / discrete with B^T in LDS / discrete with B^T read
// ahead x decode to bytes / decode to int32 / rows double / rows float / projection double / projection float), the
// forgetting probe of the family in both directions, the plan, the warm-up and the pass the protocol
// (plan::two_attempts, plan.hpp) runs.
//
// Forward half: k_filter_wide (filter_wide.hip, not changed) through filter_wide_launch, with rows = the workspace
// in double, no projection, no logc.  Backward half: k_smooth_wide_bwd over the same segments.  The workspace holds
// the filtered rows of one range of segments (plan::smooth_ranges; option smooth_ws_mb); every segment's arithmetic
// is its own, so the results do not depend on the budget.  Then k_wide_check over the boundary vectors of both
// directions at BOUNDARY_TOL.  Nothing here reads or writes c->filt, c->post, c->marg, the score plans or the
// E-step's state: the buffers are c->smooth.*, the plan's sizes ds.smooth_*, the only other fields touched are
// opt.smooth_* (read) and last.smooth_segments; the results go where the caller (post_api.hip, marg_api.hip) says.
#include <algorithm>
#include <vector>

#include "filter_wide_launch.hpp"
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "plan.hpp"
#include "seg_host.hpp"
#include "smooth_wide_kernels.hpp"
#include "smooth_wide_launch.hpp"

namespace bhmm {
namespace {

constexpr size_t SMOOTH_WIDE_LDS_BT = 16 * 1024; // B^T staged in LDS up to this size (k_filter_wide's limit)
enum { SMOOTH_FAILS = 0, SMOOTH_DEV = 1, SMOOTH_FLAGGED = 2, SMOOTH_WORDS = 3 };

// one range of the plan: the segments [s0, s1), whose first global step is g_first
struct BwdArgs {
    const ScoreWideModel *dm;
    int W;
    Segs sg; // the sub-view of the tables
    const double *ws;
    int64_t g_first;
    double *bexit, *bentry; // advanced to the range's first segment, like sg
    uint8_t *trouble;
};

template <int NP, int KIND, bool BT_LDS, int STAGE, typename OT>
int launch_one(bhmm_ctx *c, const BwdArgs &a, const SmoothWideOut &o, size_t lds)
{
    constexpr int GP = 64 / NP;
    BHMM_HIP(launch(k_smooth_wide_bwd<NP, KIND, BT_LDS, STAGE, OT>, dim3((a.sg.nseg + GP - 1) / GP), dim3(64), lds,
                    c->stream, a.dm, a.W, c->d_offsets.p, a.sg, c->d_obs_rm.p, a.ws, a.g_first,
                    static_cast<OT *>(o.out), o.conf, o.V, o.Q, a.bexit, a.bentry, a.trouble));
    return BHMM_OK;
}

template <int NP, int KIND, bool BT_LDS>
int launch_forms(bhmm_ctx *c, const BwdArgs &a, const SmoothWideOut &o, size_t lds)
{
    if (o.form == SMOOTH_FORM_DECODE || o.form == SMOOTH_FORM_DECODE_CONF)
        return o.narrow ? launch_one<NP, KIND, BT_LDS, SMOOTH_DECODE, uint8_t>(c, a, o, lds)
                        : launch_one<NP, KIND, BT_LDS, SMOOTH_DECODE, int32_t>(c, a, o, lds);
    if (o.form == SMOOTH_FORM_ROWS)
        return o.narrow ? launch_one<NP, KIND, BT_LDS, SMOOTH_ROWS, float>(c, a, o, lds)
                        : launch_one<NP, KIND, BT_LDS, SMOOTH_ROWS, double>(c, a, o, lds);
    return o.narrow ? launch_one<NP, KIND, BT_LDS, SMOOTH_PROJ, float>(c, a, o, lds)
                    : launch_one<NP, KIND, BT_LDS, SMOOTH_PROJ, double>(c, a, o, lds);
}

template <int NP>
int launch_np(bhmm_ctx *c, const BwdArgs &a, const SmoothWideOut &o)
{
    if (c->kind == EMIT_GAUSS)
        return launch_forms<NP, EMIT_GAUSS, false>(c, a, o, 0);
    const size_t lds_bt = (size_t)c->M * NP * sizeof(double);
    if (lds_bt <= SMOOTH_WIDE_LDS_BT)
        return launch_forms<NP, EMIT_DISC, true>(c, a, o, lds_bt);
    return launch_forms<NP, EMIT_DISC, false>(c, a, o, 0);
}

int bwd_launch(bhmm_ctx *c, int np, const BwdArgs &a, const SmoothWideOut &o)
{
    return np == 16 ? launch_np<16>(c, a, o) : (np == 32 ? launch_np<32>(c, a, o) : launch_np<64>(c, a, o));
}

// k_wide_probe<np, kind>, the chains of both directions (2 P lane groups); curve: 2 * Wmax words, zeroed
template <int NP>
int probe_np(bhmm_ctx *c, const WideModel &m, const int64_t *d_starts, int P, int Wmax, unsigned int *d_curve)
{
    constexpr int GP = 64 / NP;
    if (c->kind == EMIT_GAUSS)
        BHMM_HIP(launch(k_wide_probe<NP, EMIT_GAUSS>, dim3(2 * P / GP), dim3(64), 0, c->stream, m, c->d_obs_rm.p,
                        d_starts, P, Wmax, d_curve));
    else
        BHMM_HIP(launch(k_wide_probe<NP, EMIT_DISC>, dim3(2 * P / GP), dim3(64), 0, c->stream, m, c->d_obs_rm.p,
                        d_starts, P, Wmax, d_curve));
    return BHMM_OK;
}

// the segment plan of the smoothing pass on this observation set: made at the first eligible call (and again when
// smooth_seglen changes), never after a check.  Not the filter plan, not the score plan and not the E-step's
int smooth_plan(bhmm_ctx *c)
{
    auto &d = c->ds;
    auto &b = c->smooth;
    if (d.smooth_nseg > 0 && d.smooth_seglen_opt == c->opt.smooth_seglen)
        return BHMM_OK;
    const int64_t seglen = plan::score_seglen(c->total, c->N, c->num_simd, c->opt.smooth_seglen);
    int rc, ntiles;
    if ((rc = make_seg_tables(c, b.seg, seglen, false, &d.smooth_nseg, &d.smooth_ntraj, &ntiles)))
        return rc;
    // the same plan on the host: the ranges of the budgeted workspace are cut from it
    plan::PassPlan p;
    plan::plan_pass(c->offsets, c->K, seglen, false, p);
    b.seg_len = p.seg.len;
    b.seg_g0.resize(p.seg.t0.size());
    for (size_t s = 0; s < p.seg.t0.size(); ++s)
        b.seg_g0[s] = c->offsets[p.seg.traj[s]] + p.seg.t0[s];
    d.smooth_seglen_opt = c->opt.smooth_seglen;
    return BHMM_OK;
}

// warm-up: the chains of k_wide_probe in both directions, read as WideFilt::probe (filter_api.hip) reads the forward
// ones -- within 1e-13 from then on, times 1.5, rounded up to 8, at most Wmax -- in the worse of the two directions
int probe(bhmm_ctx *c, const WideModel &m, int *W)
{
    *W = W_UNPROBED;
    const int Wmax = plan::probe_wmax_wide(longest_traj(c));
    if (Wmax == 0)
        return BHMM_OK;
    Probe pr;
    int rc;
    if ((rc = probe_stage(c, c->smooth.probe, Wmax, 1, pr)))
        return rc;
    rc = c->N == 16   ? probe_np<16>(c, m, pr.d_starts, PROBE_P, Wmax, pr.d_curve)
         : c->N == 32 ? probe_np<32>(c, m, pr.d_starts, PROBE_P, Wmax, pr.d_curve)
                      : probe_np<64>(c, m, pr.d_starts, PROBE_P, Wmax, pr.d_curve);
    if (rc)
        return rc;
    std::vector<float> curve; // (forward | backward)
    if ((rc = probe_read(c, pr, curve)))
        return rc;
    // (not forgotten within Wmax: Wmax, the check decides)
    *W = std::min(plan::warmup_wide_of(plan::curve_last(curve.data(), Wmax, 1e-13f, true)), Wmax);
    return BHMM_OK;
}

// both launches over every range, then the flags and the check; words: SMOOTH_WORDS of them
int pass(bhmm_ctx *c, const ScoreWideModel *dm, int W, const SmoothWideOut &o, unsigned int *words)
{
    auto &b = c->smooth;
    const int n = c->n, nseg = c->ds.smooth_nseg, gp = 64 / c->N;
    std::vector<plan::SegRange> ranges;
    plan::smooth_ranges(b.seg_len, gp, (int64_t)n * (int64_t)sizeof(double), (int64_t)c->opt.smooth_ws_mb << 20, ranges);
    int64_t most = 1;
    for (const auto &r : ranges)
        most = std::max(most, r.steps);
    int rc;
    if ((rc = b.ws.ensure((size_t)most * n)))
        return rc;
    BHMM_HIP(hipMemsetAsync(b.fails.p, 0, SMOOTH_WORDS * sizeof(unsigned int), c->stream));
    for (const auto &r : ranges) {
        const int64_t g_first = b.seg_g0[r.s0];
        Segs sg;
        sg.traj = b.seg.seg_traj.p + r.s0;
        sg.t0 = b.seg.seg_t0.p + r.s0;
        sg.len = b.seg.seg_len.p + r.s0;
        sg.nseg = r.s1 - r.s0;
        sg.W = W;
        FilterWideArgs f;
        f.dm = dm;
        f.W = W;
        f.sg = sg;
        f.rows = b.ws.p - g_first * n; // (global step g lands at ws[(g - g_first) * n])
        f.logc = nullptr;
        f.V = nullptr;
        f.Q = 0;
        f.f32 = false;
        f.aentry = b.aentry.p + (int64_t)r.s0 * n;
        f.aexit = b.aexit.p + (int64_t)r.s0 * n;
        f.dead = b.dead.p + r.s0;
        if ((rc = filter_wide_launch(c, c->N, f)))
            return rc;
        BwdArgs a;
        a.dm = dm;
        a.W = W;
        a.sg = sg;
        a.ws = b.ws.p;
        a.g_first = g_first;
        a.bexit = b.bexit.p + (int64_t)r.s0 * n;
        a.bentry = b.bentry.p + (int64_t)r.s0 * n;
        a.trouble = b.trouble.p + r.s0;
        if ((rc = bwd_launch(c, c->N, a, o)))
            return rc;
    }
    BHMM_HIP(launch(k_smooth_flags, dim3((nseg + 255) / 256), dim3(256), 0, c->stream, b.dead.p, b.trouble.p, nseg,
                    b.fails.p + SMOOTH_FLAGGED));
    if (nseg > c->ds.smooth_ntraj) // (no boundary: the exact recursions)
        BHMM_HIP(launch(k_wide_check, dim3((nseg + 15) / 16), dim3(256), 0, c->stream,
                        segs_of_tables<Segs>(b.seg, nseg, W), n, b.aentry.p, b.aexit.p, b.bexit.p, b.bentry.p,
                        BOUNDARY_TOL, b.fails.p));
    BHMM_HIP(hipMemcpyAsync(words, b.fails.p, SMOOTH_WORDS * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    return BHMM_OK;
}

} // namespace

int smooth_wide_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                    const SmoothWideOut &o, int *fallbacks, bool *verified)
{
    auto &b = c->smooth;
    const int M = c->M, n = c->n;
    *verified = false;
    int rc;
    if ((rc = smooth_plan(c)))
        return rc;
    const int nseg = c->last.smooth_segments = c->ds.smooth_nseg;
    const bool segmented = nseg > c->ds.smooth_ntraj;
    const bool disc = c->kind == EMIT_DISC;
    const size_t np = wide_block_size(n, M, disc, true);
    const size_t nvec = (size_t)std::max(nseg, 1) * n;
    if ((rc = b.model.ensure(sizeof(ScoreWideModel))) || (rc = b.wpar.ensure(np)) || (rc = b.aentry.ensure(nvec)) ||
        (rc = b.aexit.ensure(nvec)) || (rc = b.bexit.ensure(nvec)) || (rc = b.bentry.ensure(nvec)) ||
        (rc = b.dead.ensure(std::max(nseg, 1))) || (rc = b.trouble.ensure(std::max(nseg, 1))) ||
        (rc = b.fails.ensure(SMOOTH_WORDS)))
        return rc;
    if (nseg == 0) { // (no trajectory has a step: nothing to write)
        *verified = true;
        return BHMM_OK;
    }
    std::vector<double> h(np, 0.0);
    ScoreWideModel m;
    m.Bt = fill_wide_block(n, M, disc, true, A, pi, par0, par1, h.data(), b.wpar.p, m.w);
    ScoreWideModel *dm = reinterpret_cast<ScoreWideModel *>(b.model.p);
    BHMM_HIP(hipMemcpyAsync(b.wpar.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(dm, &m, sizeof(ScoreWideModel), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream)); // (h and m are temporaries)
    // a plan without a boundary runs the exact recursions: no probe, no check
    int W = (int)std::min<int64_t>(((int64_t)c->opt.smooth_W + 7) / 8 * 8, 1 << 30);
    if (segmented && c->opt.smooth_W <= 0 && (rc = probe(c, m.w, &W)))
        return rc;
    W = std::max(W, 8);
    return plan::two_attempts(
        W, 1 << 30, fallbacks,
        [&](int w, plan::Verdict *v) {
            unsigned int words[SMOOTH_WORDS] = {0, 0, 0};
            const int rc2 = pass(c, dm, w, o, words);
            // probability zero, a NaN observation, a sum outside the range: the generic path gives its answer (or its
            // error); nothing is counted
            *v = words[SMOOTH_FLAGGED] != 0 ? plan::Verdict::abandon : plan::verdict_of(words[SMOOTH_FAILS]);
            return rc2;
        },
        verified);
}

} // namespace bhmm
