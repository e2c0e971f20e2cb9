// filter_api.hip -- bhmm_filter: the filtered state probabilities P(s_t = i | o_0 .. o_t) of every step of every
// loaded trajectory (or their projection on up to 8 columns) and the one-step predictive log-densities
// log p(o_t | o_0 .. o_{t-1}), in double or float, in host buffers or left in device buffers of the caller.
// Kernels in filter_kernels.hpp; DESIGN.md section 16.
//
// Up to 8 states, gaussian or discrete (the fused path, filter_path 1): k_filter_sweep -- the forward sweep of
// k_score_fwd with the row and the increment as last stage -- over the E-step's chunk plan, then
// k_filter_first_dead (per trajectory the first chunk whose exit vector is all zero), k_filter_check over the
// boundary vectors up to there and k_filter_bury (zero rows and -inf in every chunk after it).  Warm-up from the
// forward reading of the forgetting probe, as bhmm_score takes it, or the option filter_W.  Boundaries that do
// not verify: counted in filter_fallbacks, the call runs again with twice the warm-up, and if they fail again it
// takes the serial path.
//
// 9 to 64 states, gaussian or discrete (the time-parallel path, filter_path 2): k_filter_wide
// (filter_wide_kernels.hpp; compiled in filter_wide.hip) -- the forward sweep of k_score_wide that sums every
// step, with the row and the increment as last stage -- over a segment plan that belongs to filtering alone
// (filter_plan: a function of the offsets, the state count and the device; option filter_seglen), then
// k_filter_first_dead, k_filter_seg_check and k_filter_seg_bury.  W from the forward chains of k_wide_probe as
// bhmm_score reads them, or filter_W; the same protocol.  Taken when the option filter_parallel is 1, or -1 (the
// default) and the set has at least FILTER_WIDE_MIN_TOTAL steps (host_internal.hpp).
//
// 65 to 128 states, gaussian or discrete, loaded observations (the matrix-core path, filter_path 3): k_filter_tile
// (filter_tile_kernels.hpp; compiled in filter_tile_nt.hip, one unit per column-tile count) -- k_score_tile for one
// model with the row and the increment as last stage -- over a segment plan and tile table of its own
// (filter_tile_plan: plan::score_tile_seglen with filter_seglen, plan::plan_tiles).  W by the rule of bhmm_score's
// Tile::calibrate: two passes of the kernel without outputs at W = 32 and 64, the decay of the largest boundary
// deviation extrapolated (score_tile_extrapolate), or filter_W.  The kernel flags every segment that left its number
// range (probability zero, an outlier, a NaN observation): k_filter_tile_redo marks their trajectories, which
// k_filter_serial does again, whole, behind the pass on the same stream (counted in filter_redone); their boundaries
// are not checked (k_filter_tile_check).  Boundaries that do not verify: the same protocol as above.  Taken when
// filter_parallel is not 0 and the option filter_tile is 1, or -1 (the default) and the set has at least
// FILTER_TILE_MIN_TOTAL steps.
//
// Everything else (more than 128 states, explicit pobs, filter_parallel / filter_tile 0 or a small set;
// filter_path 0): k_filter_serial, one workgroup per trajectory.
//
// The three verified paths run one protocol (plan::two_attempts, plan.hpp): a pass at the measured warm-up, and after
// boundaries that did not verify one more at twice that.  What they share with bhmm_score and the posterior calls is
// in plan.hpp (arithmetic, protocol), seg_host.hpp (device side) and fused_host.hpp (up to 8 states): the constants of
// the protocol, the probe's sample positions, staging and reading, the model upload and the warm-up of the fused path
// (upload_fused_model, fused_probe), the parameter block of a WideModel (fill_wide_block), the making of a plan's
// tables (make_seg_tables into c->filt.seg at 9..64 states, c->filt.tseg at 65..128) and the staging of the serial
// path's parameters (stage_serial_models).
//
// Nothing here reads or writes the state other calls use: the buffers are c->filt.*, the plans' sizes
// ds.filt_*, the only other fields touched are opt.filter_* (read) and last.filter_*.  Host results are staged in c->filt.rows / c->filt.logc and
// cross the link in ONE copy each, after the boundaries verified (copy_to_host_pinned, host_internal.hpp).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "filter_kernels.hpp"
#include "filter_tile_launch.hpp"
#include "filter_wide_launch.hpp"
#include "fused_host.hpp"
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "model_check.hpp"
#include "plan.hpp"
#include "seg_host.hpp"

namespace bhmm {
FILTER_TILE_LAUNCH_DECL(extern, 5)
FILTER_TILE_LAUNCH_DECL(extern, 6)
FILTER_TILE_LAUNCH_DECL(extern, 7)
FILTER_TILE_LAUNCH_DECL(extern, 8)
namespace {

// (BOUNDARY_TOL, W_UNPROBED, LDS_BT_MAX, the probe and the plan: seg_host.hpp, shared with bhmm_score and the
// posterior calls; the protocol: plan.hpp)

struct Out {          // where the results go on the device, and what they are
    void *rows;       // [total][Qp] of double / float, or nullptr
    void *logc;       // [total] of double / float, or nullptr
    const double *V;  // device copy of the projection, or nullptr
    int Q;            // its columns (0: none)
    int Qp;           // values per row
    bool f32;
};

template <int N, int KIND>
struct Fused {
    template <typename OT, bool PROJ, bool WANT_LOGC>
    static auto kernel(bool bt_lds)
    {
        return bt_lds ? k_filter_sweep<N, KIND, true, OT, PROJ, WANT_LOGC>
                      : k_filter_sweep<N, KIND, false, OT, PROJ, WANT_LOGC>;
    }

    // the sweep, the first dead chunk of every trajectory, the check and the fix-up; *v: failed with boundaries out
    // of tolerance
    template <typename OT>
    static int pass(bhmm_ctx *c, const Model<N> *dm, int W, const double *dBt, const Out &o, plan::Verdict *v)
    {
        unsigned int fails = 0;
        auto &b = c->filt;
        const int G = c->G, groups = c->Gp / 64;
        const Chunks ch = chunks_of(c);
        const size_t lds_bt = (size_t)c->M * score_bt_stride(N) * sizeof(double);
        const bool bt_lds = KIND == EMIT_DISC && lds_bt <= LDS_BT_MAX;
        const bool proj = o.Q > 0 && o.rows != nullptr;
        BHMM_HIP(hipMemsetAsync(b.fails.p, 0, sizeof(unsigned int), c->stream));
        auto *kern = proj ? (o.logc ? kernel<OT, true, true>(bt_lds) : kernel<OT, true, false>(bt_lds))
                          : (o.logc ? kernel<OT, false, true>(bt_lds) : kernel<OT, false, false>(bt_lds));
        BHMM_HIP(launch(kern, dim3(groups), dim3(64), bt_lds ? lds_bt : 0, c->stream, dm, W, ch, G, c->d_obs_ci.p,
                        c->d_obs_rm.p, dBt, c->M, static_cast<OT *>(o.rows), o.V, o.Q, static_cast<OT *>(o.logc),
                        b.aentry.p, b.aexit.p, b.dead.p));
        if (G > 1) { // (one chunk: no boundary, nothing after a dead chunk)
            BHMM_HIP(launch(k_filter_first_dead, dim3(c->K), dim3(64), 0, c->stream, c->d_traj_c0.p, b.dead.p,
                            b.first_dead.p));
            BHMM_HIP(launch(k_filter_check<N>, dim3((G + 255) / 256), dim3(256), 0, c->stream, ch, G, b.aentry.p,
                            b.aexit.p, b.first_dead.p, BOUNDARY_TOL, b.fails.p));
            BHMM_HIP(launch(k_filter_bury<OT>, dim3((G + 255) / 256), dim3(256), 0, c->stream, ch, G, b.first_dead.p,
                            static_cast<OT *>(o.rows), o.Qp, static_cast<OT *>(o.logc)));
        }
        BHMM_HIP(hipMemcpyAsync(&fails, b.fails.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        *v = plan::verdict_of(fails);
        return BHMM_OK;
    }

    // *verified: the results in o stand
    static int run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                   const Out &o, bool *verified)
    {
        auto &b = c->filt;
        *verified = false;
        Model<N> m;
        int rc;
        if ((rc = b.aentry.ensure((size_t)c->Gp * N)) || (rc = b.aexit.ensure((size_t)c->Gp * N)) ||
            (rc = b.dead.ensure(c->Gp)) || (rc = b.first_dead.ensure(std::max(c->K, 1))) || (rc = b.fails.ensure(1)) ||
            (rc = upload_fused_model<N, KIND>(c, b.model, b.Bt, A, pi, par0, par1, m)))
            return rc;
        const Model<N> *dm = reinterpret_cast<const Model<N> *>(b.model.p);
        // the forward reading of the forgetting probe, as bhmm_score takes it
        int W = c->opt.filter_W;
        if (W <= 0 && (rc = fused_probe<N, KIND>(c, b.probe, m, b.Bt.p, false, &W)))
            return rc;
        return plan::two_attempts(
            W, 1 << 30, &c->last.filter_fallbacks,
            [&](int w, plan::Verdict *v) {
                return o.f32 ? pass<float>(c, dm, w, b.Bt.p, o, v) : pass<double>(c, dm, w, b.Bt.p, o, v);
            },
            verified);
    }
};

template <int N>
int run_n(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, const Out &o,
          bool *verified)
{
    return c->kind == EMIT_GAUSS ? Fused<N, EMIT_GAUSS>::run(c, A, pi, par0, par1, o, verified)
                                 : Fused<N, EMIT_DISC>::run(c, A, pi, par0, par1, o, verified);
}

// ---- 9..64 states ------------------------------------------------------------------------------

// the segment plan of filtering on this observation set: made at the first eligible call (and again when
// filter_seglen changes), never after a check.  Not the score plan and not the E-step's
int filter_plan(bhmm_ctx *c)
{
    auto &d = c->ds;
    if (d.filt_nseg > 0 && d.filt_seglen_opt == c->opt.filter_seglen)
        return BHMM_OK;
    int rc, ntiles;
    if ((rc = make_seg_tables(c, c->filt.seg, plan::score_seglen(c->total, c->N, c->num_simd, c->opt.filter_seglen),
                              false, &d.filt_nseg, &d.filt_ntraj, &ntiles)))
        return rc;
    d.filt_seglen_opt = c->opt.filter_seglen;
    return BHMM_OK;
}

struct WideFilt {
    // warm-up: k_wide_probe's forward chains, read as bhmm_score reads them (score_api.hip, Wide::probe) --
    // chains within 1e-13 from then on, times 1.5, rounded up to 8
    static int probe(bhmm_ctx *c, const WideModel &m, int *W)
    {
        *W = W_UNPROBED;
        const int Wmax = plan::probe_wmax_wide(longest_traj(c));
        if (Wmax == 0)
            return BHMM_OK;
        Probe pr;
        int rc;
        if ((rc = probe_stage(c, c->filt.probe, Wmax, 1, pr)) ||
            (rc = filter_wide_probe_launch(c, c->N, m, pr.d_starts, PROBE_P, Wmax, pr.d_curve)))
            return rc;
        std::vector<float> curve; // (the kernel's layout: forward | backward, the latter stays zero)
        if ((rc = probe_read(c, pr, curve)))
            return rc;
        // (not forgotten within Wmax: Wmax, the check decides)
        *W = std::min(plan::warmup_wide_of(plan::curve_last(curve.data(), Wmax, 1e-13f, false)), Wmax);
        return BHMM_OK;
    }

    // the sweep, the first dead segment of every trajectory, the check and the fix-up; *v: failed with boundaries out
    // of tolerance
    static int pass(bhmm_ctx *c, const ScoreWideModel *dm, int W, const Out &o, plan::Verdict *v)
    {
        unsigned int fails = 0;
        auto &b = c->filt;
        const int nseg = c->ds.filt_nseg;
        FilterWideArgs a;
        a.dm = dm;
        a.W = W;
        a.sg = segs_of_tables<Segs>(b.seg, nseg, W);
        a.rows = o.rows;
        a.logc = o.logc;
        a.V = o.V;
        a.Q = o.Q;
        a.f32 = o.f32;
        a.aentry = b.aentry.p;
        a.aexit = b.aexit.p;
        a.dead = b.dead.p;
        int rc;
        if ((rc = filter_wide_launch(c, c->N, a)))
            return rc;
        if (nseg > c->ds.filt_ntraj) { // (no boundary: the exact recursion, nothing after a dead segment)
            const FiltSegs fs{b.seg.seg_traj.p, b.seg.seg_t0.p, b.seg.seg_len.p, c->d_offsets.p, nseg};
            BHMM_HIP(hipMemsetAsync(b.fails.p, 0, sizeof(unsigned int), c->stream));
            BHMM_HIP(launch(k_filter_first_dead, dim3(c->K), dim3(64), 0, c->stream, b.seg.seg_traj0.p, b.dead.p,
                            b.first_dead.p));
            BHMM_HIP(launch(k_filter_seg_check, dim3((nseg + 255) / 256), dim3(256), 0, c->stream, fs, c->n, b.aentry.p,
                            b.aexit.p, b.first_dead.p, BOUNDARY_TOL, b.fails.p));
            if (o.f32)
                BHMM_HIP(launch(k_filter_seg_bury<float>, dim3(nseg), dim3(64), 0, c->stream, fs, b.first_dead.p,
                                static_cast<float *>(o.rows), o.Qp, static_cast<float *>(o.logc)));
            else
                BHMM_HIP(launch(k_filter_seg_bury<double>, dim3(nseg), dim3(64), 0, c->stream, fs, b.first_dead.p,
                                static_cast<double *>(o.rows), o.Qp, static_cast<double *>(o.logc)));
            BHMM_HIP(hipMemcpyAsync(&fails, b.fails.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        }
        BHMM_HIP(hipStreamSynchronize(c->stream));
        *v = plan::verdict_of(fails);
        return BHMM_OK;
    }

    // *verified: the results in o stand
    static int run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                   const Out &o, bool *verified)
    {
        auto &b = c->filt;
        const int M = c->M, n = c->n, K = c->K;
        *verified = false;
        int rc;
        if ((rc = filter_plan(c)))
            return rc;
        const int nseg = c->last.filter_segments = c->ds.filt_nseg;
        const bool segmented = nseg > c->ds.filt_ntraj;
        const bool disc = c->kind == EMIT_DISC;
        const size_t np = wide_block_size(n, M, disc, true);
        if ((rc = b.model.ensure(sizeof(ScoreWideModel))) || (rc = b.wpar.ensure(np)) ||
            (rc = b.aentry.ensure((size_t)std::max(nseg, 1) * n)) || (rc = b.aexit.ensure((size_t)std::max(nseg, 1) * n)) ||
            (rc = b.dead.ensure(std::max(nseg, 1))) || (rc = b.first_dead.ensure(std::max(K, 1))) ||
            (rc = b.fails.ensure(1)))
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
        // a plan without a boundary runs the exact recursion: no probe, no check
        int W = (c->opt.filter_W + 7) / 8 * 8;
        if (segmented && c->opt.filter_W <= 0 && (rc = probe(c, m.w, &W)))
            return rc;
        W = std::max(W, 8);
        return plan::two_attempts(W, 1 << 30, &c->last.filter_fallbacks,
                                  [&](int w, plan::Verdict *v) { return pass(c, dm, w, o, v); }, verified);
    }
};

// the serial path: parallel over trajectories only
// (only: nullptr, or one byte per trajectory on the device -- the marked ones alone)
template <typename OT>
int serial(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, const Out &o,
           const uint8_t *only = nullptr)
{
    const int n = c->n, K = c->K;
    if (n > SCORE_SERIAL_R * 1024)
        return invalid_arg("bhmm_filter: more than 4096 states");
    StackedModels d;
    int rc;
    if ((rc = stage_serial_models(c, c->filt.par, 1, StackedModels(c, A, pi, par0, par1), d)))
        return rc;
    BHMM_HIP(hipStreamSynchronize(c->stream)); // (the caller's arrays may be temporaries)
    if (K == 0)
        return BHMM_OK;
    const int bd = std::min(1024, (n + 63) / 64 * 64);
    const size_t lds = ((size_t)n + 16) * sizeof(double);
    BHMM_HIP(dispatch_kind(c->kind, [&](auto KIND) {
        return launch(k_filter_serial<decltype(KIND)::value, OT>, dim3(K), dim3(bd), lds, c->stream, n, c->M,
                      c->d_offsets.p, c->d_obs_rm.p, d.A, d.pi, d.par0, d.par1, o.V, o.Q, static_cast<OT *>(o.rows),
                      static_cast<OT *>(o.logc), only);
    }));
    return BHMM_OK;
}

// ---- 65..128 states ----------------------------------------------------------------------------

// the segment plan and the tile table of k_filter_tile on this observation set: made at the first eligible call
// (and again when filter_seglen changes), never after a check.  Neither the score plan nor the plan above
int filter_tile_plan(bhmm_ctx *c)
{
    auto &d = c->ds;
    if (d.filt_tile_nseg > 0 && d.filt_tile_seglen_opt == c->opt.filter_seglen)
        return BHMM_OK;
    int rc;
    if ((rc = make_seg_tables(c, c->filt.tseg, plan::score_tile_seglen(c->total, c->num_simd, c->opt.filter_seglen),
                              true, &d.filt_tile_nseg, &d.filt_tile_ntraj, &d.filt_tile_ntiles)))
        return rc;
    d.filt_tile_seglen_opt = c->opt.filter_seglen;
    return BHMM_OK;
}

template <int KIND>
struct TileFilt {
    // what a pass left
    struct Verdict {
        unsigned int fails;  // boundaries out of tolerance (those of trajectories marked for redo are not looked at)
        float dev;           // largest boundary deviation
        unsigned int redone; // trajectories with a segment outside the kernel's range
    };

    // the kernel at warm-up W, the trajectories to do again and the boundary check.  o == nullptr: boundary vectors
    // only (calibration)
    static int pass(bhmm_ctx *c, ScoreTileModel *dm, ScoreTileModel &m, int W, const Out *o, Verdict *v)
    {
        auto &b = c->filt;
        const int n = c->n, nseg = c->ds.filt_tile_nseg;
        m.W = W;
        BHMM_HIP(hipMemcpyAsync(dm, &m, sizeof(ScoreTileModel), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (m changes between passes)
        FilterTileArgs a;
        a.dm = dm;
        a.sg = segs_of_tables<Segs>(b.tseg, nseg, W);
        a.tp = TilePlan{b.tseg.tile_seg.p, c->ds.filt_tile_ntiles};
        a.rows = o ? o->rows : nullptr;
        a.logc = o ? o->logc : nullptr;
        a.V = o ? o->V : nullptr;
        a.Q = o ? o->Q : 0;
        a.f32 = o ? o->f32 : false;
        a.aentry = b.aentry.p;
        a.aexit = b.aexit.p;
        a.seg_flag = b.dead.p;
        BHMM_HIP(hipMemsetAsync(b.fails.p, 0, FILTER_TILE_WORDS * sizeof(unsigned int), c->stream));
        int rc = n <= 80   ? filter_tile_launch<5, KIND>(c, a)
                 : n <= 96  ? filter_tile_launch<6, KIND>(c, a)
                 : n <= 112 ? filter_tile_launch<7, KIND>(c, a)
                            : filter_tile_launch<8, KIND>(c, a);
        if (rc)
            return rc;
        BHMM_HIP(launch(k_filter_tile_redo, dim3(c->K), dim3(64), 0, c->stream, b.tseg.seg_traj0.p, b.dead.p, b.redo.p,
                        b.fails.p));
        if (nseg > c->ds.filt_tile_ntraj) // (no boundary: the exact recursion)
            BHMM_HIP(launch(k_filter_tile_check, dim3((nseg + 15) / 16), dim3(256), 0, c->stream, a.sg, n, b.aentry.p,
                            b.aexit.p, b.redo.p, BOUNDARY_TOL, b.fails.p));
        unsigned int f[FILTER_TILE_WORDS];
        BHMM_HIP(hipMemcpyAsync(f, b.fails.p, sizeof(f), hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        v->fails = f[FILTER_TILE_FAILS];
        memcpy(&v->dev, &f[FILTER_TILE_DEV], sizeof(float));
        v->redone = f[FILTER_TILE_REDONE];
        return BHMM_OK;
    }

    // warm-up by the rule of bhmm_score's Tile::calibrate (score_api.hip): the kernel itself, without outputs, at
    // two warm-ups; the largest boundary deviation of each; the decay between them extrapolated
    static int calibrate(bhmm_ctx *c, ScoreTileModel *dm, ScoreTileModel &m, int *W)
    {
        auto good = [](const Verdict &v) { return v.fails == 0 && (double)v.dev <= SCORE_TILE_DEV_OK; };
        Verdict v0, v1;
        int rc;
        *W = SCORE_TILE_W0;
        if ((rc = pass(c, dm, m, SCORE_TILE_W0, nullptr, &v0)) || good(v0))
            return rc;
        if ((rc = pass(c, dm, m, SCORE_TILE_W1, nullptr, &v1)))
            return rc;
        *W = good(v1) ? SCORE_TILE_W1 : score_tile_extrapolate((double)v0.dev, (double)v1.dev);
        return BHMM_OK;
    }

    // *verified: the results in o stand
    static int run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                   const Out &o, bool *verified)
    {
        auto &b = c->filt;
        const int M = c->M, n = c->n, K = c->K;
        *verified = false;
        int rc;
        if ((rc = filter_tile_plan(c)))
            return rc;
        const int nseg = c->last.filter_segments = c->ds.filt_tile_nseg;
        const bool segmented = nseg > c->ds.filt_tile_ntraj;
        constexpr bool disc = KIND == EMIT_DISC;
        const size_t np = wide_block_size(n, M, disc, false); // (the kernel reads B^T)
        if ((rc = b.model.ensure(sizeof(ScoreTileModel))) || (rc = b.wpar.ensure(np)) ||
            (rc = b.aentry.ensure((size_t)std::max(nseg, 1) * n)) || (rc = b.aexit.ensure((size_t)std::max(nseg, 1) * n)) ||
            (rc = b.dead.ensure(std::max(nseg, 1))) || (rc = b.redo.ensure(std::max(K, 1))) ||
            (rc = b.fails.ensure(FILTER_TILE_WORDS)))
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
        // W: multiples of four (the refresh of the scaling).  A plan without a boundary runs the exact recursion: no
        // calibration, no check
        int W = segmented ? (c->opt.filter_W + 3) & ~3 : 0;
        if (segmented && c->opt.filter_W <= 0 && (rc = calibrate(c, dm, m, &W)))
            return rc;
        return plan::two_attempts(
            W, SCORE_TILE_W_MAX, &c->last.filter_fallbacks,
            [&](int w, plan::Verdict *pv) {
                Verdict v;
                int rc2;
                if ((rc2 = pass(c, dm, m, w, &o, &v)) || (*pv = plan::verdict_of(v.fails)) != plan::Verdict::verified)
                    return rc2;
                // the trajectories with a segment outside the kernel's range again, whole, on the serial kernel:
                // behind the pass, on the same stream
                c->last.filter_redone = (int)v.redone;
                if (v.redone == 0)
                    return BHMM_OK;
                return o.f32 ? serial<float>(c, A, pi, par0, par1, o, b.redo.p)
                             : serial<double>(c, A, pi, par0, par1, o, b.redo.p);
            },
            verified);
    }
};

// a staged result to the caller's host buffer in one copy
int deliver(bhmm_ctx *c, void *host, const void *dev, size_t bytes)
{
    return bytes == 0 ? BHMM_OK : copy_to_host_pinned(c, host, dev, bytes);
}

} // namespace
} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_filter(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                const double *V, int Q, void *rows, void *logc, int flags)
{
    int rc = enter_model_call(c, A && pi && (rows || logc), "A / pi == NULL, or rows and logc both NULL", true, par0,
                              par1);
    if (rc)
        return rc;
    if (flags & ~(BHMM_FILT_F32 | BHMM_FILT_DEVICE))
        return invalid_arg("bhmm_filter: unknown flag");
    if ((V == nullptr) != (Q == 0) || Q < 0 || Q > MARG_QMAX)
        return invalid_arg("bhmm_filter: V with 1 <= Q <= 8 columns, or V == NULL and Q == 0");
    const bool on_dev = (flags & BHMM_FILT_DEVICE) != 0;
    if (on_dev && ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(logc)) & 15))
        return invalid_arg("bhmm_filter: a device buffer must be aligned to 16 bytes");
    for (int e = 0; e < c->n * Q; ++e)
        if (!std::isfinite(V[e]))
            return invalid_arg("bhmm_filter: V has a non-finite entry");
    if ((rc = check_models(c, "bhmm_filter", 1, A, pi, par0, par1)))
        return rc;
    auto &b = c->filt;
    Out o;
    o.f32 = (flags & BHMM_FILT_F32) != 0;
    o.Q = Q;
    o.Qp = Q > 0 ? Q : c->n;
    o.V = nullptr;
    const size_t esz = o.f32 ? sizeof(float) : sizeof(double);
    const size_t rows_bytes = rows ? (size_t)c->total * o.Qp * esz : 0, logc_bytes = logc ? (size_t)c->total * esz : 0;
    if (!on_dev) { // (BHMM_ERR_NO_MEM: nothing is truncated)
        if (rows && (rc = b.rows.ensure(std::max<size_t>(rows_bytes, 16))))
            return rc;
        if (logc && (rc = b.logc.ensure(std::max<size_t>(logc_bytes, 16))))
            return rc;
    }
    o.rows = !rows ? nullptr : (on_dev ? rows : static_cast<void *>(b.rows.p));
    o.logc = !logc ? nullptr : (on_dev ? logc : static_cast<void *>(b.logc.p));
    if (Q > 0 && rows) {
        if ((rc = b.V.ensure((size_t)c->n * Q)))
            return rc;
        BHMM_HIP(hipMemcpyAsync(b.V.p, V, (size_t)c->n * Q * sizeof(double), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (V may be a temporary of the caller's)
        o.V = b.V.p;
    }
    const bool emis = c->kind == EMIT_GAUSS || c->kind == EMIT_DISC;
    const bool fused = fused_takes(c);
    // 9..64 states (lanes per segment in c->N): always, never, or from FILTER_WIDE_MIN_TOTAL steps on
    const bool wide = c->wide && emis && c->n <= 64 && c->opt.filter_parallel != 0 &&
                      (c->opt.filter_parallel == 1 || c->total >= FILTER_WIDE_MIN_TOTAL);
    // 65..128 states on loaded observations (as bhmm_score decides): always, never, or from FILTER_TILE_MIN_TOTAL
    // steps on
    const bool tile = c->gen && c->n <= 128 && emis && c->opt.filter_parallel != 0 && c->opt.filter_tile != 0 &&
                      (c->opt.filter_tile == 1 || c->total >= FILTER_TILE_MIN_TOTAL);
    c->last.filter_path = fused ? 1 : (wide ? 2 : (tile ? 3 : 0));
    c->last.filter_segments = 0;
    c->last.filter_redone = 0;
    bool verified = false;
    if (tile) {
        if ((rc = c->kind == EMIT_GAUSS ? TileFilt<EMIT_GAUSS>::run(c, A, pi, par0, par1, o, &verified)
                                        : TileFilt<EMIT_DISC>::run(c, A, pi, par0, par1, o, &verified)))
            return rc;
    } else if (wide) {
        if ((rc = WideFilt::run(c, A, pi, par0, par1, o, &verified)))
            return rc;
    } else if (fused) {
        rc = dispatch_n(c->n, [&](auto N) { return run_n<decltype(N)::value>(c, A, pi, par0, par1, o, &verified); });
        if (rc)
            return rc;
    }
    if (!verified && (rc = o.f32 ? serial<float>(c, A, pi, par0, par1, o) : serial<double>(c, A, pi, par0, par1, o)))
        return rc;
    if (on_dev) // the results are where the caller wants them, ordered on the context's stream
        return BHMM_OK;
    if (rows && (rc = deliver(c, rows, o.rows, rows_bytes)))
        return rc;
    if (logc && (rc = deliver(c, logc, o.logc, logc_bytes)))
        return rc;
    BHMM_HIP(hipStreamSynchronize(c->stream)); // (synchronous also when there was nothing to copy)
    return BHMM_OK;
}

} // extern "C"
