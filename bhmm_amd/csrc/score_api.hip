// score_api.hip -- bhmm_score: log-likelihood of every loaded trajectory under each of several models
// (forward pass only).  Kernels in score_kernels.hpp; DESIGN.md section 13.
//
// Up to 8 states, gaussian or discrete: k_score_fwd over the E-step's chunk plan, all models of a batch
// (at most SCORE_MAX_MODELS) in one launch, then k_score_check and k_score_logl.  Every model has a
// warm-up of its own (the forgetting probe of the E-step, k_forget_probe, or the option score_W), so
// its result does not depend on the other models of the call.  A model whose boundaries do not verify
// runs again alone with twice the warm-up; if they fail again it takes the exact serial recursion
// (k_score_serial).
//
// 9 to 64 states, gaussian or discrete: k_score_wide (score_wide_kernels.hpp) over a segment plan that belongs
// to scoring alone (score_plan: a function of the offsets, the state count and the device; option
// score_seglen; tables in c->score.seg), all models of a batch in one launch, then k_score_wide_check and k_score_logl.  W per model
// from k_wide_probe (or score_W); the same protocol: a failed model runs again alone with twice the warm-up,
// on the kernel that sums every step, then takes the exact serial recursion.
//
// 65 to 128 states, gaussian or discrete: k_score_tile (score_tile_kernels.hpp) on the fp64 matrix cores, sixteen
// segments per workgroup, over a segment plan and a tile table that again belong to scoring alone
// (score_plan with tiles; plan::score_tile_seglen, option score_seglen).  W per model from two passes of the kernel
// itself (tile_calibrate) or the option score_W; the protocol is the same, but a model that left the number range
// of the lazily scaled kernel goes straight to the exact serial recursion (there is no tile kernel that sums
// every step).
//
// Explicit pobs and more than 128 states always take the exact path.
//
// The three paths run the protocol per model through one loop (retry_alone) over one view of the caller's stacked
// arrays (StackedModels).  What they share with bhmm_filter and the posterior calls is in plan.hpp (arithmetic, the
// doubling of a warm-up), seg_host.hpp (device side) and fused_host.hpp (up to 8 states): the constants of the
// protocol, the probe's sample positions, staging and reading, the padded B^T and the warm-up of the fused path
// (fill_Bt_padded, fused_probe_models), the parameter block of a WideModel (fill_wide_block), the making of a plan's
// tables (make_seg_tables) and the staging of the serial recursion's parameters (stage_serial_models).
//
// Nothing here reads or writes the E-step's state (ds.* but the score plan's own fields, carried vectors,
// warm-up lengths, d_Bt, the E-step's segment plans, the timing events, the pinned landing zones): the
// buffers are c->score.*, the only other fields touched are opt.score_* (read) and last.score_*.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "fused_host.hpp"
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "model_check.hpp"
#include "plan.hpp"
#include "score_kernels.hpp"
#include "score_wide_kernels.hpp"
#include "score_tile_launch.hpp"
#include "seg_host.hpp"

namespace bhmm {

SCORE_TILE_LAUNCH_DECL(extern, 5)
SCORE_TILE_LAUNCH_DECL(extern, 6)
SCORE_TILE_LAUNCH_DECL(extern, 7)
SCORE_TILE_LAUNCH_DECL(extern, 8)

namespace {

// (BOUNDARY_TOL, W_UNPROBED, LDS_BT_MAX, the probe and the plan: seg_host.hpp, shared with bhmm_filter and the
// posterior calls)

// per (trajectory, model) log-likelihood on the exact serial recursion for models [0, S) of the stacked
// arrays; out[s * K + k]
int score_serial(bhmm_ctx *c, int S, const StackedModels &h, double *out)
{
    const int n = c->n, K = c->K;
    const int bd = std::min(1024, (n + 63) / 64 * 64);
    const size_t lds = ((size_t)n + 16) * sizeof(double);
    auto &b = c->score;
    int rc;
    for (int s0 = 0; s0 < S; s0 += SCORE_MAX_MODELS) {
        const int Sb = std::min(SCORE_MAX_MODELS, S - s0);
        StackedModels d;
        if ((rc = b.logLk.ensure((size_t)Sb * K)) || (rc = stage_serial_models(c, b.par, Sb, h.at(s0), d)))
            return rc;
        BHMM_HIP(dispatch_kind(c->kind, [&](auto KIND) {
            return launch(k_score_serial<decltype(KIND)::value>, dim3(K, Sb), dim3(bd), lds, c->stream, n, c->M, K,
                          c->d_offsets.p, c->d_obs_rm.p, d.A, d.pi, d.par0, d.par1, b.logLk.p);
        }));
        BHMM_HIP(hipMemcpyAsync(out + (size_t)s0 * K, b.logLk.p, (size_t)Sb * K * sizeof(double),
                                hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (the parameter buffer is reused by the next batch)
    }
    return BHMM_OK;
}

// models per launch: at most SCORE_MAX_MODELS, and boundary vectors (`rows` chunks or segments of n states, entry and
// exit, and a log-normaliser each) of at most 1 GiB
int models_per_launch(int rows, int n)
{
    const size_t per_model = (size_t)std::max(rows, 1) * (2 * n + 1) * sizeof(double);
    return (int)std::max<size_t>(1, std::min<size_t>(SCORE_MAX_MODELS, ((size_t)1 << 30) / per_model));
}

// The protocol per model of a batch (h, out: the batch's models and results): a model whose first pass left
// boundaries that did not verify (first(s): failed) counts one fallback and runs again alone, second(s, &v), with
// twice the warm-up; one that fails again, or that left the kernel's number range (abandon), takes the exact serial
// recursion
template <class First, class Second>
int retry_alone(bhmm_ctx *c, int Sb, const StackedModels &h, double *out, First first, Second second)
{
    int rc;
    for (int s = 0; s < Sb; ++s) {
        plan::Verdict v = first(s);
        if (v == plan::Verdict::failed) {
            ++c->last.score_fallbacks;
            if ((rc = second(s, &v)))
                return rc;
        }
        if (v != plan::Verdict::verified && (rc = score_serial(c, 1, h.at(s), out + (size_t)s * c->K)))
            return rc;
    }
    return BHMM_OK;
}

// N: the kernel's state count (the real one for the lane-per-chunk layout, 2 / 4 / 8 padded for PAIR)
template <int N, int KIND, bool PAIR>
struct Fast {
    // one launch sequence for models [0, Sb) of the tables on the device; logLk and the failure counters to the host
    static int pass(bhmm_ctx *c, int Sb, const Model<N> *dm, const int32_t *dW, const double *dBt, double *logLk_h,
                    unsigned int *fails_h)
    {
        auto &b = c->score;
        const int K = c->K, G = c->G, Gp = c->Gp;
        const Chunks ch = chunks_of(c);
        const size_t lds_bt = (size_t)c->M * score_bt_stride(N) * sizeof(double);
        const bool bt_lds = KIND == EMIT_DISC && lds_bt <= LDS_BT_MAX;
        BHMM_HIP(hipMemsetAsync(b.fails.p, 0, Sb * sizeof(unsigned int), c->stream));
        const dim3 grid(Gp / 64, Sb);
        const dim3 block(PAIR ? 32 * N : 64);
        auto kern = [&]() {
            if constexpr (PAIR)
                return bt_lds ? k_score_pair<N, KIND, true> : k_score_pair<N, KIND, false>;
            else
                return bt_lds ? k_score_fwd<N, KIND, true> : k_score_fwd<N, KIND, false>;
        }();
        BHMM_HIP(launch(kern, grid, block, bt_lds ? lds_bt : 0, c->stream, dm, dW, ch, G, Gp, c->d_obs_ci.p,
                        c->d_obs_rm.p, dBt, c->M, b.logLc.p, b.aentry.p, b.aexit.p));
        if (G > 1)
            BHMM_HIP(launch(k_score_check<N>, dim3((G + 255) / 256, Sb), dim3(256), 0, c->stream, ch, G, Gp, b.logLc.p,
                            b.aentry.p, b.aexit.p, BOUNDARY_TOL, b.fails.p));
        BHMM_HIP(launch(k_score_logl, dim3(K, Sb), dim3(64), 0, c->stream, c->d_traj_c0.p, K, Gp, b.logLc.p,
                        b.logLk.p));
        BHMM_HIP(hipMemcpyAsync(fails_h, b.fails.p, Sb * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipMemcpyAsync(logLk_h, b.logLk.p, (size_t)Sb * K * sizeof(double), hipMemcpyDeviceToHost,
                                c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        return BHMM_OK;
    }

    static int run(bhmm_ctx *c, int S, const StackedModels &h, double *logL)
    {
        auto &b = c->score;
        const int K = c->K, M = c->M, n = c->n;
        const int Sb_max = models_per_launch(c->Gp, N);
        int rc;
        if ((rc = b.logLc.ensure((size_t)Sb_max * c->Gp)) || (rc = b.aentry.ensure((size_t)Sb_max * c->Gp * N)) ||
            (rc = b.aexit.ensure((size_t)Sb_max * c->Gp * N)) || (rc = b.logLk.ensure((size_t)Sb_max * K)) ||
            (rc = b.fails.ensure(Sb_max)) || (rc = b.W.ensure(Sb_max)) ||
            (rc = b.models.ensure((size_t)Sb_max * sizeof(Model<N>))) ||
            (KIND == EMIT_DISC && (rc = b.Bt.ensure((size_t)Sb_max * M * N))))
            return rc;
        Model<N> *dm = reinterpret_cast<Model<N> *>(b.models.p);
        std::vector<unsigned int> fails(Sb_max);
        for (int s0 = 0; s0 < S; s0 += Sb_max) {
            const int Sb = std::min(Sb_max, S - s0);
            std::vector<Model<N>> m(Sb);
            std::vector<double> bt(KIND == EMIT_DISC ? (size_t)Sb * M * N : 0, 0.0); // (padded states: zero)
            for (int s = 0; s < Sb; ++s) {
                const StackedModels g = h.at(s0 + s);
                fill_model<N>(m[s], n, KIND, M, g.A, g.pi, g.par0, g.par1);
                if (KIND == EMIT_DISC)
                    fill_Bt_padded(n, N, M, g.par0, bt.data() + (size_t)s * M * N);
            }
            if (KIND == EMIT_DISC) {
                BHMM_HIP(hipMemcpyAsync(b.Bt.p, bt.data(), bt.size() * sizeof(double), hipMemcpyHostToDevice,
                                        c->stream));
                BHMM_HIP(hipStreamSynchronize(c->stream));
            }
            BHMM_HIP(hipMemcpyAsync(dm, m.data(), Sb * sizeof(Model<N>), hipMemcpyHostToDevice, c->stream));
            // every model has a warm-up of its own: the forward reading of its forgetting curve
            std::vector<int> W(Sb, c->opt.score_W);
            if (c->opt.score_W <= 0 &&
                (rc = fused_probe_models<N, KIND>(c, b.probe, Sb, m.data(), b.Bt.p, false, W.data())))
                return rc;
            BHMM_HIP(hipMemcpyAsync(b.W.p, W.data(), Sb * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            double *out = logL + (size_t)s0 * K;
            if ((rc = pass(c, Sb, dm, b.W.p, b.Bt.p, out, fails.data())) ||
                (rc = retry_alone(
                     c, Sb, h.at(s0), out, [&](int s) { return plan::verdict_of(fails[s]); },
                     [&](int s, plan::Verdict *v) {
                         const int W2 = plan::doubled(W[s], 1 << 30);
                         BHMM_HIP(hipMemcpyAsync(b.W.p + s, &W2, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
                         unsigned int f2 = 0;
                         const int rc2 = pass(c, 1, dm + s, b.W.p + s,
                                              KIND == EMIT_DISC ? b.Bt.p + (size_t)s * M * N : nullptr,
                                              out + (size_t)s * K, &f2);
                         *v = plan::verdict_of(f2);
                         return rc2;
                     })))
                return rc;
        }
        return BHMM_OK;
    }
};

template <int N, bool PAIR>
int run_n(bhmm_ctx *c, int S, const StackedModels &h, double *logL)
{
    return c->kind == EMIT_GAUSS ? Fast<N, EMIT_GAUSS, PAIR>::run(c, S, h, logL)
                                 : Fast<N, EMIT_DISC, PAIR>::run(c, S, h, logL);
}

// ---- 9..128 states: the plan ----------------------------------------------------------------------

// the segment plan of scoring on this observation set: made once (and again when score_seglen changes),
// never after a check.  tiles: 65..128 states, plan::score_tile_seglen and the tile table of k_score_tile
int score_plan(bhmm_ctx *c, bool tiles)
{
    auto &d = c->ds;
    if (d.score_nseg > 0 && d.score_seglen_opt == c->opt.score_seglen)
        return BHMM_OK;
    const int64_t seglen = tiles ? plan::score_tile_seglen(c->total, c->num_simd, c->opt.score_seglen)
                                 : plan::score_seglen(c->total, c->N, c->num_simd, c->opt.score_seglen);
    int rc;
    if ((rc = make_seg_tables(c, c->score.seg, seglen, tiles, &d.score_nseg, &d.score_ntraj, &d.score_ntiles)))
        return rc;
    d.score_seglen_opt = c->opt.score_seglen;
    return BHMM_OK;
}

// ---- 9..64 states ------------------------------------------------------------------------------

template <int NP, int KIND>
struct Wide {
    static constexpr int GP = 64 / NP;

    // warm-up of every model of the batch: k_wide_probe once per model (its forward chains only: the first
    // PROBE_P / GP workgroups), read like wide_probe_run (plan::warmup_wide_of) -- chains within 1e-13 from then on,
    // times 1.5 -- and capped at the longest warm-up the probe measures
    static int probe(bhmm_ctx *c, int Sb, const std::vector<ScoreWideModel> &m, std::vector<int> &W)
    {
        W.assign(Sb, W_UNPROBED);
        const int Wmax = plan::probe_wmax_wide(longest_traj(c));
        if (Wmax == 0)
            return BHMM_OK;
        Probe pr;
        int rc;
        if ((rc = probe_stage(c, c->score.probe, Wmax, Sb, pr)))
            return rc;
        const size_t curve_words = 2 * (size_t)Wmax; // (the kernel's layout: forward | backward, the latter stays zero)
        for (int s = 0; s < Sb; ++s)
            BHMM_HIP(launch(k_wide_probe<NP, KIND>, dim3(PROBE_P / GP), dim3(64), 0, c->stream, m[s].w, c->d_obs_rm.p,
                            pr.d_starts, PROBE_P, Wmax, pr.d_curve + s * curve_words));
        std::vector<float> curve;
        if ((rc = probe_read(c, pr, curve)))
            return rc;
        for (int s = 0; s < Sb; ++s) // (not forgotten within Wmax: Wmax, the check decides)
            W[s] = std::min(plan::warmup_wide_of(plan::curve_last(curve.data() + s * curve_words, Wmax, 1e-13f, false)),
                            Wmax);
        return BHMM_OK;
    }

    // one launch sequence for models [0, Sb) of the tables on the device
    static int pass(bhmm_ctx *c, int Sb, const ScoreWideModel *dm, const int32_t *dW, bool lazy, double *logLk_h,
                    unsigned int *fails_h)
    {
        auto &b = c->score;
        const int K = c->K, nseg = c->ds.score_nseg;
        const Segs sg = segs_of_tables<Segs>(b.seg, nseg, 0); // (W per model: dW)
        const size_t lds_bt = (size_t)c->M * NP * sizeof(double);
        const bool bt_lds = KIND == EMIT_DISC && lds_bt <= LDS_BT_MAX;
        BHMM_HIP(hipMemsetAsync(b.fails.p, 0, Sb * sizeof(unsigned int), c->stream));
        constexpr bool D = KIND == EMIT_DISC; // (gaussian: one instantiation per scaling)
        auto *kern = lazy ? (bt_lds ? k_score_wide<NP, KIND, true, D> : k_score_wide<NP, KIND, true, false>)
                          : (bt_lds ? k_score_wide<NP, KIND, false, D> : k_score_wide<NP, KIND, false, false>);
        BHMM_HIP(launch(kern, dim3((nseg + GP - 1) / GP, Sb), dim3(64), bt_lds ? lds_bt : 0, c->stream, dm, dW,
                        c->d_offsets.p, sg, c->d_obs_rm.p, b.logLc.p, b.aentry.p, b.aexit.p, b.fails.p));
        if (nseg > c->ds.score_ntraj)
            BHMM_HIP(launch(k_score_wide_check, dim3((nseg + 15) / 16, Sb), dim3(256), 0, c->stream, sg, c->n,
                            b.logLc.p, b.aentry.p, b.aexit.p, BOUNDARY_TOL, b.fails.p));
        BHMM_HIP(launch(k_score_logl, dim3(K, Sb), dim3(64), 0, c->stream, b.seg.seg_traj0.p, K, nseg, b.logLc.p,
                        b.logLk.p));
        BHMM_HIP(hipMemcpyAsync(fails_h, b.fails.p, Sb * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipMemcpyAsync(logLk_h, b.logLk.p, (size_t)Sb * K * sizeof(double), hipMemcpyDeviceToHost,
                                c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        return BHMM_OK;
    }

    static int run(bhmm_ctx *c, int S, const StackedModels &h, double *logL)
    {
        auto &b = c->score;
        const int K = c->K, M = c->M, n = c->n;
        int rc;
        if ((rc = score_plan(c, false)))
            return rc;
        const int nseg = c->last.score_segments = c->ds.score_nseg;
        const int Sb_max = models_per_launch(nseg, n);
        constexpr bool disc = KIND == EMIT_DISC;
        const size_t np = wide_block_size(n, M, disc, true);
        if ((rc = b.logLc.ensure((size_t)Sb_max * nseg)) || (rc = b.aentry.ensure((size_t)Sb_max * nseg * n)) ||
            (rc = b.aexit.ensure((size_t)Sb_max * nseg * n)) || (rc = b.logLk.ensure((size_t)Sb_max * K)) ||
            (rc = b.fails.ensure(Sb_max)) || (rc = b.W.ensure(Sb_max)) ||
            (rc = b.models.ensure((size_t)Sb_max * sizeof(ScoreWideModel))) || (rc = b.wpar.ensure(Sb_max * np)))
            return rc;
        ScoreWideModel *dm = reinterpret_cast<ScoreWideModel *>(b.models.p);
        std::vector<unsigned int> fails(Sb_max);
        for (int s0 = 0; s0 < S; s0 += Sb_max) {
            const int Sb = std::min(Sb_max, S - s0);
            std::vector<double> hp(Sb * np, 0.0);
            std::vector<ScoreWideModel> m(Sb);
            for (int s = 0; s < Sb; ++s) {
                const StackedModels g = h.at(s0 + s);
                m[s].Bt = fill_wide_block(n, M, disc, true, g.A, g.pi, g.par0, g.par1, hp.data() + s * np,
                                          b.wpar.p + s * np, m[s].w);
            }
            BHMM_HIP(hipMemcpyAsync(b.wpar.p, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
            BHMM_HIP(hipMemcpyAsync(dm, m.data(), Sb * sizeof(ScoreWideModel), hipMemcpyHostToDevice, c->stream));
            BHMM_HIP(hipStreamSynchronize(c->stream)); // (hp and m are temporaries; the probe takes m by value)
            // W: multiples of four (the lazy refresh); no boundary at all, no warm-up to measure
            std::vector<int> W(Sb, (c->opt.score_W + 3) & ~3);
            if (c->opt.score_W <= 0 && nseg > c->ds.score_ntraj && (rc = probe(c, Sb, m, W)))
                return rc;
            if (nseg > c->ds.score_ntraj)
                c->last.score_W_max = std::max(c->last.score_W_max, *std::max_element(W.begin(), W.end()));
            BHMM_HIP(hipMemcpyAsync(b.W.p, W.data(), Sb * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            double *out = logL + (size_t)s0 * K;
            // (a vector outside the lazy kernel's range counts as a boundary that did not verify: the second pass is
            // the kernel that sums every step)
            if ((rc = pass(c, Sb, dm, b.W.p, c->opt.score_lazy, out, fails.data())) ||
                (rc = retry_alone(
                     c, Sb, h.at(s0), out, [&](int s) { return plan::verdict_of(fails[s]); },
                     [&](int s, plan::Verdict *v) {
                         const int W2 = plan::doubled(W[s], 1 << 30);
                         BHMM_HIP(hipMemcpyAsync(b.W.p + s, &W2, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
                         unsigned int f2 = 0;
                         const int rc2 = pass(c, 1, dm + s, b.W.p + s, false, out + (size_t)s * K, &f2);
                         *v = plan::verdict_of(f2);
                         return rc2;
                     })))
                return rc;
        }
        return BHMM_OK;
    }
};

template <int NP>
int run_wide(bhmm_ctx *c, int S, const StackedModels &h, double *logL)
{
    return c->kind == EMIT_GAUSS ? Wide<NP, EMIT_GAUSS>::run(c, S, h, logL) : Wide<NP, EMIT_DISC>::run(c, S, h, logL);
}

// ---- 65..128 states ----------------------------------------------------------------------------

// (SCORE_TILE_W0 .. SCORE_TILE_W_MAX, the constants of the calibration: host_internal.hpp, shared with bhmm_filter)

template <int KIND>
struct Tile {
    // what a pass left per model
    struct Verdict {
        unsigned int range, fails; // rows outside the lazy scaling's range; boundaries that did not verify
        float dev;                 // largest boundary deviation
    };

    // one launch sequence for models [0, Sb) of the table on the device.  logLk_h == nullptr: boundary vectors and
    // their check only (calibration)
    static int pass(bhmm_ctx *c, int Sb, const ScoreTileModel *dm, double *logLk_h, Verdict *v)
    {
        auto &b = c->score;
        const int K = c->K, nseg = c->ds.score_nseg, n = c->n;
        const Segs sg = segs_of_tables<Segs>(b.seg, nseg, 0); // (W per model: in its table entry)
        const TilePlan tp{b.seg.tile_seg.p, c->ds.score_ntiles};
        BHMM_HIP(hipMemsetAsync(b.fails.p, 0, (size_t)Sb * SCORE_TILE_FLAGS * sizeof(unsigned int), c->stream));
        int rc = n <= 80   ? score_tile_launch<5, KIND>(c, Sb, dm, sg, tp, b.fails.p)
                 : n <= 96  ? score_tile_launch<6, KIND>(c, Sb, dm, sg, tp, b.fails.p)
                 : n <= 112 ? score_tile_launch<7, KIND>(c, Sb, dm, sg, tp, b.fails.p)
                            : score_tile_launch<8, KIND>(c, Sb, dm, sg, tp, b.fails.p);
        if (rc)
            return rc;
        if (nseg > c->ds.score_ntraj)
            BHMM_HIP(launch(k_score_tile_check, dim3((nseg + 15) / 16, Sb), dim3(256), 0, c->stream, sg, n, b.aentry.p,
                            b.aexit.p, BOUNDARY_TOL, b.fails.p));
        if (logLk_h)
            BHMM_HIP(launch(k_score_logl, dim3(K, Sb), dim3(64), 0, c->stream, b.seg.seg_traj0.p, K, nseg, b.logLc.p,
                            b.logLk.p));
        std::vector<unsigned int> f((size_t)Sb * SCORE_TILE_FLAGS);
        BHMM_HIP(hipMemcpyAsync(f.data(), b.fails.p, f.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        if (logLk_h)
            BHMM_HIP(hipMemcpyAsync(logLk_h, b.logLk.p, (size_t)Sb * K * sizeof(double), hipMemcpyDeviceToHost,
                                    c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        for (int s = 0; s < Sb; ++s) {
            v[s].range = f[SCORE_TILE_FLAGS * s];
            v[s].fails = f[SCORE_TILE_FLAGS * s + 1];
            memcpy(&v[s].dev, &f[SCORE_TILE_FLAGS * s + 2], sizeof(float));
        }
        return BHMM_OK;
    }

    static int upload(bhmm_ctx *c, int Sb, ScoreTileModel *dm, std::vector<ScoreTileModel> &m, const std::vector<int> &W)
    {
        for (int s = 0; s < Sb; ++s)
            m[s].W = W[s];
        BHMM_HIP(hipMemcpyAsync(dm, m.data(), Sb * sizeof(ScoreTileModel), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (m changes between passes)
        return BHMM_OK;
    }

    // Warm-up of every model of the batch, the way tile_gen.hip calibrates the E-step's: the kernel itself at two
    // warm-ups, the largest boundary deviation of each, and the geometric decay between the two (the filter
    // forgets its start vector) extrapolated to 1e-13, times SCORE_TILE_MARGIN (score_tile_extrapolate in
    // host_internal.hpp).  A function of the model, the observation set and the plan: every model is measured on
    // its own counters.
    static int calibrate(bhmm_ctx *c, int Sb, ScoreTileModel *dm, std::vector<ScoreTileModel> &m, std::vector<int> &W)
    {
        std::vector<Verdict> v0(Sb), v1(Sb);
        int rc;
        W.assign(Sb, SCORE_TILE_W0);
        if ((rc = upload(c, Sb, dm, m, W)) || (rc = pass(c, Sb, dm, nullptr, v0.data())))
            return rc;
        auto good = [](const Verdict &v) { return v.fails == 0 && (double)v.dev <= SCORE_TILE_DEV_OK; };
        bool all = true;
        for (int s = 0; s < Sb; ++s)
            all = all && (good(v0[s]) || v0[s].range != 0);
        if (all)
            return BHMM_OK;
        std::vector<int> W1(Sb, SCORE_TILE_W1);
        if ((rc = upload(c, Sb, dm, m, W1)) || (rc = pass(c, Sb, dm, nullptr, v1.data())))
            return rc;
        for (int s = 0; s < Sb; ++s) {
            if (good(v0[s]) || v0[s].range != 0)
                continue; // (outside the range: the pass that follows sends the model to the serial recursion)
            W[s] = good(v1[s]) ? SCORE_TILE_W1 : score_tile_extrapolate((double)v0[s].dev, (double)v1[s].dev);
        }
        return BHMM_OK;
    }

    static int run(bhmm_ctx *c, int S, const StackedModels &h, double *logL)
    {
        auto &b = c->score;
        const int K = c->K, M = c->M, n = c->n;
        int rc;
        if ((rc = score_plan(c, true)))
            return rc;
        if (c->ds.score_ntiles == 0) // (no trajectory has a step)
            return score_serial(c, S, h, logL);
        const int nseg = c->last.score_segments = c->ds.score_nseg;
        const bool segmented = nseg > c->ds.score_ntraj;
        const int Sb_max = models_per_launch(nseg, n);
        constexpr bool disc = KIND == EMIT_DISC;
        const size_t np = wide_block_size(n, M, disc, false); // (the kernel reads B^T)
        if ((rc = b.logLc.ensure((size_t)Sb_max * nseg)) || (rc = b.aentry.ensure((size_t)Sb_max * nseg * n)) ||
            (rc = b.aexit.ensure((size_t)Sb_max * nseg * n)) || (rc = b.logLk.ensure((size_t)Sb_max * K)) ||
            (rc = b.fails.ensure((size_t)Sb_max * SCORE_TILE_FLAGS)) ||
            (rc = b.models.ensure((size_t)Sb_max * sizeof(ScoreTileModel))) || (rc = b.wpar.ensure(Sb_max * np)))
            return rc;
        ScoreTileModel *dm = reinterpret_cast<ScoreTileModel *>(b.models.p);
        std::vector<Verdict> v(Sb_max);
        for (int s0 = 0; s0 < S; s0 += Sb_max) {
            const int Sb = std::min(Sb_max, S - s0);
            std::vector<double> hp(Sb * np, 0.0);
            std::vector<ScoreTileModel> m(Sb);
            for (int s = 0; s < Sb; ++s) {
                const StackedModels g = h.at(s0 + s);
                m[s].Bt = fill_wide_block(n, M, disc, false, g.A, g.pi, g.par0, g.par1, hp.data() + s * np,
                                          b.wpar.p + s * np, m[s].w);
                m[s].W = 0;
            }
            BHMM_HIP(hipMemcpyAsync(b.wpar.p, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
            BHMM_HIP(hipStreamSynchronize(c->stream)); // (hp is a temporary)
            // W: multiples of four (the refresh of the scaling); no boundary at all, no warm-up to measure
            std::vector<int> W(Sb, segmented ? (c->opt.score_W + 3) & ~3 : 0);
            if (segmented && c->opt.score_W <= 0 && (rc = calibrate(c, Sb, dm, m, W)))
                return rc;
            if (segmented)
                c->last.score_W_max = std::max(c->last.score_W_max, *std::max_element(W.begin(), W.end()));
            double *out = logL + (size_t)s0 * K;
            // (outside the lazy scaling's range: the exact recursion at once -- there is no tile kernel that sums every
            // step)
            auto verdict = [](const Verdict &r) { return r.range != 0 ? plan::Verdict::abandon : plan::verdict_of(r.fails); };
            if ((rc = upload(c, Sb, dm, m, W)) || (rc = pass(c, Sb, dm, out, v.data())) ||
                (rc = retry_alone(
                     c, Sb, h.at(s0), out, [&](int s) { return verdict(v[s]); },
                     [&](int s, plan::Verdict *pv) {
                         std::vector<ScoreTileModel> one(1, m[s]);
                         Verdict v2 = {};
                         int rc2;
                         if ((rc2 = upload(c, 1, dm + s, one, std::vector<int>(1, plan::doubled(W[s], SCORE_TILE_W_MAX)))) ||
                             (rc2 = pass(c, 1, dm + s, out + (size_t)s * K, &v2)))
                             return rc2;
                         *pv = v2.range != 0 ? plan::Verdict::failed : plan::verdict_of(v2.fails);
                         return BHMM_OK;
                     })))
                return rc;
        }
        return BHMM_OK;
    }
};

} // namespace
} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_score(bhmm_ctx *c, int nmodels, const double *A, const double *pi, const double *par0, const double *par1,
               double *logL)
{
    int rc = enter_model_call(c, A && pi && logL, "A / pi / logL == NULL", true, par0, par1);
    if (rc)
        return rc;
    if (nmodels < 1)
        return invalid_arg("bhmm_score: nmodels must be >= 1");
    if ((rc = check_models(c, "bhmm_score", nmodels, A, pi, par0, par1)))
        return rc;
    const bool emis = c->kind == EMIT_GAUSS || c->kind == EMIT_DISC;
    const bool fast = fused_takes(c);
    const bool tile = c->gen && c->n <= 128 && emis; // 65..128 states
    c->last.score_path = fast ? 1 : (c->wide && emis ? 2 : (tile ? 3 : 0));
    c->last.score_segments = c->last.score_W_max = 0;
    const StackedModels h(c, A, pi, par0, par1);
    if (tile)
        return c->kind == EMIT_GAUSS ? Tile<EMIT_GAUSS>::run(c, nmodels, h, logL)
                                     : Tile<EMIT_DISC>::run(c, nmodels, h, logL);
    if (c->last.score_path == 2) // 9..64 states: lanes per segment in c->N
        return c->N == 16   ? run_wide<16>(c, nmodels, h, logL)
               : c->N == 32 ? run_wide<32>(c, nmodels, h, logL)
                            : run_wide<64>(c, nmodels, h, logL);
    if (!fast)
        return score_serial(c, nmodels, h, logL);
    if (c->opt.score_layout == 1) // one lane per chunk, the real state count
        return dispatch_n(c->n, [&](auto N) { return run_n<decltype(N)::value, false>(c, nmodels, h, logL); });
    switch (c->N) { // N/2 lanes per chunk (P1's layout), padded state count
    case 2:
        return run_n<2, true>(c, nmodels, h, logL);
    case 4:
        return run_n<4, true>(c, nmodels, h, logL);
    default:
        return run_n<8, true>(c, nmodels, h, logL);
    }
}

} // extern "C"
