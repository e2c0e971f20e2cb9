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
// Nothing here reads or writes the state other calls use: the buffers are c->filt.*, the plans' sizes
// ds.filt_*, the only other fields touched are opt.filter_* (read) and last.filter_*.  Host results are staged in c->filt.rows / c->filt.logc and
// cross the link in ONE copy each, after the boundaries verified (a pageable buffer of 8 MiB or more is pinned
// for it).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "filter_kernels.hpp"
#include "filter_tile_launch.hpp"
#include "filter_wide_launch.hpp"
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "model_check.hpp"
#include "plan.hpp"

namespace bhmm {
FILTER_TILE_LAUNCH_DECL(extern, 5)
FILTER_TILE_LAUNCH_DECL(extern, 6)
FILTER_TILE_LAUNCH_DECL(extern, 7)
FILTER_TILE_LAUNCH_DECL(extern, 8)
namespace {

constexpr double FILTER_TOL = 1e-11;         // boundary check: componentwise relative (bhmm_score's)
constexpr int FILTER_W_UNPROBED = 288;       // warm-up when the trajectories are too short to probe (bhmm_score's)
constexpr size_t FILTER_LDS_BT = 16 * 1024;  // B^T staged in LDS up to this size
constexpr double FILTER_WIDE_MARGIN = 1.5;   // 9..64 states: warm-up over the probe's reading (bhmm_score's factor)

struct Out {          // where the results go on the device, and what they are
    void *rows;       // [total][Qp] of double / float, or nullptr
    void *logc;       // [total] of double / float, or nullptr
    const double *V;  // device copy of the projection, or nullptr
    int Q;            // its columns (0: none)
    int Qp;           // values per row
    bool f32;
};

// warm-up from the forgetting curve, the reading bhmm_score takes (score_api.hip, Fast::probe): forward chains
// within 0.01 of the check's tolerance from then on, + 15 %, doubled.  0 where the trajectories are too short to
// probe
template <int N, int KIND>
int filter_probe(bhmm_ctx *c, const Model<N> &m, const double *dBt, int *W)
{
    *W = 0;
    const int64_t maxT = longest_traj(c);
    const int Wmax = (int)std::min<int64_t>(1024, maxT / 2) / 4 * 4;
    if (Wmax < 32)
        return BHMM_OK;
    std::vector<int> longk;
    for (int k = 0; k < c->K; ++k)
        if (c->offsets[k + 1] - c->offsets[k] >= Wmax)
            longk.push_back(k);
    const int P = 256;
    std::vector<int64_t> starts(P);
    for (int i = 0; i < P; ++i) {
        const int k = longk[i % longk.size()];
        const int64_t room = c->offsets[k + 1] - c->offsets[k] - Wmax + 1;
        const int64_t rep = i / (int64_t)longk.size(), reps = (P + longk.size() - 1) / longk.size();
        starts[i] = c->offsets[k] + (room - 1) * rep / std::max<int64_t>(reps - 1, 1);
    }
    const size_t curve_words = 2 * (size_t)Wmax; // forward | backward (the kernel's layout)
    int rc;
    if ((rc = c->filt.probe.ensure(P * sizeof(int64_t) + curve_words * sizeof(unsigned int))))
        return rc;
    int64_t *d_starts = reinterpret_cast<int64_t *>(c->filt.probe.p);
    unsigned int *d_curve = reinterpret_cast<unsigned int *>(d_starts + P);
    BHMM_HIP(hipMemcpyAsync(d_starts, starts.data(), P * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemsetAsync(d_curve, 0, curve_words * sizeof(unsigned int), c->stream));
    BHMM_HIP(launch(k_forget_probe<N, KIND>, dim3((2 * P + 63) / 64), dim3(64), 0, c->stream, m, c->d_obs_rm.p,
                    KIND == EMIT_DISC ? dBt : nullptr, d_starts, P, Wmax, d_curve));
    std::vector<float> curve(Wmax); // the forward direction: the first Wmax entries
    BHMM_HIP(hipMemcpyAsync(curve.data(), d_curve, curve.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    const float target = (float)(0.01 * FILTER_TOL);
    int last = -1;
    for (int w = 0; w < Wmax; ++w)
        if (curve[w] >= target)
            last = w;
    const int w = (int)std::ceil(1.15 * (last + 2));
    *W = 2 * std::min(std::max(16, (w + 3) / 4 * 4), Wmax);
    return BHMM_OK;
}

template <int N, int KIND>
struct Fused {
    template <typename OT, bool PROJ, bool WANT_LOGC>
    static auto kernel(bool bt_lds)
    {
        return bt_lds ? k_filter_sweep<N, KIND, true, OT, PROJ, WANT_LOGC>
                      : k_filter_sweep<N, KIND, false, OT, PROJ, WANT_LOGC>;
    }

    // the sweep, the first dead chunk of every trajectory, the check and the fix-up; *fails: boundaries out of
    // tolerance
    template <typename OT>
    static int pass(bhmm_ctx *c, const Model<N> *dm, int W, const double *dBt, const Out &o, unsigned int *fails)
    {
        auto &b = c->filt;
        const int G = c->G, groups = c->Gp / 64;
        const Chunks ch = chunks_of(c);
        const size_t lds_bt = (size_t)c->M * score_bt_stride(N) * sizeof(double);
        const bool bt_lds = KIND == EMIT_DISC && lds_bt <= FILTER_LDS_BT;
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
                            b.aexit.p, b.first_dead.p, FILTER_TOL, b.fails.p));
            BHMM_HIP(launch(k_filter_bury<OT>, dim3((G + 255) / 256), dim3(256), 0, c->stream, ch, G, b.first_dead.p,
                            static_cast<OT *>(o.rows), o.Qp, static_cast<OT *>(o.logc)));
        }
        BHMM_HIP(hipMemcpyAsync(fails, b.fails.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        return BHMM_OK;
    }

    // *verified: the results in o stand
    static int run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                   const Out &o, bool *verified)
    {
        auto &b = c->filt;
        const int M = c->M, n = c->n;
        *verified = false;
        int rc;
        if ((rc = b.model.ensure(sizeof(Model<N>))) || (rc = b.aentry.ensure((size_t)c->Gp * N)) ||
            (rc = b.aexit.ensure((size_t)c->Gp * N)) || (rc = b.dead.ensure(c->Gp)) ||
            (rc = b.first_dead.ensure(std::max(c->K, 1))) || (rc = b.fails.ensure(1)) ||
            (KIND == EMIT_DISC && (rc = b.Bt.ensure((size_t)M * N))))
            return rc;
        Model<N> m;
        fill_model<N>(m, n, KIND, M, A, pi, par0, par1);
        Model<N> *dm = reinterpret_cast<Model<N> *>(b.model.p);
        std::vector<double> bt;
        if (KIND == EMIT_DISC) {
            bt.resize((size_t)M * N);
            for (int i = 0; i < n; ++i)
                for (int s = 0; s < M; ++s)
                    bt[(size_t)s * N + i] = par0[(size_t)i * M + s];
            BHMM_HIP(hipMemcpyAsync(b.Bt.p, bt.data(), bt.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        }
        BHMM_HIP(hipMemcpyAsync(dm, &m, sizeof(Model<N>), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (m and bt are temporaries)
        int W = c->opt.filter_W;
        if (W <= 0) {
            if ((rc = filter_probe<N, KIND>(c, m, b.Bt.p, &W)))
                return rc;
            W = W > 0 ? W : FILTER_W_UNPROBED;
        }
        for (int attempt = 0; attempt < 2; ++attempt) {
            unsigned int fails = 0;
            rc = o.f32 ? pass<float>(c, dm, W, b.Bt.p, o, &fails) : pass<double>(c, dm, W, b.Bt.p, o, &fails);
            if (rc)
                return rc;
            if (fails == 0) {
                *verified = true;
                return BHMM_OK;
            }
            if (attempt == 0)
                ++c->last.filter_fallbacks; // boundaries that did not verify at the first warm-up
            W = (int)std::min<int64_t>(2 * (int64_t)W, 1 << 30);
        }
        return BHMM_OK;
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
    auto &b = c->filt;
    if (d.filt_nseg > 0 && d.filt_seglen_opt == c->opt.filter_seglen)
        return BHMM_OK;
    plan::SegPlan sp; // (plan.hpp: pure host code)
    plan::plan_segments(c->offsets, c->K, plan::score_seglen(c->total, c->N, c->num_simd, c->opt.filter_seglen), 1,
                        sp);
    const size_t ns = sp.traj.size();
    int rc;
    if ((rc = b.seg_traj.ensure(ns)) || (rc = b.seg_len.ensure(ns)) || (rc = b.seg_t0.ensure(ns)) ||
        (rc = b.seg_traj0.ensure(c->K + 1)))
        return rc;
    BHMM_HIP(hipMemcpyAsync(b.seg_traj.p, sp.traj.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(b.seg_len.p, sp.len.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(b.seg_t0.p, sp.t0.data(), ns * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(b.seg_traj0.p, sp.traj0.data(), (c->K + 1) * sizeof(int32_t), hipMemcpyHostToDevice,
                            c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream)); // (sp is a temporary)
    d.filt_nseg = (int)ns;
    d.filt_ntraj = 0;
    for (int k = 0; k < c->K; ++k)
        d.filt_ntraj += c->offsets[k + 1] > c->offsets[k];
    d.filt_seglen_opt = c->opt.filter_seglen;
    return BHMM_OK;
}

struct WideFilt {
    // warm-up: k_wide_probe's forward chains, read as bhmm_score reads them (score_api.hip, Wide::probe) --
    // chains within 1e-13 from then on, times 1.5, rounded up to 8
    static int probe(bhmm_ctx *c, const WideModel &m, int *W)
    {
        *W = FILTER_W_UNPROBED;
        const int Wmax = (int)std::min<int64_t>(8192, longest_traj(c) / 2) / 8 * 8;
        if (Wmax < 64)
            return BHMM_OK; // (trajectories of fewer than 128 steps)
        std::vector<int> longk;
        for (int k = 0; k < c->K; ++k)
            if (c->offsets[k + 1] - c->offsets[k] >= Wmax)
                longk.push_back(k);
        const int P = 256;
        std::vector<int64_t> starts(P);
        for (int i = 0; i < P; ++i) {
            const int k = longk[i % longk.size()];
            const int64_t room = c->offsets[k + 1] - c->offsets[k] - Wmax + 1;
            const int64_t rep = i / (int64_t)longk.size(), reps = (P + longk.size() - 1) / longk.size();
            starts[i] = c->offsets[k] + (room - 1) * rep / std::max<int64_t>(reps - 1, 1);
        }
        const size_t curve_words = 2 * (size_t)Wmax; // (the kernel's layout: forward | backward, the latter stays zero)
        int rc;
        if ((rc = c->filt.probe.ensure(P * sizeof(int64_t) + curve_words * sizeof(unsigned int))))
            return rc;
        int64_t *d_starts = reinterpret_cast<int64_t *>(c->filt.probe.p);
        unsigned int *d_curve = reinterpret_cast<unsigned int *>(d_starts + P);
        BHMM_HIP(hipMemcpyAsync(d_starts, starts.data(), P * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipMemsetAsync(d_curve, 0, curve_words * sizeof(unsigned int), c->stream));
        if ((rc = filter_wide_probe_launch(c, c->N, m, d_starts, P, Wmax, d_curve)))
            return rc;
        std::vector<float> curve(Wmax); // the forward direction: the first Wmax entries
        BHMM_HIP(hipMemcpyAsync(curve.data(), d_curve, curve.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        int last = -1;
        for (int w = 0; w < Wmax; ++w)
            if (curve[w] >= 1e-13f)
                last = w;
        const int w = (int)std::ceil(FILTER_WIDE_MARGIN * (last + 2));
        *W = std::min(std::max(16, (w + 7) / 8 * 8), Wmax); // (not forgotten within Wmax: Wmax, the check decides)
        return BHMM_OK;
    }

    // the sweep, the first dead segment of every trajectory, the check and the fix-up; *fails: boundaries out of
    // tolerance
    static int pass(bhmm_ctx *c, const ScoreWideModel *dm, int W, const Out &o, unsigned int *fails)
    {
        auto &b = c->filt;
        const int nseg = c->ds.filt_nseg;
        FilterWideArgs a;
        a.dm = dm;
        a.W = W;
        a.sg.traj = b.seg_traj.p;
        a.sg.t0 = b.seg_t0.p;
        a.sg.len = b.seg_len.p;
        a.sg.nseg = nseg;
        a.sg.W = W;
        a.rows = o.rows;
        a.logc = o.logc;
        a.V = o.V;
        a.Q = o.Q;
        a.f32 = o.f32;
        a.aentry = b.aentry.p;
        a.aexit = b.aexit.p;
        a.dead = b.dead.p;
        *fails = 0;
        int rc;
        if ((rc = filter_wide_launch(c, c->N, a)))
            return rc;
        if (nseg > c->ds.filt_ntraj) { // (no boundary: the exact recursion, nothing after a dead segment)
            const FiltSegs fs{b.seg_traj.p, b.seg_t0.p, b.seg_len.p, c->d_offsets.p, nseg};
            BHMM_HIP(hipMemsetAsync(b.fails.p, 0, sizeof(unsigned int), c->stream));
            BHMM_HIP(launch(k_filter_first_dead, dim3(c->K), dim3(64), 0, c->stream, b.seg_traj0.p, b.dead.p,
                            b.first_dead.p));
            BHMM_HIP(launch(k_filter_seg_check, dim3((nseg + 255) / 256), dim3(256), 0, c->stream, fs, c->n, b.aentry.p,
                            b.aexit.p, b.first_dead.p, FILTER_TOL, b.fails.p));
            if (o.f32)
                BHMM_HIP(launch(k_filter_seg_bury<float>, dim3(nseg), dim3(64), 0, c->stream, fs, b.first_dead.p,
                                static_cast<float *>(o.rows), o.Qp, static_cast<float *>(o.logc)));
            else
                BHMM_HIP(launch(k_filter_seg_bury<double>, dim3(nseg), dim3(64), 0, c->stream, fs, b.first_dead.p,
                                static_cast<double *>(o.rows), o.Qp, static_cast<double *>(o.logc)));
            BHMM_HIP(hipMemcpyAsync(fails, b.fails.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        }
        BHMM_HIP(hipStreamSynchronize(c->stream));
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
        // parameter block of the model: wide_model's layout, then B and B^T (bhmm_score's)
        const bool disc = c->kind == EMIT_DISC;
        const size_t nB = disc ? (size_t)n * M : 0, np = (size_t)n * n + 7 * n + 2 * nB;
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
        const double *dp = b.wpar.p;
        memcpy(h.data(), A, sizeof(double) * n * n);
        memcpy(h.data() + (size_t)n * n, pi, sizeof(double) * n);
        WideModel &w = m.w;
        w.A = dp;
        w.pi = dp + (size_t)n * n;
        w.mu = w.pi + n;
        w.isig = w.mu + n;
        w.cnorm = w.isig + n;
        w.sigma = w.cnorm + n;
        w.ga = w.sigma + n;
        w.gb = w.ga + n;
        w.gmg = 0.0;
        w.B = nullptr;
        w.n = n;
        w.M = M;
        m.Bt = nullptr;
        double *q = h.data() + (size_t)n * n + n;
        if (!disc) {
            for (int i = 0; i < n; ++i) {
                q[i] = par0[i];
                q[n + i] = 1.0 / par1[i];
                q[2 * n + i] = 1.0 / (sqrt(2.0 * M_PI) * par1[i]);
                q[3 * n + i] = par1[i];
            }
            gauss_pdf_constants(n, n, par1, q + 4 * n, q + 5 * n, &w.gmg);
        } else {
            double *hB = q + 6 * n, *hBt = hB + nB;
            memcpy(hB, par0, sizeof(double) * nB);
            for (int i = 0; i < n; ++i)
                for (int s = 0; s < M; ++s)
                    hBt[(size_t)s * n + i] = par0[(size_t)i * M + s];
            w.B = w.gb + n;
            m.Bt = w.B + nB;
        }
        ScoreWideModel *dm = reinterpret_cast<ScoreWideModel *>(b.model.p);
        BHMM_HIP(hipMemcpyAsync(b.wpar.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipMemcpyAsync(dm, &m, sizeof(ScoreWideModel), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (h and m are temporaries)
        // a plan without a boundary runs the exact recursion: no probe, no check
        int W = (c->opt.filter_W + 7) / 8 * 8;
        if (segmented && c->opt.filter_W <= 0 && (rc = probe(c, m.w, &W)))
            return rc;
        W = std::max(W, 8);
        for (int attempt = 0; attempt < 2; ++attempt) {
            unsigned int fails = 0;
            if ((rc = pass(c, dm, W, o, &fails)))
                return rc;
            if (fails == 0) {
                *verified = true;
                return BHMM_OK;
            }
            if (attempt == 0)
                ++c->last.filter_fallbacks; // boundaries that did not verify at the first warm-up
            W = (int)std::min<int64_t>(2 * (int64_t)W, 1 << 30);
        }
        return BHMM_OK;
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
    const size_t np0 = c->kind == EMIT_GAUSS ? (size_t)n : (c->kind == EMIT_DISC ? (size_t)n * c->M : 0);
    const size_t np1 = c->kind == EMIT_GAUSS ? (size_t)n : 0;
    auto &b = c->filt;
    int rc;
    if ((rc = b.par.ensure((size_t)n * n + n + np0 + np1)))
        return rc;
    double *dA = b.par.p, *dpi = dA + (size_t)n * n, *dp0 = dpi + n, *dp1 = dp0 + np0;
    BHMM_HIP(hipMemcpyAsync(dA, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(dpi, pi, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (np0)
        BHMM_HIP(hipMemcpyAsync(dp0, par0, np0 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (np1)
        BHMM_HIP(hipMemcpyAsync(dp1, par1, np1 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream)); // (the caller's arrays may be temporaries)
    if (K == 0)
        return BHMM_OK;
    const int bd = std::min(1024, (n + 63) / 64 * 64);
    const size_t lds = ((size_t)n + 16) * sizeof(double);
    OT *rows = static_cast<OT *>(o.rows), *logc = static_cast<OT *>(o.logc);
    const void *obs = c->d_obs_rm.p;
    hipError_t e;
    if (c->kind == EMIT_GAUSS)
        e = launch(k_filter_serial<EMIT_GAUSS, OT>, dim3(K), dim3(bd), lds, c->stream, n, c->M, c->d_offsets.p, obs, dA,
                   dpi, dp0, dp1, o.V, o.Q, rows, logc, only);
    else if (c->kind == EMIT_DISC)
        e = launch(k_filter_serial<EMIT_DISC, OT>, dim3(K), dim3(bd), lds, c->stream, n, c->M, c->d_offsets.p, obs, dA,
                   dpi, dp0, nullptr, o.V, o.Q, rows, logc, only);
    else
        e = launch(k_filter_serial<EMIT_EXPL, OT>, dim3(K), dim3(bd), lds, c->stream, n, c->M, c->d_offsets.p, obs, dA,
                   dpi, nullptr, nullptr, o.V, o.Q, rows, logc, only);
    BHMM_HIP(e);
    return BHMM_OK;
}

// ---- 65..128 states ----------------------------------------------------------------------------

// the segment plan and the tile table of k_filter_tile on this observation set: made at the first eligible call
// (and again when filter_seglen changes), never after a check.  Neither the score plan nor the plan above
int filter_tile_plan(bhmm_ctx *c)
{
    auto &d = c->ds;
    auto &b = c->filt;
    if (d.filt_tile_nseg > 0 && d.filt_tile_seglen_opt == c->opt.filter_seglen)
        return BHMM_OK;
    plan::SegPlan sp; // (plan.hpp: pure host code)
    plan::plan_segments(c->offsets, c->K, plan::score_tile_seglen(c->total, c->num_simd, c->opt.filter_seglen), 1, sp);
    std::vector<int32_t> tile_seg;
    plan::plan_tiles(sp, c->offsets, false, tile_seg);
    const size_t ns = sp.traj.size();
    int rc;
    if ((rc = b.tseg_traj.ensure(std::max<size_t>(ns, 1))) || (rc = b.tseg_len.ensure(std::max<size_t>(ns, 1))) ||
        (rc = b.tseg_t0.ensure(std::max<size_t>(ns, 1))) || (rc = b.tseg_traj0.ensure(c->K + 1)) ||
        (rc = b.tile_seg.ensure(std::max<size_t>(tile_seg.size(), 16))))
        return rc;
    BHMM_HIP(hipMemcpyAsync(b.tseg_traj.p, sp.traj.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(b.tseg_len.p, sp.len.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(b.tseg_t0.p, sp.t0.data(), ns * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(b.tseg_traj0.p, sp.traj0.data(), (c->K + 1) * sizeof(int32_t), hipMemcpyHostToDevice,
                            c->stream));
    BHMM_HIP(hipMemcpyAsync(b.tile_seg.p, tile_seg.data(), tile_seg.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                            c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream)); // (sp and tile_seg are temporaries)
    d.filt_tile_nseg = (int)ns;
    d.filt_tile_ntiles = (int)(tile_seg.size() / 16);
    d.filt_tile_ntraj = 0;
    for (int k = 0; k < c->K; ++k)
        d.filt_tile_ntraj += c->offsets[k + 1] > c->offsets[k];
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
        a.sg.traj = b.tseg_traj.p;
        a.sg.t0 = b.tseg_t0.p;
        a.sg.len = b.tseg_len.p;
        a.sg.nseg = nseg;
        a.sg.W = W;
        a.tp = TilePlan{b.tile_seg.p, c->ds.filt_tile_ntiles};
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
        BHMM_HIP(launch(k_filter_tile_redo, dim3(c->K), dim3(64), 0, c->stream, b.tseg_traj0.p, b.dead.p, b.redo.p,
                        b.fails.p));
        if (nseg > c->ds.filt_tile_ntraj) // (no boundary: the exact recursion)
            BHMM_HIP(launch(k_filter_tile_check, dim3((nseg + 15) / 16), dim3(256), 0, c->stream, a.sg, n, b.aentry.p,
                            b.aexit.p, b.redo.p, FILTER_TOL, b.fails.p));
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
        // parameter block of the model: wide_model's layout, then B^T (bhmm_score's)
        const size_t nB = KIND == EMIT_DISC ? (size_t)n * M : 0, np = (size_t)n * n + 7 * n + nB;
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
        const double *dp = b.wpar.p;
        memcpy(h.data(), A, sizeof(double) * n * n);
        memcpy(h.data() + (size_t)n * n, pi, sizeof(double) * n);
        WideModel &w = m.w;
        w.A = dp;
        w.pi = dp + (size_t)n * n;
        w.mu = w.pi + n;
        w.isig = w.mu + n;
        w.cnorm = w.isig + n;
        w.sigma = w.cnorm + n;
        w.ga = w.sigma + n;
        w.gb = w.ga + n;
        w.gmg = 0.0;
        w.B = nullptr; // (the kernel reads B^T)
        w.n = n;
        w.M = M;
        m.Bt = nullptr;
        m.W = 0;
        double *q = h.data() + (size_t)n * n + n;
        if (KIND == EMIT_GAUSS) {
            for (int i = 0; i < n; ++i) {
                q[i] = par0[i];
                q[n + i] = 1.0 / par1[i];
                q[2 * n + i] = 1.0 / (sqrt(2.0 * M_PI) * par1[i]);
                q[3 * n + i] = par1[i];
            }
            gauss_pdf_constants(n, n, par1, q + 4 * n, q + 5 * n, &w.gmg);
        } else {
            double *hBt = q + 6 * n;
            for (int i = 0; i < n; ++i)
                for (int s = 0; s < M; ++s)
                    hBt[(size_t)s * n + i] = par0[(size_t)i * M + s];
            m.Bt = w.gb + n;
        }
        ScoreTileModel *dm = reinterpret_cast<ScoreTileModel *>(b.model.p);
        BHMM_HIP(hipMemcpyAsync(b.wpar.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (h is a temporary)
        // W: multiples of four (the refresh of the scaling).  A plan without a boundary runs the exact recursion: no
        // calibration, no check
        int W = segmented ? (c->opt.filter_W + 3) & ~3 : 0;
        if (segmented && c->opt.filter_W <= 0 && (rc = calibrate(c, dm, m, &W)))
            return rc;
        for (int attempt = 0; attempt < 2; ++attempt) {
            Verdict v;
            if ((rc = pass(c, dm, m, W, &o, &v)))
                return rc;
            if (v.fails == 0) {
                // the trajectories with a segment outside the kernel's range again, whole, on the serial kernel:
                // behind the pass, on the same stream
                c->last.filter_redone = (int)v.redone;
                if (v.redone != 0 && (rc = o.f32 ? serial<float>(c, A, pi, par0, par1, o, b.redo.p)
                                                 : serial<double>(c, A, pi, par0, par1, o, b.redo.p)))
                    return rc;
                *verified = true;
                return BHMM_OK;
            }
            if (attempt == 0)
                ++c->last.filter_fallbacks; // boundaries that did not verify at the first warm-up
            W = (int)std::min<int64_t>(2 * (int64_t)W, SCORE_TILE_W_MAX);
        }
        return BHMM_OK;
    }
};

// a staged result to the caller's host buffer in one copy: a pageable buffer of 8 MiB or more is pinned for the
// transfer, one the caller pinned is used as it is
int deliver(bhmm_ctx *c, void *host, const void *dev, size_t bytes)
{
    if (bytes == 0)
        return BHMM_OK;
    hipPointerAttribute_t attr;
    const bool caller_pinned = hipPointerGetAttributes(&attr, host) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    const bool pinned = !caller_pinned && bytes >= ((size_t)8 << 20) &&
                        hipHostRegister(host, bytes, hipHostRegisterDefault) == hipSuccess;
    if (!pinned)
        (void)hipGetLastError();
    hipError_t ce = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream);
    if (ce == hipSuccess)
        ce = hipStreamSynchronize(c->stream);
    if (pinned)
        (void)hipHostUnregister(host);
    BHMM_HIP(ce);
    return BHMM_OK;
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
    const bool fused = !c->wide && !c->gen && c->n <= 8 && emis && c->G > 0;
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
        switch (c->n) {
        case 1:
            rc = run_n<1>(c, A, pi, par0, par1, o, &verified);
            break;
        case 2:
            rc = run_n<2>(c, A, pi, par0, par1, o, &verified);
            break;
        case 3:
            rc = run_n<3>(c, A, pi, par0, par1, o, &verified);
            break;
        case 4:
            rc = run_n<4>(c, A, pi, par0, par1, o, &verified);
            break;
        case 5:
            rc = run_n<5>(c, A, pi, par0, par1, o, &verified);
            break;
        case 6:
            rc = run_n<6>(c, A, pi, par0, par1, o, &verified);
            break;
        case 7:
            rc = run_n<7>(c, A, pi, par0, par1, o, &verified);
            break;
        default:
            rc = run_n<8>(c, A, pi, par0, par1, o, &verified);
            break;
        }
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
