// seg_host.hpp -- host scaffolding the verified time-parallel passes share (the E-step's probes, bhmm_score,
// bhmm_filter, bhmm_posterior_decode, bhmm_posterior_marginals): the constants of their protocol, the staging of
// the forgetting probe around each caller's kernel launch, the padded B^T of the kernels for up to 8 states, the
// parameter block of a WideModel, the upload of a forward-only pass's segment plan, and the staging of the exact
// serial recursions' parameters.  What only the paths for up to 8 states share is in fused_host.hpp.  The arithmetic
// and the acceptance protocol are plan.hpp's (pure host code); this header touches the device.
#pragma once
#include <math.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "plan.hpp"

namespace bhmm {

constexpr double BOUNDARY_TOL = 1e-11;      // boundary check: componentwise relative (the E-step's spec_tol default)
constexpr int W_UNPROBED = 288;             // warm-up when the trajectories are too short to probe (the E-step's)
constexpr size_t LDS_BT_MAX = 16 * 1024;    // B^T of a model staged in LDS up to this size
constexpr int PROBE_P = 256;                // sample positions of the forgetting probe
// (the factor on the probe's reading at 9..64 states: plan::PROBE_WIDE_MARGIN)

// ---- the forgetting probe: staging around the caller's launch ----
// buf holds [starts (PROBE_P) | curve (ncurves x 2 Wmax words: forward | backward)].  probe_stage computes and
// uploads the sample positions and zeroes the curves; the caller launches its kernel once per curve on c->stream;
// probe_read brings the curves back and waits (the host copy of the positions lives in the Probe until then).
struct Probe {
    std::vector<int64_t> starts;
    int64_t *d_starts = nullptr;
    unsigned int *d_curve = nullptr;
    size_t words = 0; // of all curves
};
inline int probe_stage(bhmm_ctx *c, DevBuf<char> &buf, int Wmax, int ncurves, Probe &p)
{
    plan::probe_starts(c->offsets, c->K, Wmax, PROBE_P, p.starts);
    p.words = (size_t)ncurves * 2 * Wmax;
    int rc;
    if ((rc = buf.ensure(PROBE_P * sizeof(int64_t) + p.words * sizeof(unsigned int))))
        return rc;
    p.d_starts = reinterpret_cast<int64_t *>(buf.p);
    p.d_curve = reinterpret_cast<unsigned int *>(p.d_starts + PROBE_P);
    BHMM_HIP(hipMemcpyAsync(p.d_starts, p.starts.data(), PROBE_P * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemsetAsync(p.d_curve, 0, p.words * sizeof(unsigned int), c->stream));
    return BHMM_OK;
}
inline int probe_read(bhmm_ctx *c, const Probe &p, std::vector<float> &curve)
{
    curve.resize(p.words);
    BHMM_HIP(hipMemcpyAsync(curve.data(), p.d_curve, p.words * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    return BHMM_OK;
}

// ---- B^T of a discrete model for the kernels up to 8 states ----
// bt[M][N] (zeroed by the caller: the padded states stay zero) from B[n][M]
inline void fill_Bt_padded(int n, int N, int M, const double *B, double *bt)
{
    for (int i = 0; i < n; ++i)
        for (int o = 0; o < M; ++o)
            bt[(size_t)o * N + i] = B[(size_t)i * M + o];
}

// ---- the parameter block of a WideModel (wide_kernels.hpp) ----
// [A (n x n) | pi | mu | 1/sigma | cnorm | sigma | ga | gb] (the emission entries stay zero unless gaussian), then
// for a discrete model B (n x M, with_B) and B^T (M x n).  fill_wide_block writes one model's block to h (zeroed
// by the caller) and sets w's pointers into the copy of it at dev; returns where B^T will be (nullptr: gaussian).
// with_B false: w.B = nullptr, the kernel reads B^T alone (65..128 states).
inline size_t wide_block_size(int n, int M, bool disc, bool with_B)
{
    return (size_t)n * n + 7 * n + (disc ? (with_B ? 2 : 1) * (size_t)n * M : 0);
}
// the part every block has (pi == nullptr: zeros); WM: WideModel
template <class WM>
const double *fill_wide_common(int n, int M, bool gauss, const double *A, const double *pi, const double *par0,
                               const double *par1, double *h, const double *dev, WM &w)
{
    memcpy(h, A, sizeof(double) * n * n);
    double *q = h + (size_t)n * n;
    w.gmg = 0.0;
    for (int i = 0; i < n; ++i) {
        q[i] = pi ? pi[i] : 0.0;
        if (gauss) {
            q[n + i] = par0[i];
            q[2 * n + i] = 1.0 / par1[i];
            q[3 * n + i] = 1.0 / (sqrt(2.0 * M_PI) * par1[i]);
            q[4 * n + i] = par1[i];
        }
    }
    if (gauss)
        gauss_pdf_constants(n, n, par1, q + 5 * n, q + 6 * n, &w.gmg);
    w.A = dev;
    w.pi = dev + (size_t)n * n;
    w.mu = w.pi + n;
    w.isig = w.mu + n;
    w.cnorm = w.isig + n;
    w.sigma = w.cnorm + n;
    w.ga = w.sigma + n;
    w.gb = w.ga + n;
    w.B = nullptr;
    w.n = n;
    w.M = M;
    return w.gb + n; // the end of the common part
}
template <class WM>
const double *fill_wide_block(int n, int M, bool disc, bool with_B, const double *A, const double *pi,
                              const double *par0, const double *par1, double *h, const double *dev, WM &w)
{
    const double *end = fill_wide_common(n, M, !disc, A, pi, par0, par1, h, dev, w);
    if (!disc)
        return nullptr;
    const size_t nB = (size_t)n * M;
    double *hB = h + (end - dev), *hBt = with_B ? hB + nB : hB;
    if (with_B) {
        memcpy(hB, par0, sizeof(double) * nB);
        w.B = end;
    }
    for (int i = 0; i < n; ++i)
        for (int o = 0; o < M; ++o)
            hBt[(size_t)o * n + i] = par0[(size_t)i * M + o];
    return dev + (hBt - h);
}

// ---- the segment plan of a forward-only pass ----
// plan::plan_pass for segments of at most seglen steps, its tables (every one sized for at least one element)
// uploaded on the context's stream; waits for the copies (the plan is a temporary)
inline int make_seg_tables(bhmm_ctx *c, SegTables &t, int64_t seglen, bool tiles, int *nseg, int *ntraj, int *ntiles)
{
    plan::PassPlan p;
    plan::plan_pass(c->offsets, c->K, seglen, tiles, p);
    const size_t ns = p.seg.traj.size(), ns1 = std::max<size_t>(ns, 1);
    int rc;
    if ((rc = t.seg_traj.ensure(ns1)) || (rc = t.seg_len.ensure(ns1)) || (rc = t.seg_t0.ensure(ns1)) ||
        (rc = t.seg_traj0.ensure(c->K + 1)) || (tiles && (rc = t.tile_seg.ensure(std::max<size_t>(p.tile_seg.size(), 16)))))
        return rc;
    BHMM_HIP(hipMemcpyAsync(t.seg_traj.p, p.seg.traj.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(t.seg_len.p, p.seg.len.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(t.seg_t0.p, p.seg.t0.data(), ns * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(t.seg_traj0.p, p.seg.traj0.data(), (c->K + 1) * sizeof(int32_t), hipMemcpyHostToDevice,
                            c->stream));
    if (tiles)
        BHMM_HIP(hipMemcpyAsync(t.tile_seg.p, p.tile_seg.data(), p.tile_seg.size() * sizeof(int32_t),
                                hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    *nseg = (int)ns;
    *ntraj = p.ntraj;
    *ntiles = (int)(p.tile_seg.size() / 16);
    return BHMM_OK;
}

// the kernels' view of such tables (W: per call, or 0 where every model brings its own)
template <class SEGS>
SEGS segs_of_tables(const SegTables &t, int nseg, int W)
{
    SEGS sg;
    sg.traj = t.seg_traj.p;
    sg.t0 = t.seg_t0.p;
    sg.len = t.seg_len.p;
    sg.nseg = nseg;
    sg.W = W;
    return sg;
}

// ---- the exact serial recursions (k_score_serial, k_filter_serial) ----
// The caller's stacked arrays of S models as the kernels read them, [A | pi | par0 | par1] in buf, copied on the
// context's stream (no wait); what the emission kind does not have is nullptr.  view.at(g): model g of them
struct StackedModels {
    const double *A = nullptr, *pi = nullptr, *par0 = nullptr, *par1 = nullptr;
    size_t n = 0, np0 = 0, np1 = 0; // values per model of pi, par0 and par1
    StackedModels() = default;
    StackedModels(const bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1)
        : A(A), pi(pi), n(c->n), np0(c->kind == EMIT_GAUSS ? n : (c->kind == EMIT_DISC ? n * c->M : 0)),
          np1(c->kind == EMIT_GAUSS ? n : 0)
    {
        this->par0 = np0 ? par0 : nullptr;
        this->par1 = np1 ? par1 : nullptr;
    }
    StackedModels at(size_t g) const
    {
        StackedModels v = *this;
        v.A += g * n * n, v.pi += g * n;
        v.par0 = par0 ? par0 + g * np0 : nullptr;
        v.par1 = par1 ? par1 + g * np1 : nullptr;
        return v;
    }
};
inline int stage_serial_models(bhmm_ctx *c, DevBuf<double> &buf, size_t S, const StackedModels &h, StackedModels &d)
{
    if (int rc = buf.ensure(S * (h.n * h.n + h.n + h.np0 + h.np1)))
        return rc;
    d = h;
    double *dA = buf.p, *dpi = dA + S * h.n * h.n, *dp0 = dpi + S * h.n, *dp1 = dp0 + S * h.np0;
    BHMM_HIP(hipMemcpyAsync(dA, h.A, S * h.n * h.n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(dpi, h.pi, S * h.n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (h.np0)
        BHMM_HIP(hipMemcpyAsync(dp0, h.par0, S * h.np0 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (h.np1)
        BHMM_HIP(hipMemcpyAsync(dp1, h.par1, S * h.np1 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    d.A = dA, d.pi = dpi, d.par0 = h.np0 ? dp0 : nullptr, d.par1 = h.np1 ? dp1 : nullptr;
    return BHMM_OK;
}
// f(std::integral_constant<int, KIND>()) for one of the three emission kinds
template <class F>
auto dispatch_kind(int kind, F f)
{
    if (kind == EMIT_GAUSS)
        return f(std::integral_constant<int, EMIT_GAUSS>());
    if (kind == EMIT_DISC)
        return f(std::integral_constant<int, EMIT_DISC>());
    return f(std::integral_constant<int, EMIT_EXPL>());
}
// f(std::integral_constant<int, NP>()) for the lanes per state vector of the kernels up to 64 states: 8 (LO = 8
// only), 16, 32 or 64
template <int LO = 8, class F>
auto dispatch_np(int np, F f)
{
    if constexpr (LO <= 8)
        if (np == 8)
            return f(std::integral_constant<int, 8>());
    if (np == 16)
        return f(std::integral_constant<int, 16>());
    if (np == 32)
        return f(std::integral_constant<int, 32>());
    return f(std::integral_constant<int, 64>());
}

} // namespace bhmm
