// estep_f32.hip -- host side of the single-precision E-step for up to 8 states (BHMM_FLAG_SINGLE):
// eligibility, the fp32 model, the warm-up length, launches and the verdict.  The kernels are in
// estep_f32.hpp; the packed statistics come out of the fp64 path's k_logl / k_finalize, so the
// vector has the layout of bhmm_ctx_stats_size and everything after the E-step is unchanged.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "estep_f32.hpp"

namespace bhmm {

namespace {

// the smallest nonzero model entry the fp32 kernels take (products of a few such entries stay normal)
constexpr double F32_MIN_ENTRY = 0x1p-100;
// LDS the fp32 sweep may use (discrete: B^T in fp32 + the 64-bit count table)
constexpr size_t F32_LDS_MAX = 150 * 1024;
// discrete symbol counts are integer sums of gamma rounded to 2^-31 (estep_f32.hpp): an entry is off by at most
// 2^-32 per step that carries its symbol, i.e. by total * 2^-32 in the worst case -- an ABSOLUTE error.  A state
// whose count is not large against that (nearly unoccupied: its row could even come out as zero) has its
// symbol counts resolved to this fraction of its total only by the fp64 path
constexpr double F32_COUNT_REL = 1e-6;

bool entry_ok(double v) { return std::isfinite(v) && v >= 0.0 && (v == 0.0 || v >= F32_MIN_ENTRY); }

int stats_len(const bhmm_ctx *c)
{
    const int n = c->n;
    return 1 + n + n * n + n + (c->kind == EMIT_GAUSS ? 2 * n : (c->kind == EMIT_DISC ? n * c->M : 0));
}

template <int N, int KIND>
int run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
        double *stats_dev, bool *done)
{
    const int n = c->n;
    // ---- model: ranges fp32 holds without loss ----
    for (int e = 0; e < n * n; ++e)
        if (!entry_ok(A[e]))
            return BHMM_OK;
    for (int i = 0; i < n; ++i)
        if (!entry_ok(pi[i]))
            return BHMM_OK;
    if (KIND == EMIT_GAUSS) {
        for (int i = 0; i < n; ++i)
            if (!std::isfinite(par0[i]) || !(par1[i] > 0.0) || !std::isfinite(par1[i]) ||
                1.0 / (sqrt(2.0 * M_PI) * par1[i]) > 1048576.0)
                return BHMM_OK;
    } else {
        for (int64_t e = 0; e < (int64_t)n * c->M; ++e)
            if (!entry_ok(par0[e]))
                return BHMM_OK;
    }
    const size_t sm = f32_smem_bytes<N, KIND>(c->M);
    if (sm > F32_LDS_MAX)
        return BHMM_OK; // (alphabet too large for the tables in LDS)

    Model<N> m; // fp64 model of the finalisation (xi = A o sums, packed offsets)
    fill_model<N>(m, n, c->kind, c->M, A, pi, par0, par1);
    ModelF<N> mf;
    memset(&mf, 0, sizeof(mf));
    for (int e = 0; e < N * N; ++e)
        mf.A[e] = (float)m.A[e];
    for (int i = 0; i < N; ++i) {
        mf.pi[i] = (float)m.pi[i];
        mf.gk[i] = 1.f;
        mf.gc[i] = -INFINITY;
    }
    if (KIND == EMIT_GAUSS)
        for (int i = 0; i < n; ++i) {
            mf.mu[i] = par0[i];
            mf.gk[i] = (float)(1.4426950408889634 / (2.0 * par1[i] * par1[i]));
            mf.gc[i] = (float)(-log2(sqrt(2.0 * M_PI) * par1[i]));
        }
    mf.nreal = n;
    mf.M = c->M;

    int rc;
    // ---- warm-up: the measured forgetting curve read at a thousandth of the fp32 tolerance, +50 % ----
    // (the curve samples 256 stretches, the check sees every boundary, and rounding alone leaves the
    // fp32 check a floor of about 1.5e-6: the warm-up's own error must stay well below that.  Read
    // like the fp64 path -- a hundredth, +15 % -- a 4 x 1e6 discrete set checked at 1.3e-5)
    int W = c->opt.f32_W > 0 ? c->opt.f32_W : c->ds.f32_W;
    if (W <= 0) {
        int Wp = 0;
        if ((rc = probe_warmup_target(c, A, pi, par0, par1, 1e-3 * c->opt.f32_tol, &Wp)))
            return rc;
        W = c->ds.f32_W = std::max((Wp * 3 / 2 + 3) / 4 * 4, 16);
    }
    mf.W = W;

    const int S = stats_len(c);
    if ((rc = c->d_f32vec.ensure((size_t)4 * c->Gp * N)) || (rc = c->d_f32words.ensure(2)))
        return rc;
    if (!c->h_small)
        BHMM_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_small), 8192 * sizeof(double), hipHostMallocDefault));
    if (KIND == EMIT_DISC) {
        if ((rc = c->d_Bt32.ensure((size_t)c->M * N)))
            return rc;
        std::vector<float> bt((size_t)c->M * N, 0.f);
        for (int i = 0; i < n; ++i)
            for (int o = 0; o < c->M; ++o)
                bt[(size_t)o * N + i] = (float)par0[(size_t)i * c->M + o];
        BHMM_HIP(hipMemcpyAsync(c->d_Bt32.p, bt.data(), bt.size() * sizeof(float), hipMemcpyHostToDevice,
                                c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (bt is a temporary)
    }
    BHMM_HIP(hipMemsetAsync(c->d_f32words.p, 0, 2 * sizeof(unsigned int), c->stream));
    const Chunks ch = chunks_of(c);
    const int nblk = c->Gp / 64;
    BHMM_HIP(hipEventRecord(c->ev[2], c->stream));
    BHMM_HIP(launch(k_estep_f32<N, KIND>, dim3(nblk), dim3(32 * N), sm, c->stream, mf, ch, c->d_obs_ci.p,
                    c->d_obs_rm.p, c->d_offsets.p, c->d_Bt32.p, reinterpret_cast<float *>(c->d_ws.p),
                    c->d_f32vec.p, c->Gp, c->d_logLc.p, c->d_gamma0.p, c->d_partials.p, c->d_dpartials.p,
                    c->d_f32words.p + 1));
    BHMM_HIP(hipEventRecord(c->ev[3], c->stream));
    if (c->G > 1)
        BHMM_HIP(launch(k_f32_check<N>, dim3((c->G + 255) / 256), dim3(256), 0, c->stream, ch, c->G, c->Gp,
                        c->d_f32vec.p, c->d_f32words.p));
    BHMM_HIP(launch(k_logl, dim3(c->K), dim3(64), 0, c->stream, c->d_traj_c0.p, c->K, c->d_logLc.p,
                    c->d_logLk.p));
    const int nfin = StatLayout<N, KIND>::S + (KIND == EMIT_DISC ? c->M * N : 0) + N + 1;
    BHMM_HIP(launch(k_finalize<N, KIND>, dim3(nfin), dim3(64), 0, c->stream, m, c->K, nblk, c->d_partials.p,
                    c->d_dpartials.p, c->d_logLk.p, c->d_gamma0.p, stats_dev));
    BHMM_HIP(hipEventRecord(c->ev[4], c->stream));
    // verdict words, statistics and (few trajectories) logL_k on one synchronisation
    c->logLk_prefetched = c->K <= 4096;
    BHMM_HIP(hipMemcpyAsync(c->h_small, c->d_f32words.p, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost,
                            c->stream));
    BHMM_HIP(hipMemcpyAsync(c->h_pinned, stats_dev, S * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (c->logLk_prefetched)
        BHMM_HIP(hipMemcpyAsync(c->h_pinned + S, c->d_logLk.p, c->K * sizeof(double), hipMemcpyDeviceToHost,
                                c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    unsigned int words[2];
    memcpy(words, c->h_small, sizeof(words));
    float dev;
    memcpy(&dev, &words[0], sizeof(dev));
    c->last.f32_last_dev = dev;
    bool ok = words[1] == 0 && dev <= c->opt.f32_tol;
    for (int e = 0; e < S && ok; ++e)
        ok = std::isfinite(c->h_pinned[e]);
    if (KIND == EMIT_DISC) // (packed layout: state counts behind logL, sum gamma_0 and C)
        for (int i = 0; i < n && ok; ++i)
            ok = (double)c->total * 0x1p-32 <= F32_COUNT_REL * c->h_pinned[1 + n + n * n + i];
    if (!ok) {
        // boundaries that did not verify: a longer warm-up for the next call (unless the caller fixed it)
        if (words[1] == 0 && !(dev <= c->opt.f32_tol) && c->opt.f32_W <= 0)
            c->ds.f32_W = std::min(2 * W, 1 << 16);
        c->prefetched = false;
        return BHMM_OK;
    }
    c->prefetched = true;
    c->ev_lean = true;
    c->ev_pending = true;
    *done = true;
    return BHMM_OK;
}

template <int N>
int run_n(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
          double *stats_dev, bool *done)
{
    return c->kind == EMIT_GAUSS ? run<N, EMIT_GAUSS>(c, A, pi, par0, par1, stats_dev, done)
                                 : run<N, EMIT_DISC>(c, A, pi, par0, par1, stats_dev, done);
}

} // namespace

int estep_f32(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
              double *stats_dev, int flags, bool *done)
{
    *done = false;
    // the chunk-parallel family with fused emissions, no gamma rows, not on the careful kernels
    if (c->wide || c->gen || c->N > 8 || (c->kind != EMIT_GAUSS && c->kind != EMIT_DISC) ||
        (flags & BHMM_FLAG_STORE_GAMMA) || c->ds.careful || c->bt_global)
        return BHMM_OK;
    // whatever this call leaves in the workspaces, the fp64 path's carried boundary vectors no longer
    // belong to the E-step before the next one
    c->ds.carry_valid = false;
    switch (c->N) {
    case 2:
        return run_n<2>(c, A, pi, par0, par1, stats_dev, done);
    case 4:
        return run_n<4>(c, A, pi, par0, par1, stats_dev, done);
    default:
        return run_n<8>(c, A, pi, par0, par1, stats_dev, done);
    }
}

} // namespace bhmm
