// gmm_api.hip -- gaussian-mixture emissions per state (bhmm_gmm_emissions, bhmm_gmm_fetch_resp, bhmm_gmm_moments,
// bhmm_logpdf_gmm) and the component draws of their Gibbs sweep (bhmm_gmm_path_components, bhmm_gmm_sample_paths):
// kernels in gmm_kernels.hpp, the factorisation of the N M components on the host (host::mvn_prepare through
// mvn_make_table); DESIGN.md sections 25 and 26.
//
// The mixture runs on the observations bhmm_ctx_set_observations_mvn keeps in c->mvn.X.  bhmm_gmm_emissions makes the
// rows, m_t and shifts of the mixture densities where bhmm_mvn_emissions makes those of single gaussians -- the same
// buffers, the same re-load as explicit observations -- so everything after it (bhmm_mvn_fetch_scale,
// bhmm_mvn_fetch_rows, every context call with par0 = par1 = NULL) is unchanged.  What the mixture adds is the
// (total, N M) buffer c->gmm.resp: log responsibilities after the emissions, the weights u_t(i,c) = gamma_t(i) r_t(i,c)
// after bhmm_gmm_moments, which runs the moment kernels of mvn_api.hip over its N M columns.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "gmm_kernels.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "mvn_host.hpp"

namespace bhmm {
namespace {

using namespace gmm;

// [mu | W | c | log w] of the N M components, validated; BHMM_ERR_INVALID / BHMM_ERR_SIGMA
int make_table(const char *who, int N, int M, int D, int cov_type, const double *weights, const double *means,
               const double *covs, std::vector<double> &tab)
{
    if (M < 1 || (int64_t)N * M > 4096)
        return invalid_arg(std::string(who) + ": M >= 1 components per state and N * M <= 4096");
    const int nm = N * M;
    for (int i = 0; i < N; ++i) {
        long double sum = 0.0L;
        for (int c = 0; c < M; ++c) {
            const double w = weights[(size_t)i * M + c];
            if (!std::isfinite(w) || w < 0.0)
                return invalid_arg(std::string(who) + ": a mixture weight is negative or not finite");
            sum += w;
        }
        if (fabsl(sum - 1.0L) > 1e-8L)
            return invalid_arg(std::string(who) + ": the mixture weights of state " + std::to_string(i) +
                               " do not sum to 1");
    }
    if (int rc = mvn_make_table(who, nm, D, cov_type, means, covs, tab))
        return rc;
    const size_t at = tab.size();
    tab.resize(at + nm);
    for (int q = 0; q < nm; ++q) // log w in long double, rounded once; -inf for a weight of zero
        tab[at + q] = weights[q] > 0.0 ? (double)logl((long double)weights[q]) : -INFINITY;
    return BHMM_OK;
}

template <bool DIAG>
hipError_t launch_rows(hipStream_t stream, const double *X, int64_t total, int D, int n, int M, const double *tab,
                       double *rows, double *m, double *logp, double *resp)
{
    const dim3 grid((unsigned)((total + ROWS_THREADS - 1) / ROWS_THREADS)), block(ROWS_THREADS);
#define BHMM_GMM_ROWS(DMAX)                                                                                            \
    launch(k_gmm_rows<DMAX, DIAG>, grid, block, 0, stream, X, total, D, n, M, tab, rows, m, logp, resp)
    if (D <= 2)
        return BHMM_GMM_ROWS(2);
    if (D <= 4)
        return BHMM_GMM_ROWS(4);
    if (D <= 8)
        return BHMM_GMM_ROWS(8);
    if (D <= 16)
        return BHMM_GMM_ROWS(16);
    if (D <= 32)
        return BHMM_GMM_ROWS(32);
    return BHMM_GMM_ROWS(64);
#undef BHMM_GMM_ROWS
}

int run_rows(hipStream_t stream, const double *X, int64_t total, int D, int n, int M, int cov_type, const double *tab,
             double *rows, double *m, double *logp, double *resp)
{
    if ((total + ROWS_THREADS - 1) / ROWS_THREADS > 0x7fffffff)
        return invalid_arg("gaussian-mixture emissions: more steps than a grid has workgroups");
    BHMM_HIP(cov_type == BHMM_COV_DIAG ? launch_rows<true>(stream, X, total, D, n, M, tab, rows, m, logp, resp)
                                       : launch_rows<false>(stream, X, total, D, n, M, tab, rows, m, logp, resp));
    return BHMM_OK;
}

template <typename PT, bool DIAG>
hipError_t launch_draw(hipStream_t stream, const double *X, const PT *path, int64_t total, int D, int n, int M,
                       const double *tab, const int64_t *off, const int64_t *soff, int K, uint64_t key, int32_t *labels,
                       unsigned int *status)
{
    const dim3 grid((unsigned)((total + ROWS_THREADS - 1) / ROWS_THREADS)), block(ROWS_THREADS);
#define BHMM_GMM_DRAW(DMAX)                                                                                            \
    launch(k_gmm_draw_components<PT, DMAX, DIAG>, grid, block, 0, stream, X, path, total, D, n, M, tab, off, soff, K,  \
           key, labels, status)
    if (D <= 2)
        return BHMM_GMM_DRAW(2);
    if (D <= 4)
        return BHMM_GMM_DRAW(4);
    if (D <= 8)
        return BHMM_GMM_DRAW(8);
    if (D <= 16)
        return BHMM_GMM_DRAW(16);
    if (D <= 32)
        return BHMM_GMM_DRAW(32);
    return BHMM_GMM_DRAW(64);
#undef BHMM_GMM_DRAW
}

bool mixture_loaded(const bhmm_ctx *c) { return c && c->mvn.active && c->mvn.rows_valid && c->gmm.M > 0; }

// The components of the path at path_dev (device; int32 or one byte per step) under the table of the last
// bhmm_gmm_emissions, as labels s_t M + c_t in c->gmm.labels, then the packed moments of those labels about the
// table's own means into moments (host); the labels go to the host only when asked for.  A state outside [0, n):
// BHMM_ERR_INVALID, nothing is delivered.
int run_components(bhmm_ctx *c, const char *who, const void *path_dev, int path_u8, uint64_t seed, int32_t *labels,
                   double *moments)
{
    auto &b = c->mvn;
    auto &g = c->gmm;
    int rc;
    if ((b.total + ROWS_THREADS - 1) / ROWS_THREADS > 0x7fffffff)
        return invalid_arg(std::string(who) + ": more steps than a grid has workgroups");
    if ((rc = g.labels.ensure((size_t)b.total)) || (rc = g.draw_status.ensure(1)))
        return rc;
    for (hipEvent_t &e : g.ev)
        if (!e)
            BHMM_HIP(hipEventCreate(&e));
    const bool diag = g.cov_type == BHMM_COV_DIAG;
    const int64_t *soff = c->d_soff.p; // (nullptr: a step's position in the random stream is its index)
    const uint64_t key = draw_key(seed);
    BHMM_HIP(hipMemsetAsync(g.draw_status.p, 0, sizeof(unsigned int), c->stream));
    BHMM_HIP(hipEventRecord(g.ev[2], c->stream));
#define BHMM_GMM_DRAW_PT(PT)                                                                                           \
    (diag ? launch_draw<PT, true>(c->stream, b.X.p, static_cast<const PT *>(path_dev), b.total, b.D, b.n, g.M, g.tab.p, \
                                  b.d_offsets.p, soff, b.K, key, g.labels.p, g.draw_status.p)                          \
          : launch_draw<PT, false>(c->stream, b.X.p, static_cast<const PT *>(path_dev), b.total, b.D, b.n, g.M,        \
                                   g.tab.p, b.d_offsets.p, soff, b.K, key, g.labels.p, g.draw_status.p))
    BHMM_HIP(path_u8 ? BHMM_GMM_DRAW_PT(uint8_t) : BHMM_GMM_DRAW_PT(int32_t));
#undef BHMM_GMM_DRAW_PT
    BHMM_HIP(hipEventRecord(g.ev[3], c->stream));
    unsigned int status = 0;
    BHMM_HIP(hipMemcpyAsync(&status, g.draw_status.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    (void)hipEventElapsedTime(&g.draw_ms, g.ev[2], g.ev[3]);
    if (status & DRAW_BAD_STATE)
        return invalid_arg(std::string(who) + ": the path holds a state outside [0, " + std::to_string(b.n) + ")");
    // the means of the table's front are the means the moments are taken about: nothing is uploaded
    if ((rc = mvn_run_path_moments(c, who, g.labels.p, 0, b.n * g.M, nullptr, g.tab.p, g.cov_type, moments)))
        return rc;
    if (labels) {
        BHMM_HIP(hipMemcpyAsync(labels, g.labels.p, (size_t)b.total * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
    }
    return BHMM_OK;
}

} // namespace
} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_gmm_emissions(bhmm_ctx *c, int M, const double *weights, const double *means, const double *covs,
                       int cov_type, int want_resp)
{
    if (!c || !c->mvn.active)
        return invalid_arg("bhmm_gmm_emissions: no multivariate observations loaded");
    if (!weights || !means || !covs)
        return invalid_arg("bhmm_gmm_emissions: weights / means / covs == NULL");
    auto &b = c->mvn;
    auto &g = c->gmm;
    int rc;
    if ((rc = mvn_shape_ok("bhmm_gmm_emissions", b.n, b.D, cov_type)))
        return rc;
    std::vector<double> tab;
    if ((rc = make_table("bhmm_gmm_emissions", b.n, M, b.D, cov_type, weights, means, covs, tab)))
        return rc;
    BHMM_HIP(hipSetDevice(c->device));
    b.rows_valid = false;
    g.forget();
    // (the table stays in g.tab for the component draws of bhmm_gmm_path_components: b.tab takes the means of every
    // moments call)
    if ((rc = g.tab.ensure(tab.size())))
        return rc;
    if (want_resp && (rc = g.resp.ensure((size_t)b.total * b.n * M)))
        return rc;
    BHMM_HIP(hipMemcpyAsync(g.tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (hipEvent_t &e : b.ev)
        if (!e)
            BHMM_HIP(hipEventCreate(&e));
    BHMM_HIP(hipEventRecord(b.ev[0], c->stream));
    if ((rc = run_rows(c->stream, b.X.p, b.total, b.D, b.n, M, cov_type, g.tab.p, b.rows.p, b.m.p, nullptr,
                       want_resp ? g.resp.p : nullptr)))
        return rc;
    BHMM_HIP(mvn_launch_shift(c));
    BHMM_HIP(hipEventRecord(b.ev[1], c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream)); // (tab is a temporary; the re-load below waits for the stream anyway)
    (void)hipEventElapsedTime(&b.rows_ms, b.ev[0], b.ev[1]);
    const auto t0 = std::chrono::steady_clock::now();
    b.reloading = true;
    rc = bhmm_ctx_set_observations(c, BHMM_EMIT_EXPLICIT, b.rows.p, b.offsets.data(), b.K, b.n, 0, b.chunk, 1);
    b.reloading = false;
    b.reload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc)
        return rc;
    b.rows_valid = true;
    g.M = M;
    g.cov_type = cov_type;
    g.resp_log = g.resp_any = want_resp != 0;
    return BHMM_OK;
}

int bhmm_gmm_fetch_resp(bhmm_ctx *c, double *out)
{
    if (!c || !c->mvn.active || !c->mvn.rows_valid || !c->gmm.resp_any)
        return invalid_arg("bhmm_gmm_fetch_resp: no bhmm_gmm_emissions with want_resp has run on these observations");
    if (!out)
        return invalid_arg("bhmm_gmm_fetch_resp: out == NULL");
    auto &b = c->mvn;
    BHMM_HIP(hipSetDevice(c->device));
    BHMM_HIP(hipMemcpyAsync(out, c->gmm.resp.p, (size_t)b.total * b.n * c->gmm.M * sizeof(double),
                            hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    return BHMM_OK;
}

int bhmm_gmm_moments(bhmm_ctx *c, const double *gamma_dev, const double *means, int cov_type, double *out)
{
    if (!c || !c->mvn.active)
        return invalid_arg("bhmm_gmm_moments: no multivariate observations loaded");
    if (!gamma_dev || !means || !out)
        return invalid_arg("bhmm_gmm_moments: gamma_dev / means / out == NULL");
    auto &b = c->mvn;
    auto &g = c->gmm;
    if (!b.rows_valid || !g.resp_log)
        return invalid_arg("bhmm_gmm_moments: the last emissions were not bhmm_gmm_emissions with want_resp (or their "
                           "responsibilities have been turned into weights already)");
    const int nm = b.n * g.M;
    if (int rc = mvn_shape_ok("bhmm_gmm_moments", nm, b.D, cov_type))
        return rc;
    BHMM_HIP(hipSetDevice(c->device));
    for (hipEvent_t &e : g.ev)
        if (!e)
            BHMM_HIP(hipEventCreate(&e));
    const int64_t count = b.total * nm;
    const unsigned blocks = (unsigned)std::min<int64_t>((count + WEIGHTS_THREADS - 1) / WEIGHTS_THREADS, 1 << 20);
    g.resp_log = false; // (whatever happens below, the buffer holds log responsibilities no more)
    BHMM_HIP(hipEventRecord(g.ev[0], c->stream));
    BHMM_HIP(launch(k_gmm_weights, dim3(blocks), dim3(WEIGHTS_THREADS), 0, c->stream, g.resp.p, gamma_dev, count, g.M));
    BHMM_HIP(hipEventRecord(g.ev[1], c->stream));
    const int rc = mvn_run_moments(c, g.resp.p, nm, means, cov_type, out);
    if (!rc)
        (void)hipEventElapsedTime(&g.weights_ms, g.ev[0], g.ev[1]);
    return rc;
}

int bhmm_gmm_path_components(bhmm_ctx *c, const void *paths, int path_u8, int paths_on_device, uint64_t seed,
                             int32_t *labels, double *moments)
{
    if (!mixture_loaded(c))
        return invalid_arg("bhmm_gmm_path_components: the last emissions on these observations were not "
                           "bhmm_gmm_emissions");
    if (!paths || !moments)
        return invalid_arg("bhmm_gmm_path_components: paths / moments == NULL");
    auto &b = c->mvn;
    if (path_u8 && b.n > 256) // (every byte is a state then; the int32 form holds the others)
        return invalid_arg("bhmm_gmm_path_components: one byte per step holds at most 256 states (use the int32 form)");
    BHMM_HIP(hipSetDevice(c->device));
    if (paths_on_device) {
        if (reinterpret_cast<uintptr_t>(paths) % 16)
            return invalid_arg("bhmm_gmm_path_components: a device path must be aligned to 16 bytes");
        return run_components(c, "bhmm_gmm_path_components", paths, path_u8, seed, labels, moments);
    }
    const size_t bytes = (size_t)b.total * (path_u8 ? sizeof(uint8_t) : sizeof(int32_t));
    if (int rc = b.path.ensure(bytes))
        return rc;
    BHMM_HIP(hipMemcpyAsync(b.path.p, paths, bytes, hipMemcpyHostToDevice, c->stream));
    return run_components(c, "bhmm_gmm_path_components", b.path.p, path_u8, seed, labels, moments);
}

int bhmm_gmm_sample_paths(bhmm_ctx *c, const double *A, const double *pi, const double *u, uint64_t seed,
                          int32_t *paths, int32_t *labels, int64_t *counts, int64_t *n0, double *moments)
{
    if (!mixture_loaded(c))
        return invalid_arg("bhmm_gmm_sample_paths: the last emissions on these observations were not "
                           "bhmm_gmm_emissions");
    if (!A || !pi || !moments)
        return invalid_arg("bhmm_gmm_sample_paths: A / pi / moments == NULL");
    auto &b = c->mvn;
    if (c->n != b.n || c->total != b.total)
        return invalid_arg("bhmm_gmm_sample_paths: the loaded emission rows are not those of the multivariate set");
    // the draw leaves its int32 path at the front of c->d_scratch2 (keep_path, as for bhmm_mvn_sample_paths) ...
    c->keep_path = true;
    const int rc = bhmm_sample_paths(c, A, pi, nullptr, nullptr, u, seed, paths, counts, n0, nullptr);
    c->keep_path = false;
    if (rc)
        return rc;
    // ... where the components are drawn and their moments taken, before anything else uses that buffer
    return run_components(c, "bhmm_gmm_sample_paths", c->d_scratch2.p, 0, seed, labels, moments);
}

int bhmm_logpdf_gmm(double *logp, const double *X, int64_t T, int D, int N, int M, const double *weights,
                    const double *means, const double *covs, int cov_type)
{
    if (!logp || !X || !weights || !means || !covs || T < 1)
        return invalid_arg("bhmm_logpdf_gmm: NULL argument or empty problem");
    int rc;
    if ((rc = mvn_shape_ok("bhmm_logpdf_gmm", N, D, cov_type)))
        return rc;
    std::vector<double> tab;
    if ((rc = make_table("bhmm_logpdf_gmm", N, M, D, cov_type, weights, means, covs, tab)))
        return rc;
    MvnTmp tmp;
    double *dX, *dtab, *dl;
    if ((rc = tmp.alloc(&dX, (size_t)T * D)) || (rc = tmp.alloc(&dtab, tab.size())) || (rc = tmp.alloc(&dl, (size_t)T * N)))
        return rc;
    BHMM_HIP(hipMemcpy(dX, X, (size_t)T * D * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(dtab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = run_rows(nullptr, dX, T, D, N, M, cov_type, dtab, nullptr, nullptr, dl, nullptr))) // (L alone)
        return rc;
    BHMM_HIP(hipMemcpy(logp, dl, (size_t)T * N * sizeof(double), hipMemcpyDeviceToHost));
    return BHMM_OK;
}

} // extern "C"
