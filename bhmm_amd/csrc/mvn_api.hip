// mvn_api.hip -- multivariate gaussian emissions (bhmm_ctx_set_observations_mvn, bhmm_mvn_emissions,
// bhmm_mvn_fetch_scale, bhmm_mvn_fetch_rows, bhmm_mvn_moments, bhmm_mvn_path_moments, bhmm_mvn_sample_paths,
// bhmm_logpdf_mvn): kernels in mvn_kernels.hpp, the factorisation on the host (host::mvn_prepare, host_model.cpp);
// DESIGN.md sections 23 and 24.
// The checks of shapes and parameters, the launcher of the moment kernels for any column count and the shift launch
// are declared in mvn_host.hpp: gmm_api.hip (mixtures per state) calls them too.
//
// The recursions know nothing of this kind.  bhmm_mvn_emissions turns the observations kept in c->mvn.X into scaled
// emission rows in c->mvn.rows and hands those to bhmm_ctx_set_observations as BHMM_EMIT_EXPLICIT observations on the
// device -- the public entry point, nothing of the chunk layouts is touched here -- so every context call then works
// with par0 = par1 = NULL.  c->mvn.* outlives that re-load (c->mvn.reloading tells bhmm_ctx_set_observations that
// the call is ours); bhmm_ctx_destroy frees it with the context.
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "host_internal.hpp"
#include "host_model.hpp"
#include "launch.hpp"
#include "mvn_host.hpp"
#include "mvn_kernels.hpp"

namespace bhmm {

using namespace mvn;

int mvn_shape_ok(const char *who, int n, int D, int cov_type)
{
    if (n < 1 || n > 4096)
        return invalid_arg(std::string(who) + ": 1..4096 hidden states are supported");
    if (D < 1 || D > BHMM_MVN_MAX_D)
        return invalid_arg(std::string(who) + ": 1 <= D <= " + std::to_string(BHMM_MVN_MAX_D) + " dimensions");
    if (cov_type != BHMM_COV_FULL && cov_type != BHMM_COV_DIAG)
        return invalid_arg(std::string(who) + ": cov_type is BHMM_COV_FULL or BHMM_COV_DIAG");
    return BHMM_OK;
}

int mvn_make_table(const char *who, int n, int D, int cov_type, const double *means, const double *covs,
                   std::vector<double> &tab)
{
    for (size_t e = 0; e < (size_t)n * D; ++e)
        if (!std::isfinite(means[e]))
            return invalid_arg(std::string(who) + ": a mean is not finite");
    const size_t fs = factor_size(D, cov_type == BHMM_COV_DIAG);
    tab.resize((size_t)n * D + (size_t)n * fs + n);
    memcpy(tab.data(), means, (size_t)n * D * sizeof(double));
    return host::mvn_prepare(n, D, cov_type, covs, nullptr, tab.data() + (size_t)n * D,
                             tab.data() + (size_t)n * D + (size_t)n * fs);
}

hipError_t mvn_launch_shift(bhmm_ctx *c)
{
    auto &b = c->mvn;
    return launch(k_mvn_shift, dim3((unsigned)std::min(b.K, 65535)), dim3(SHIFT_THREADS), 0, c->stream, b.m.p,
                  b.d_offsets.p, b.K, b.shift.p);
}

// (c->mvn.tab: the table of the last emissions is not needed any more once the rows are made)
int mvn_run_moments(bhmm_ctx *c, const double *gamma_dev, int ncols, const double *means, int cov_type, double *out)
{
    auto &b = c->mvn;
    int rc;
    const bool diag = cov_type == BHMM_COV_DIAG;
    const int D = b.D, n = ncols;
    const int64_t ms = (int64_t)moment_stride(D, diag), E = (int64_t)n * ms;
    const int epb = (int)std::min<int64_t>(E, MOM_THREADS);
    const int64_t gy = (E + epb - 1) / epb;
    const int nsi_max = (int)std::min<int64_t>(n, (epb - 1) / ms + 2);
    const int64_t tiles = (b.total + MOM_TILE - 1) / MOM_TILE;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(tiles, MOM_MAX_GROUPS / gy));
    const int64_t span = (b.total + G - 1) / G;
    const size_t lds = ((size_t)MOM_TILE * (D + nsi_max) + MOM_THREADS) * sizeof(double);
    BHMM_HIP(hipSetDevice(c->device));
    if ((rc = b.part.ensure((size_t)G * E)) || (rc = b.out.ensure((size_t)E)) || (rc = b.tab.ensure((size_t)n * D)))
        return rc;
    BHMM_HIP(hipMemcpyAsync(b.tab.p, means, (size_t)n * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const dim3 grid((unsigned)G, (unsigned)gy), block(MOM_THREADS);
    for (hipEvent_t &e : b.ev)
        if (!e)
            BHMM_HIP(hipEventCreate(&e));
    BHMM_HIP(hipEventRecord(b.ev[2], c->stream));
    BHMM_HIP(diag ? launch(k_mvn_moments<true>, grid, block, lds, c->stream, b.X.p, gamma_dev, b.total, D, n, b.tab.p,
                           span, epb, nsi_max, b.part.p)
                  : launch(k_mvn_moments<false>, grid, block, lds, c->stream, b.X.p, gamma_dev, b.total, D, n, b.tab.p,
                           span, epb, nsi_max, b.part.p));
    BHMM_HIP(launch(k_mvn_moments_finish, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, c->stream, b.part.p, G, E,
                    b.out.p));
    BHMM_HIP(hipEventRecord(b.ev[3], c->stream));
    BHMM_HIP(hipMemcpyAsync(out, b.out.p, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    (void)hipEventElapsedTime(&b.moments_ms, b.ev[2], b.ev[3]);
    return BHMM_OK;
}

// Packed moments of the hard labels at path_dev (device; int32 or one byte per step) about the nlabels means into out
// (host): k_mvn_path_moments, one slab per workgroup, then k_mvn_moments_finish over the slabs.  The labels are the
// states of a hidden path (nlabels = n) or its components s_t M + c_t (nlabels = n M, gmm_api.hip); the means come
// from the host (means) or, means == NULL, lie on the device already (means_dev).  A label outside [0, nlabels) is
// found by the kernel before it indexes anything with it: BHMM_ERR_INVALID, nothing is delivered.
int mvn_run_path_moments(bhmm_ctx *c, const char *who, const void *path_dev, int path_u8, int nlabels,
                         const double *means, const double *means_dev, int cov_type, double *out)
{
    auto &b = c->mvn;
    const bool diag = cov_type == BHMM_COV_DIAG;
    const int D = b.D, n = nlabels;
    const int mode = diag ? PM_ELEM_DIAG : (D >= PM_BLOCK_MIN_D ? PM_BLOCK : PM_ELEM_FULL);
    const size_t E = (size_t)n * moment_stride(D, diag);
    const PmPlan pl = pm_plan(b.total, D, n, mode);
    int rc;
    if ((rc = b.part.ensure((size_t)pl.groups * E)) || (rc = b.out.ensure(E)) ||
        (means && (rc = b.tab.ensure((size_t)n * D))) || (rc = b.path_status.ensure(1)))
        return rc;
    // (the table of the last bhmm_mvn_emissions is not needed any more: the rows are made)
    if (means)
        BHMM_HIP(hipMemcpyAsync(b.tab.p, means, (size_t)n * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double *mu_dev = means ? b.tab.p : means_dev;
    BHMM_HIP(hipMemsetAsync(b.path_status.p, 0, sizeof(unsigned int), c->stream));
    for (hipEvent_t &e : b.ev)
        if (!e)
            BHMM_HIP(hipEventCreate(&e));
    BHMM_HIP(hipEventRecord(b.ev[4], c->stream));
    if (!pl.slab_lds) // the slabs are accumulated where they lie
        BHMM_HIP(hipMemsetAsync(b.part.p, 0, (size_t)pl.groups * E * sizeof(double), c->stream));
    const dim3 grid((unsigned)pl.groups), block(PM_THREADS);
#define BHMM_MVN_PM(PT, MODE)                                                                                          \
    launch(k_mvn_path_moments<PT, MODE>, grid, block, pl.lds, c->stream, b.X.p, static_cast<const PT *>(path_dev),      \
           b.total, D, n, mu_dev, pl, b.part.p, b.path_status.p)
#define BHMM_MVN_PM_MODE(PT)                                                                                           \
    (mode == PM_BLOCK ? BHMM_MVN_PM(PT, PM_BLOCK) : mode == PM_ELEM_DIAG ? BHMM_MVN_PM(PT, PM_ELEM_DIAG)               \
                                                                         : BHMM_MVN_PM(PT, PM_ELEM_FULL))
    BHMM_HIP(path_u8 ? BHMM_MVN_PM_MODE(uint8_t) : BHMM_MVN_PM_MODE(int32_t));
#undef BHMM_MVN_PM_MODE
#undef BHMM_MVN_PM
    BHMM_HIP(launch(k_mvn_moments_finish, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, c->stream, b.part.p, pl.groups,
                    (int64_t)E, b.out.p));
    BHMM_HIP(hipEventRecord(b.ev[5], c->stream));
    std::vector<double> res(E);
    unsigned int status = 0;
    BHMM_HIP(hipMemcpyAsync(res.data(), b.out.p, E * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipMemcpyAsync(&status, b.path_status.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    (void)hipEventElapsedTime(&b.path_moments_ms, b.ev[4], b.ev[5]);
    if (status & PM_BAD_STATE)
        return invalid_arg(std::string(who) + ": the path holds a " + (n == b.n ? "state" : "label") + " outside [0, " +
                           std::to_string(n) + ")");
    memcpy(out, res.data(), E * sizeof(double));
    return BHMM_OK;
}

namespace {

template <bool DIAG>
hipError_t launch_rows(hipStream_t stream, const double *X, int64_t total, int D, int n, const double *tab,
                       double *rows, double *m, double *logp)
{
    const dim3 grid((unsigned)((total + ROWS_THREADS - 1) / ROWS_THREADS)), block(ROWS_THREADS);
#define BHMM_MVN_ROWS(DMAX) launch(k_mvn_rows<DMAX, DIAG>, grid, block, 0, stream, X, total, D, n, tab, rows, m, logp)
    if (D <= 2)
        return BHMM_MVN_ROWS(2);
    if (D <= 4)
        return BHMM_MVN_ROWS(4);
    if (D <= 8)
        return BHMM_MVN_ROWS(8);
    if (D <= 16)
        return BHMM_MVN_ROWS(16);
    if (D <= 32)
        return BHMM_MVN_ROWS(32);
    return BHMM_MVN_ROWS(64);
#undef BHMM_MVN_ROWS
}

int run_rows(hipStream_t stream, const double *X, int64_t total, int D, int n, int cov_type, const double *tab,
             double *rows, double *m, double *logp)
{
    if ((total + ROWS_THREADS - 1) / ROWS_THREADS > 0x7fffffff)
        return invalid_arg("multivariate gaussian emissions: more steps than a grid has workgroups");
    BHMM_HIP(cov_type == BHMM_COV_DIAG ? launch_rows<true>(stream, X, total, D, n, tab, rows, m, logp)
                                       : launch_rows<false>(stream, X, total, D, n, tab, rows, m, logp));
    return BHMM_OK;
}

} // namespace
} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_ctx_set_observations_mvn(bhmm_ctx *c, const double *X, const int64_t *offsets, int K, int D, int nstates,
                                  int chunk, int obs_on_device)
{
    if (!c || !X || !offsets || K < 1)
        return invalid_arg("bhmm_ctx_set_observations_mvn: bad context / X / offsets / K");
    if (int rc = mvn_shape_ok("bhmm_ctx_set_observations_mvn", nstates, D, BHMM_COV_FULL))
        return rc;
    for (int k = 0; k < K; ++k)
        if (offsets[k + 1] < offsets[k])
            return invalid_arg("bhmm_ctx_set_observations_mvn: offsets must be non-decreasing");
    const int64_t total = offsets[K] - offsets[0];
    if (total <= 0)
        return invalid_arg("bhmm_ctx_set_observations_mvn: no observations");
    BHMM_HIP(hipSetDevice(c->device));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    auto &b = c->mvn;
    b.active = b.rows_valid = false;
    c->gmm.forget();
    c->kind = -1; // (whatever was loaded before is not what the caller means any more: no model call until the
                  // first bhmm_mvn_emissions)
    int rc;
    if ((rc = b.X.ensure((size_t)total * D)) || (rc = b.rows.ensure((size_t)total * nstates)) ||
        (rc = b.m.ensure((size_t)total)) || (rc = b.shift.ensure((size_t)K)) || (rc = b.d_offsets.ensure((size_t)K + 1)))
        return rc;
    b.offsets.resize((size_t)K + 1);
    for (int k = 0; k <= K; ++k) // positions relative to the first step handed over
        b.offsets[k] = offsets[k] - offsets[0];
    BHMM_HIP(hipMemcpyAsync(b.X.p, X + (size_t)offsets[0] * D, (size_t)total * D * sizeof(double),
                            obs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(b.d_offsets.p, b.offsets.data(), ((size_t)K + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                            c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    b.D = D;
    b.n = nstates;
    b.K = K;
    b.chunk = chunk;
    b.total = total;
    b.active = true;
    return BHMM_OK;
}

int bhmm_mvn_emissions(bhmm_ctx *c, const double *means, const double *covs, int cov_type)
{
    if (!c || !c->mvn.active)
        return invalid_arg("bhmm_mvn_emissions: no multivariate observations loaded");
    if (!means || !covs)
        return invalid_arg("bhmm_mvn_emissions: means / covs == NULL");
    auto &b = c->mvn;
    int rc;
    if ((rc = mvn_shape_ok("bhmm_mvn_emissions", b.n, b.D, cov_type)))
        return rc;
    std::vector<double> tab;
    if ((rc = mvn_make_table("bhmm_mvn_emissions", b.n, b.D, cov_type, means, covs, tab)))
        return rc;
    BHMM_HIP(hipSetDevice(c->device));
    b.rows_valid = false;
    c->gmm.forget(); // (the rows are not a mixture's any more)
    if ((rc = b.tab.ensure(tab.size())))
        return rc;
    BHMM_HIP(hipMemcpyAsync(b.tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (hipEvent_t &e : b.ev)
        if (!e)
            BHMM_HIP(hipEventCreate(&e));
    BHMM_HIP(hipEventRecord(b.ev[0], c->stream));
    if ((rc = run_rows(c->stream, b.X.p, b.total, b.D, b.n, cov_type, b.tab.p, b.rows.p, b.m.p, nullptr)))
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
    return BHMM_OK;
}

int bhmm_mvn_fetch_scale(bhmm_ctx *c, double *shift_k, double *m_t)
{
    if (!c || !c->mvn.active || !c->mvn.rows_valid)
        return invalid_arg("bhmm_mvn_fetch_scale: no bhmm_mvn_emissions has run on these observations");
    auto &b = c->mvn;
    BHMM_HIP(hipSetDevice(c->device));
    if (shift_k)
        BHMM_HIP(hipMemcpyAsync(shift_k, b.shift.p, (size_t)b.K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (m_t)
        BHMM_HIP(hipMemcpyAsync(m_t, b.m.p, (size_t)b.total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    return BHMM_OK;
}

int bhmm_mvn_fetch_rows(bhmm_ctx *c, double *rows)
{
    if (!c || !c->mvn.active || !c->mvn.rows_valid)
        return invalid_arg("bhmm_mvn_fetch_rows: no bhmm_mvn_emissions has run on these observations");
    if (!rows)
        return invalid_arg("bhmm_mvn_fetch_rows: rows == NULL");
    auto &b = c->mvn;
    BHMM_HIP(hipSetDevice(c->device));
    BHMM_HIP(hipMemcpyAsync(rows, b.rows.p, (size_t)b.total * b.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    return BHMM_OK;
}

int bhmm_mvn_moments(bhmm_ctx *c, const double *gamma_dev, const double *means, int cov_type, double *out)
{
    if (!c || !c->mvn.active)
        return invalid_arg("bhmm_mvn_moments: no multivariate observations loaded");
    if (!gamma_dev || !means || !out)
        return invalid_arg("bhmm_mvn_moments: gamma_dev / means / out == NULL");
    auto &b = c->mvn;
    int rc;
    if ((rc = mvn_shape_ok("bhmm_mvn_moments", b.n, b.D, cov_type)))
        return rc;
    return mvn_run_moments(c, gamma_dev, b.n, means, cov_type, out);
}

int bhmm_mvn_path_moments(bhmm_ctx *c, const void *paths, int path_u8, int paths_on_device, const double *means,
                          int cov_type, double *out)
{
    if (!c || !c->mvn.active)
        return invalid_arg("bhmm_mvn_path_moments: no multivariate observations loaded");
    if (!paths || !means || !out)
        return invalid_arg("bhmm_mvn_path_moments: paths / means / out == NULL");
    auto &b = c->mvn;
    if (int rc = mvn_shape_ok("bhmm_mvn_path_moments", b.n, b.D, cov_type))
        return rc;
    if (path_u8 && b.n > 256) // (every byte is a state then; the int32 form holds the others)
        return invalid_arg("bhmm_mvn_path_moments: one byte per step holds at most 256 states (use the int32 form)");
    BHMM_HIP(hipSetDevice(c->device));
    if (paths_on_device) {
        if (reinterpret_cast<uintptr_t>(paths) % 16)
            return invalid_arg("bhmm_mvn_path_moments: a device path must be aligned to 16 bytes");
        return mvn_run_path_moments(c, "bhmm_mvn_path_moments", paths, path_u8, b.n, means, nullptr, cov_type, out);
    }
    const size_t bytes = (size_t)b.total * (path_u8 ? sizeof(uint8_t) : sizeof(int32_t));
    if (int rc = b.path.ensure(bytes))
        return rc;
    BHMM_HIP(hipMemcpyAsync(b.path.p, paths, bytes, hipMemcpyHostToDevice, c->stream));
    return mvn_run_path_moments(c, "bhmm_mvn_path_moments", b.path.p, path_u8, b.n, means, nullptr, cov_type, out);
}

int bhmm_mvn_sample_paths(bhmm_ctx *c, const double *A, const double *pi, const double *u, uint64_t seed,
                          int32_t *paths, int64_t *counts, int64_t *n0, const double *means, int cov_type,
                          double *moments)
{
    if (!c || !c->mvn.active || !c->mvn.rows_valid)
        return invalid_arg("bhmm_mvn_sample_paths: no bhmm_mvn_emissions has run on these observations");
    if (!A || !pi || !means || !moments)
        return invalid_arg("bhmm_mvn_sample_paths: A / pi / means / moments == NULL");
    auto &b = c->mvn;
    if (int rc = mvn_shape_ok("bhmm_mvn_sample_paths", b.n, b.D, cov_type))
        return rc;
    if (c->n != b.n || c->total != b.total)
        return invalid_arg("bhmm_mvn_sample_paths: the loaded emission rows are not those of the multivariate set");
    // the draw leaves its int32 path at the front of c->d_scratch2 (sample_run<N>: because keep_path says so); it
    // crosses the link only when the caller wants it
    c->keep_path = true;
    const int rc = bhmm_sample_paths(c, A, pi, nullptr, nullptr, u, seed, paths, counts, n0, nullptr);
    c->keep_path = false;
    if (rc)
        return rc;
    // ... and is read here, before anything else uses that buffer
    return mvn_run_path_moments(c, "bhmm_mvn_sample_paths", c->d_scratch2.p, 0, b.n, means, nullptr, cov_type, moments);
}

int bhmm_logpdf_mvn(double *logp, const double *X, int64_t T, int D, int N, const double *means, const double *covs,
                    int cov_type)
{
    if (!logp || !X || !means || !covs || T < 1)
        return invalid_arg("bhmm_logpdf_mvn: NULL argument or empty problem");
    int rc;
    if ((rc = mvn_shape_ok("bhmm_logpdf_mvn", N, D, cov_type)))
        return rc;
    std::vector<double> tab;
    if ((rc = mvn_make_table("bhmm_logpdf_mvn", N, D, cov_type, means, covs, tab)))
        return rc;
    MvnTmp tmp;
    double *dX, *dtab, *dl;
    if ((rc = tmp.alloc(&dX, (size_t)T * D)) || (rc = tmp.alloc(&dtab, tab.size())) || (rc = tmp.alloc(&dl, (size_t)T * N)))
        return rc;
    BHMM_HIP(hipMemcpy(dX, X, (size_t)T * D * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(dtab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = run_rows(nullptr, dX, T, D, N, cov_type, dtab, nullptr, nullptr, dl))) // (l alone: no rows, no m_t)
        return rc;
    BHMM_HIP(hipMemcpy(logp, dl, (size_t)T * N * sizeof(double), hipMemcpyDeviceToHost));
    return BHMM_OK;
}

} // extern "C"
