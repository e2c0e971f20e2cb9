// pois_api.hip -- Poisson count emissions (bhmm_pois_emissions, bhmm_logpdf_poisson): kernel in pois_kernels.hpp,
// DESIGN.md section 27.
//
// The kind runs on the observations bhmm_ctx_set_observations_mvn keeps in c->mvn.X (counts held as doubles).
// bhmm_pois_emissions makes the rows, the step scales m_t + c_t and the shifts where bhmm_mvn_emissions makes those of
// gaussians -- the same buffers, the same re-load as explicit observations -- so everything after it
// (bhmm_mvn_fetch_scale, bhmm_mvn_fetch_rows, bhmm_mvn_moments, bhmm_mvn_path_moments, every context call with
// par0 = par1 = NULL) is unchanged.
#include <math.h>

#include <chrono>
#include <string>
#include <vector>

#include "host_internal.hpp"
#include "launch.hpp"
#include "mvn_host.hpp"
#include "pois_kernels.hpp"

namespace bhmm {
namespace {

using namespace pois;

// log(k!) for k < LFACT: a running long double sum of log k, every entry rounded once
const double *log_factorials()
{
    static const std::vector<double> lf = [] {
        std::vector<double> v(LFACT);
        long double acc = 0.0L;
        for (int k = 0; k < LFACT; ++k) {
            if (k > 1)
                acc += logl((long double)k);
            v[k] = (double)acc;
        }
        return v;
    }();
    return lf.data();
}

// [log lambda | Lambda | log k!] of n states, validated; BHMM_ERR_INVALID
int make_table(const char *who, int n, int D, const double *rates, std::vector<double> &tab)
{
    tab.resize(table_size(n, D));
    double *loglam = tab.data(), *Lam = loglam + (size_t)n * D, *lf = Lam + n;
    for (int i = 0; i < n; ++i) {
        double sum = 0.0; // (ascending d, in double: what a restatement of the kernel forms)
        for (int d = 0; d < D; ++d) {
            const double r = rates[(size_t)i * D + d];
            if (!std::isfinite(r) || r < 0.0)
                return invalid_arg(std::string(who) + ": a rate is negative or not finite");
            // log lambda in long double, rounded once; -inf for a rate of zero
            loglam[(size_t)i * D + d] = r > 0.0 ? (double)logl((long double)r) : -INFINITY;
            sum += r;
        }
        Lam[i] = sum;
    }
    const double *src = log_factorials();
    for (int k = 0; k < LFACT; ++k)
        lf[k] = src[k];
    return BHMM_OK;
}

int run_rows(hipStream_t stream, const double *X, int64_t total, int D, int n, const double *tab, double *rows,
             double *scale, double *logp, unsigned int *status)
{
    if ((total + ROWS_THREADS - 1) / ROWS_THREADS > 0x7fffffff)
        return invalid_arg("poisson emissions: more steps than a grid has workgroups");
    const dim3 grid((unsigned)((total + ROWS_THREADS - 1) / ROWS_THREADS)), block(ROWS_THREADS);
#define BHMM_POIS_ROWS(DMAX) launch(k_pois_rows<DMAX>, grid, block, 0, stream, X, total, D, n, tab, rows, scale, logp, status)
    if (D <= 2)
        BHMM_HIP(BHMM_POIS_ROWS(2));
    else if (D <= 4)
        BHMM_HIP(BHMM_POIS_ROWS(4));
    else if (D <= 8)
        BHMM_HIP(BHMM_POIS_ROWS(8));
    else if (D <= 16)
        BHMM_HIP(BHMM_POIS_ROWS(16));
    else if (D <= 32)
        BHMM_HIP(BHMM_POIS_ROWS(32));
    else
        BHMM_HIP(BHMM_POIS_ROWS(64));
#undef BHMM_POIS_ROWS
    return BHMM_OK;
}

int bad_counts(const char *who, unsigned int status)
{
    return invalid_arg(std::string(who) + ": the observations hold a count that is " +
                       (status & BAD_NEGATIVE ? "negative" : "not an integer"));
}

} // namespace
} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_pois_emissions(bhmm_ctx *c, const double *rates)
{
    if (!c || !c->mvn.active)
        return invalid_arg("bhmm_pois_emissions: no multivariate observations loaded");
    if (!rates)
        return invalid_arg("bhmm_pois_emissions: rates == NULL");
    auto &b = c->mvn;
    int rc;
    if ((rc = mvn_shape_ok("bhmm_pois_emissions", b.n, b.D, BHMM_COV_DIAG)))
        return rc;
    std::vector<double> tab;
    if ((rc = make_table("bhmm_pois_emissions", b.n, b.D, rates, tab)))
        return rc;
    BHMM_HIP(hipSetDevice(c->device));
    b.rows_valid = false;
    c->gmm.forget(); // (the rows are not a mixture's any more)
    // (the status word is the one of the path moments: both calls are synchronous and clear it first)
    if ((rc = b.tab.ensure(tab.size())) || (rc = b.path_status.ensure(1)))
        return rc;
    BHMM_HIP(hipMemcpyAsync(b.tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemsetAsync(b.path_status.p, 0, sizeof(unsigned int), c->stream));
    for (hipEvent_t &e : b.ev)
        if (!e)
            BHMM_HIP(hipEventCreate(&e));
    BHMM_HIP(hipEventRecord(b.ev[0], c->stream));
    if ((rc = run_rows(c->stream, b.X.p, b.total, b.D, b.n, b.tab.p, b.rows.p, b.m.p, nullptr, b.path_status.p)))
        return rc;
    BHMM_HIP(mvn_launch_shift(c));
    BHMM_HIP(hipEventRecord(b.ev[1], c->stream));
    unsigned int status = 0;
    BHMM_HIP(hipMemcpyAsync(&status, b.path_status.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream)); // (tab is a temporary; the re-load below waits for the stream anyway)
    (void)hipEventElapsedTime(&b.rows_ms, b.ev[0], b.ev[1]);
    if (status)
        return bad_counts("bhmm_pois_emissions", status); // nothing is loaded
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

int bhmm_logpdf_poisson(double *logp, const double *X, int64_t T, int D, int N, const double *rates)
{
    if (!logp || !X || !rates || T < 1)
        return invalid_arg("bhmm_logpdf_poisson: NULL argument or empty problem");
    int rc;
    if ((rc = mvn_shape_ok("bhmm_logpdf_poisson", N, D, BHMM_COV_DIAG)))
        return rc;
    std::vector<double> tab;
    if ((rc = make_table("bhmm_logpdf_poisson", N, D, rates, tab)))
        return rc;
    MvnTmp tmp;
    double *dX, *dtab, *dl, *dst;
    if ((rc = tmp.alloc(&dX, (size_t)T * D)) || (rc = tmp.alloc(&dtab, tab.size())) ||
        (rc = tmp.alloc(&dl, (size_t)T * N)) || (rc = tmp.alloc(&dst, 1)))
        return rc;
    unsigned int *dstatus = reinterpret_cast<unsigned int *>(dst), status = 0;
    BHMM_HIP(hipMemcpy(dX, X, (size_t)T * D * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(dtab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemset(dst, 0, sizeof(double)));
    if ((rc = run_rows(nullptr, dX, T, D, N, dtab, nullptr, nullptr, dl, dstatus))) // (l + c alone: no rows, no scale)
        return rc;
    BHMM_HIP(hipMemcpy(&status, dstatus, sizeof(unsigned int), hipMemcpyDeviceToHost));
    if (status)
        return bad_counts("bhmm_logpdf_poisson", status);
    BHMM_HIP(hipMemcpy(logp, dl, (size_t)T * N * sizeof(double), hipMemcpyDeviceToHost));
    return BHMM_OK;
}

} // extern "C"
