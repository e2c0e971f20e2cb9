// pois_kernels.hpp -- Poisson count emissions: the pass that turns counts and rates into explicit emission rows
// (pois_api.hip).  Everything after it -- k_mvn_shift, the moment kernels, the recursions -- is
// what the multivariate gaussian kind runs (mvn_kernels.hpp).
//
//   k_pois_rows   l_ti = sum_d x_td log lambda_id - Lambda_i for every step t and state i (Lambda_i = sum_d lambda_id
//                 and log lambda from the host, log 0 = -inf), one explicit fma per channel in ascending d; a channel
//                 with x_td = 0 is skipped, so it contributes exactly 0 whatever the rate (never 0 * -inf), and a
//                 positive count under rate 0 gives -inf.  m_t = max_i l_ti, the row exp(l_ti - m_t) (the largest
//                 entry of a finite row is exp(0) = 1.0 exactly); a step every state gives -inf: a row of zeros and
//                 m_t = 0.  c_t = -sum_d log(x_td !) does not depend on the state: the step scale written is
//                 m_t + c_t, the log-density, when asked for, l_ti + c_t.  A NaN count makes row, scale and
//                 log-density NaN.  A count that is negative or not an integer sets a bit of *status, once per
//                 workgroup at most.
//
// The shape is that of k_mvn_rows: one lane per step, ROWS_THREADS steps per workgroup; the tile's counts come through
// LDS in skewed pieces; the per-state table is read at addresses uniform over the wavefront (scalar loads, the fma
// takes log lambda from a scalar register); the l of ROWS_NB states at a time go through LDS so that rows are written
// in whole cache lines; above ROWS_NB states the raw l is parked in the row and rescaled once m_t is known.
// log(k!) for k < LFACT comes from a table the host made in long double (one entry per thread into LDS); a larger
// count takes Stirling's series (log_factorial_large).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mvn_density.hpp"

namespace bhmm {
namespace pois {

using mvn::nan_max;
using mvn::ROWS_NB;
using mvn::ROWS_THREADS;
using mvn::X_PIECE;

constexpr int LFACT = 256; // entries of the log-factorial table: log(0!) .. log(255!)
static_assert(LFACT == ROWS_THREADS, "one table entry per thread");
constexpr unsigned int BAD_NEGATIVE = 1u;   // a count below zero
constexpr unsigned int BAD_FRACTION = 2u;   // a count that is not an integer (or infinite)

// log(v!) for v >= LFACT by Stirling's series, (v + 1/2) log v - v + log(2 pi) / 2 + 1 / (12 v) - 1 / (360 v^3) +
// 1 / (1260 v^5): the first term dropped, 1 / (1680 v^7), is below 1e-20 there.  One log and a dozen flops where an
// inlined lgamma per channel costs the widest instantiations a hundred registers more
__device__ __forceinline__ double log_factorial_large(double v)
{
    const double r = 1.0 / v, r2 = r * r;
    const double tail = r * fma(r2, fma(r2, 1.0 / 1260.0, -1.0 / 360.0), 1.0 / 12.0);
    return fma(v + 0.5, log(v), -v) + (0.91893853320467274178 + tail);
}

// doubles of the table: [log lambda n*D | Lambda n | log k! LFACT]
__host__ __device__ inline size_t table_size(int n, int D) { return (size_t)n * D + (size_t)n + LFACT; }

// rows [total][n] and scale [total], or both nullptr (only the log-density is wanted); logp [total][n] or nullptr
template <int DMAX>
__global__ __launch_bounds__(ROWS_THREADS) void k_pois_rows(const double *__restrict__ X, int64_t total, int D, int n,
                                                            const double *__restrict__ tab, double *rows,
                                                            double *__restrict__ scale_out, double *__restrict__ logp,
                                                            unsigned int *__restrict__ status)
{
    __shared__ double s_l[ROWS_NB * ROWS_THREADS];
    __shared__ double s_m[ROWS_THREADS];
    __shared__ double s_c[ROWS_THREADS];
    __shared__ double s_lf[LFACT];
    __shared__ unsigned int s_bad;
    const double *loglam = tab, *Lam = tab + (size_t)n * D;
    const int64_t t0 = (int64_t)blockIdx.x * ROWS_THREADS;
    const int64_t t = t0 + threadIdx.x;
    const int steps = (int)(total - t0 < ROWS_THREADS ? total - t0 : ROWS_THREADS);
    const bool active = t < total;
    const bool park = rows && n > ROWS_NB; // the raw l waits in the row until m_t is known
    double m = -INFINITY;

    s_lf[threadIdx.x] = Lam[n + threadIdx.x];
    if (threadIdx.x == 0)
        s_bad = 0u;
    // the lane's counts, in registers for every state: through LDS (s_l, free until the first state) in coalesced
    // pieces, skewed by one double per 32 (k_mvn_rows)
    double x[DMAX];
#pragma unroll
    for (int a = 0; a < DMAX; ++a)
        x[a] = 0.0;
    {
        const int tile_elems = steps * D;
        const double *Xt = X + (size_t)t0 * D;
        for (int p0 = 0; p0 < tile_elems; p0 += X_PIECE) {
            const int cnt = tile_elems - p0 < X_PIECE ? tile_elems - p0 : X_PIECE;
            for (int k = threadIdx.x; k < cnt; k += ROWS_THREADS)
                s_l[k + (k >> 5)] = Xt[p0 + k];
            __syncthreads();
#pragma unroll
            for (int a = 0; a < DMAX; ++a) {
                const int k = (int)threadIdx.x * D + a - p0;
                if (a < D && active && k >= 0 && k < cnt)
                    x[a] = s_l[k + (k >> 5)];
            }
            __syncthreads();
        }
    }

    // the checks of the counts and c_t = -sum_d log(x_td !); an inactive lane holds zeros
    double c = 0.0;
    unsigned int bad = 0u;
#pragma unroll
    for (int a = 0; a < DMAX; ++a) {
        if (a < D) { // (uniform)
            const double v = x[a];
            if (v < 0.0)
                bad |= BAD_NEGATIVE;
            else if (v == v && (v != floor(v) || v == INFINITY))
                bad |= BAD_FRACTION;
            if (v >= 0.0 && v < (double)LFACT)
                c -= s_lf[(int)v];
            else // (rare: a wavefront without such a count skips it; NaN stays NaN)
                c -= log_factorial_large(v);
        }
    }
    if (bad)
        atomicOr(&s_bad, bad); // (LDS; read after the barriers of the state loop)
    s_c[threadIdx.x] = c;

    for (int i0 = 0; i0 < n; i0 += ROWS_NB) {
        const int nb = n - i0 < ROWS_NB ? n - i0 : ROWS_NB;
        for (int j = 0; j < nb; ++j) {
            const int i = i0 + j;
            const double *ll = loglam + (size_t)i * D;
            double acc = 0.0;
#pragma unroll
            for (int a = 0; a < DMAX; ++a)
                if (a < D) // (uniform)
                    acc = x[a] != 0.0 ? fma(x[a], ll[a], acc) : acc;
            const double l = acc - Lam[i];
            s_l[j * ROWS_THREADS + threadIdx.x] = l;
            m = nan_max(m, l);
        }
        if (!park)
            s_m[threadIdx.x] = m == -INFINITY ? 0.0 : m;
        __syncthreads();
        // the block's [steps][nb] values, nb contiguous doubles per step
        for (int e = threadIdx.x; e < steps * nb; e += ROWS_THREADS) {
            const int s = e / nb, j = e - s * nb;
            const size_t at = (size_t)(t0 + s) * n + i0 + j;
            const double l = s_l[j * ROWS_THREADS + s];
            if (logp)
                logp[at] = l + s_c[s];
            if (rows)
                rows[at] = park ? l : exp(l - s_m[s]);
        }
        __syncthreads(); // (s_l is written again)
    }
    if (m == -INFINITY) // impossible under every state: a row of zeros, m_t = 0
        m = 0.0;
    if (park) { // the workgroup's own rows again: l -> exp(l - m_t)
        s_m[threadIdx.x] = m;
        __syncthreads(); // (also orders the rows written above before the reads below, within the workgroup)
        double *r = rows + (size_t)t0 * n;
        for (size_t e = threadIdx.x; e < (size_t)steps * n; e += ROWS_THREADS)
            r[e] = exp(r[e] - s_m[e / n]);
    }
    if (active && scale_out)
        scale_out[t] = m + c;
    if (threadIdx.x == 0 && s_bad)
        atomicOr(status, s_bad);
}

} // namespace pois
} // namespace bhmm
