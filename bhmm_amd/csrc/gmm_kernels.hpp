// gmm_kernels.hpp -- gaussian-mixture emissions per state: the two passes over D-dimensional observations that the
// mixture adds to those of mvn_kernels.hpp (gmm_api.hip).  n states, M components each,
// b_i(x) = sum_c w_ic N(x; mu_ic, Sigma_ic).
//
//   k_gmm_rows     L_ti = log b_i(x_t) by an online log-sum-exp over a_tic = log w_ic + l_tic, l_tic the arithmetic of
//                  k_mvn_rows (mvn::log_density) on the table entry of component (i, c).  Writes m_t = max_i L_ti, the
//                  row exp(L_ti - m_t) (largest entry of a finite row exactly 1.0), when asked L_ti, and when asked
//                  the log responsibilities log r_t(i,c) = a_tic - L_ti.
//   k_gmm_weights  u_t(i,c) = gamma_t(i) exp(log r_t(i,c)), in place over the log responsibilities: the weights
//                  k_mvn_moments takes over n M columns.
//
// k_gmm_rows has the shape of k_mvn_rows: one lane per step, mvn::ROWS_THREADS steps per workgroup, x_t staged through
// LDS once and kept in registers, the table [mu | W | c | log w] of the n M components read at wave-uniform addresses.
// Per state a lane keeps a running maximum and a rescaled sum -- two registers whatever M is.  A component of weight
// zero (log w = -inf, uniform) is skipped.  The L of a block of states go through LDS so that rows are written in
// whole lines; with more states than a block the raw L is parked in the row and the workgroup rescales its own rows
// at the end, as k_mvn_rows does with l.
// With responsibilities the raw a_tic go out the same way, GMM_NA columns of the (total, n M) buffer at a time through
// the upper half of the staging buffer (the blocks of states then take the lower half: GMM_NA states), and at the
// end the workgroup normalises its own rows: a thread takes the M values of one (step, state), their maximum a* and
// s = sum_c exp(a_c - a*), and leaves (a_c - a*) - log s.  This is a_tic - L_ti with the normaliser formed from the
// stored values themselves, so sum_c exp(log r) = 1 to a few ulp whatever the size of L_ti (a_tic - fl(L_ti) would
// carry the rounding of L_ti, eps |L_ti|, into every component alike).
#pragma once
#include "mvn_density.hpp"

namespace bhmm {
namespace gmm {

using mvn::ROWS_NB;
using mvn::ROWS_THREADS;
using mvn::X_PIECE;

constexpr int GMM_NA = ROWS_NB / 2; // columns of a_tic staged at a time, and states per block then
constexpr int WEIGHTS_THREADS = 256;

// tab: [mu nm*D | W nm*factor_size | c nm | log w nm], nm = n * M, component (i, c) at i * M + c.  rows [total][n] and
// m [total], or both nullptr; logp [total][n] or nullptr; resp [total][nm] or nullptr.
template <int DMAX, bool DIAG>
__global__ __launch_bounds__(ROWS_THREADS) void k_gmm_rows(const double *__restrict__ X, int64_t total, int D, int n,
                                                           int M, const double *__restrict__ tab, double *rows,
                                                           double *__restrict__ m_out, double *__restrict__ logp,
                                                           double *resp)
{
    __shared__ double s_l[ROWS_NB * ROWS_THREADS];
    __shared__ double s_m[ROWS_THREADS];
    const int nm = n * M;
    const size_t fs = mvn::factor_size(D, DIAG);
    const double *mu = tab, *W = tab + (size_t)nm * D, *cst = W + (size_t)nm * fs, *lw = cst + nm;
    const int64_t t0 = (int64_t)blockIdx.x * ROWS_THREADS;
    const int64_t t = t0 + threadIdx.x;
    const int steps = (int)(total - t0 < ROWS_THREADS ? total - t0 : ROWS_THREADS);
    const bool active = t < total;
    const int NB = resp ? GMM_NA : ROWS_NB; // states per block
    double *s_a = s_l + GMM_NA * ROWS_THREADS;
    const bool park = rows && n > NB; // the raw L waits in the row until m_t is known
    double m = -INFINITY;

    // the lane's observation, as in k_mvn_rows
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

    int q0 = 0, qa = 0; // the columns q0 .. q0 + qa - 1 of a wait in s_a (uniform)
    for (int i0 = 0; i0 < n; i0 += NB) {
        const int nb = n - i0 < NB ? n - i0 : NB;
        for (int j = 0; j < nb; ++j) {
            const int i = i0 + j;
            double mx = -INFINITY, s = 0.0; // online log-sum-exp: s = sum_c exp(a_c - mx)
            for (int c = 0; c < M; ++c) {
                const int q = i * M + c;
                const double lwq = lw[q];
                double a = -INFINITY;
                if (lwq != -INFINITY) { // (uniform: a component of weight zero is not evaluated)
                    a = lwq + mvn::log_density<DMAX, DIAG>(x, D, mu + (size_t)q * D, W + (size_t)q * fs, cst[q]);
                    if (a != -INFINITY) { // (a density that underflowed to nothing adds nothing; NaN goes on)
                        const bool up = a > mx;
                        const double e = exp(up ? mx - a : a - mx);
                        s = up ? fma(s, e, 1.0) : s + e;
                        mx = up ? a : mx;
                    }
                }
                if (resp) {
                    s_a[qa * ROWS_THREADS + threadIdx.x] = a;
                    if (++qa == GMM_NA || q == nm - 1) { // the staged columns, qa contiguous doubles per step
                        __syncthreads();
                        for (int e = threadIdx.x; e < steps * qa; e += ROWS_THREADS) {
                            const int sp = e / qa, k = e - sp * qa;
                            resp[(size_t)(t0 + sp) * nm + q0 + k] = s_a[k * ROWS_THREADS + sp];
                        }
                        __syncthreads();
                        q0 += qa;
                        qa = 0;
                    }
                }
            }
            const double L = mx + log(s);
            s_l[j * ROWS_THREADS + threadIdx.x] = L;
            m = mvn::nan_max(m, L);
        }
        if (!park)
            s_m[threadIdx.x] = m;
        __syncthreads();
        for (int e = threadIdx.x; e < steps * nb; e += ROWS_THREADS) {
            const int sp = e / nb, j = e - sp * nb;
            const size_t at = (size_t)(t0 + sp) * n + i0 + j;
            const double L = s_l[j * ROWS_THREADS + sp];
            if (logp)
                logp[at] = L;
            if (rows)
                rows[at] = park ? L : exp(L - s_m[sp]);
        }
        __syncthreads(); // (s_l is written again)
    }
    if (park) { // the workgroup's own rows again: L -> exp(L - m_t)
        s_m[threadIdx.x] = m;
        __syncthreads(); // (also orders the rows written above before the reads below, within the workgroup)
        double *r = rows + (size_t)t0 * n;
        for (size_t e = threadIdx.x; e < (size_t)steps * n; e += ROWS_THREADS)
            r[e] = exp(r[e] - s_m[e / n]);
    }
    if (resp) { // the workgroup's own a again: the M values of (step, state) p lie at p * M
        __syncthreads(); // (orders the a written above before the reads below, within the workgroup)
        double *r = resp + (size_t)t0 * nm;
        for (int p = threadIdx.x; p < steps * n; p += ROWS_THREADS) {
            double *v = r + (size_t)p * M;
            double mx = -INFINITY;
            for (int c = 0; c < M; ++c)
                mx = mvn::nan_max(mx, v[c]);
            double s = 0.0;
            for (int c = 0; c < M; ++c)
                if (v[c] != -INFINITY)
                    s += exp(v[c] - mx);
            const double ls = log(s);
            for (int c = 0; c < M; ++c)
                v[c] = (v[c] - mx) - ls;
        }
    }
    if (active && m_out)
        m_out[t] = m;
}

// u[t][i * M + c] = gam[t][i] * exp(u[t][i * M + c]) for count = total * n * M elements
__global__ __launch_bounds__(WEIGHTS_THREADS) void k_gmm_weights(double *__restrict__ u,
                                                                 const double *__restrict__ gam, int64_t count, int M)
{
    const int64_t stride = (int64_t)gridDim.x * WEIGHTS_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * WEIGHTS_THREADS + threadIdx.x; e < count; e += stride)
        u[e] = gam[e / M] * exp(u[e]);
}

} // namespace gmm
} // namespace bhmm
