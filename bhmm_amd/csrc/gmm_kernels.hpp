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
//   k_gmm_draw_components  (at the end of this file) the component of every step of a hidden path, for the Gibbs sweep.
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

// ---- the component of every step of a hidden path (the Gibbs sweep of mixtures) ----
//   k_gmm_draw_components  c_t ~ r_t(s_t, .) for a given path s, out as the label s_t M + c_t: what k_mvn_path_moments
//                          takes over n M labels.  Only the M densities of the state the path is in are formed; no
//                          (total, n M) buffer is read or written.
// The shape of k_gmm_rows again: one lane per step, x_t staged through LDS once and kept in registers.  The table reads
// of mvn::log_density must be uniform over the wavefront, the states of its 64 steps are not: the wavefront goes
// through the distinct states it holds, one round each -- s is the state of the first lane not yet served, the lanes
// with s_t == s run the component loop on the entries s M .. s M + M - 1 and retire.  A path stays 30 to 60 steps in
// a state, so this is two or three rounds; min(n, 64) at the worst.
// The draw is one pass with three registers.  Components in ascending order, those of weight zero skipped, with the
// running maximum a* and the rescaled sum s of k_gmm_rows' online log-sum-exp: e_c = exp(a_c - a*) after the update
// of a*, s the sum of the e so far in the same units.  The first component visited is the pick; a later one replaces
// it when u s < e_c, u = draw_uniform01(key, g M + c), g the position of the step in the random stream.  The pick
// ends as c with probability (e_c / s_c) prod_{c' > c} (1 - e_c' / s_c') = e_c / s_M (the product telescopes; the
// ratios do not depend on the unit a* the sums are kept in): the categorical draw from r_t(s_t, .).  A NaN never
// satisfies the comparison: the first component stays.
constexpr unsigned int DRAW_BAD_STATE = 1u;
constexpr uint64_t DRAW_KEY_CONST = 0xC3A5C85C97CB3127ull; // the component draws' stream: key = draw_mix64(seed ^ this)

__host__ __device__ inline uint64_t draw_mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t draw_key(uint64_t seed) { return draw_mix64(seed ^ DRAW_KEY_CONST); }
// uniform01 of path_kernels.hpp (the path draw's generator), restated: [0, 1) from the counter x of stream `key`
__device__ __forceinline__ double draw_uniform01(uint64_t key, uint64_t x)
{
    return (double)(draw_mix64(key + 0x9E3779B97F4A7C15ull * (x + 1)) >> 11) * (1.0 / 9007199254740992.0);
}

// path [total] (int32 or one byte per step), tab as for k_gmm_rows, off [K + 1] the trajectories' first steps, soff [K]
// their positions in the random stream or nullptr (the position of a step is its index then), labels [total].
// A path entry outside [0, n) sets *status, indexes nothing and leaves the label -1.
template <typename PT, int DMAX, bool DIAG>
__global__ __launch_bounds__(ROWS_THREADS) void k_gmm_draw_components(const double *__restrict__ X,
                                                                      const PT *__restrict__ path, int64_t total,
                                                                      int D, int n, int M,
                                                                      const double *__restrict__ tab,
                                                                      const int64_t *__restrict__ off,
                                                                      const int64_t *__restrict__ soff, int K,
                                                                      uint64_t key, int32_t *__restrict__ labels,
                                                                      unsigned int *status)
{
    __shared__ double s_x[X_PIECE + X_PIECE / 32];
    const int nm = n * M;
    const size_t fs = mvn::factor_size(D, DIAG);
    const double *mu = tab, *W = tab + (size_t)nm * D, *cst = W + (size_t)nm * fs, *lw = cst + nm;
    const int64_t t0 = (int64_t)blockIdx.x * ROWS_THREADS;
    const int64_t t = t0 + threadIdx.x;
    const int steps = (int)(total - t0 < ROWS_THREADS ? total - t0 : ROWS_THREADS);
    const bool active = t < total;

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
                s_x[k + (k >> 5)] = Xt[p0 + k];
            __syncthreads();
#pragma unroll
            for (int a = 0; a < DMAX; ++a) {
                const int k = (int)threadIdx.x * D + a - p0;
                if (a < D && active && k >= 0 && k < cnt)
                    x[a] = s_x[k + (k >> 5)];
            }
            __syncthreads();
        }
    }

    // the lane's state and the position of its step in the random stream
    int st = -1;
    uint64_t g = (uint64_t)t;
    if (active) {
        const int64_t v = (int64_t)path[t];
        if (v >= 0 && v < n)
            st = (int)v;
        else
            *status = DRAW_BAD_STATE; // (every writer stores the same word)
        if (soff) { // the trajectory of the step: the last k with off[k] <= t
            int lo = 0, hi = K - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= t)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            g = (uint64_t)(soff[lo] + (t - off[lo]));
        }
    }

    int pick = 0;
    unsigned long long rem = __ballot(st >= 0);
    while (rem) { // one round per distinct state of the wavefront (uniform)
        const int leader = __ffsll((long long)rem) - 1;
        const int s = __builtin_amdgcn_readfirstlane(__shfl(st, leader));
        const bool mine = st == s;
        if (mine) {
            double mx = -INFINITY, sum = 0.0;
            bool first = true; // (uniform over the lanes of this round)
            for (int c = 0; c < M; ++c) {
                const int q = s * M + c;
                const double lwq = lw[q];
                if (lwq == -INFINITY) // (uniform: a component of weight zero is not visited)
                    continue;
                const double a = lwq + mvn::log_density<DMAX, DIAG>(x, D, mu + (size_t)q * D, W + (size_t)q * fs, cst[q]);
                double e;
                if (a > mx) {
                    sum = fma(sum, exp(mx - a), 1.0);
                    mx = a;
                    e = 1.0;
                } else {
                    e = a == -INFINITY ? 0.0 : exp(a - mx); // (a density that underflowed to nothing is never picked)
                    sum += e;
                }
                if (first) {
                    pick = c;
                    first = false;
                } else if (draw_uniform01(key, g * (uint64_t)M + (uint64_t)c) * sum < e) {
                    pick = c;
                }
            }
        }
        rem &= ~__ballot(mine);
    }
    if (active)
        labels[t] = st >= 0 ? st * M + pick : -1;
}

} // namespace gmm
} // namespace bhmm
