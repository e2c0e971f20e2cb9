// mvn_kernels.hpp -- multivariate gaussian emissions: the two passes over D-dimensional observations around the
// recursions, which run on explicit emission rows (mvn_api.hip).
//
//   k_mvn_rows            l_ti = -|W_i (x_t - mu_i)|^2 / 2 + c_i for every step t and state i, W_i = L_i^-1 the inverse
//                         Cholesky factor of Sigma_i (lower triangular, packed row-major; diagonal covariances: D
//                         reciprocals), c_i = -sum_d log L_i[d,d] - D log(2 pi) / 2 -- both from the host
//                         (host::mvn_prepare).  The mean is subtracted FIRST and the difference whitened: W x - W mu
//                         loses |mu| / sigma in relative accuracy.  Writes m_t = max_i l_ti, the row exp(l_ti - m_t)
//                         (the largest entry of a finite row is exp(0) = 1.0 exactly) and, when asked, l_ti.
//   k_mvn_shift           shift_k = sum_t m_t per trajectory: one workgroup each, strided partial sums per thread in
//                         ascending order, then a fixed tree.  No atomics.
//   k_mvn_moments         S0_i = sum_t g_ti, S1_i = sum_t g_ti (x_t - mu_i), S2_i = sum_t g_ti (x_t - mu_i)(x_t - mu_i)^T
//                         (lower triangle or diagonal) about the given means: one partial per workgroup and output.
//   k_mvn_moments_finish  adds the partials of an output in ascending workgroup order.  No atomics: bitwise
//                         reproducible.
//
// k_mvn_rows: one lane per step, ROWS_THREADS steps per workgroup.  A lane keeps x_t and d = x_t - mu_i in registers
// (DMAX of each: the kernel is instantiated per dimension class and its loops over the dimensions are fully unrolled;
// x_t arrives through LDS, so the tile is read from memory once and in whole cache lines); the
// per-state tables are read at addresses that are uniform over the wavefront, so they arrive as scalar loads and the
// FMA takes its table operand from a scalar register -- no per-lane gather, no LDS.  The l of ROWS_NB states at a
// time go through LDS so that rows (and l) are written in whole cache lines by the workgroup, not one state per lane
// and instruction.  With more than ROWS_NB states the raw l of a block of states is parked in the row itself and the
// workgroup rescales its own rows once every block is done and m_t is known.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace bhmm {
namespace mvn {

constexpr int ROWS_THREADS = 256; // steps per workgroup of k_mvn_rows
constexpr int ROWS_NB = 16;       // states whose l pass through LDS at a time (ROWS_NB * ROWS_THREADS doubles)
constexpr int X_PIECE = 3968;     // doubles of a tile's observations staged at a time: X_PIECE * 33 / 32 <= ROWS_NB * ROWS_THREADS
static_assert(X_PIECE + X_PIECE / 32 <= ROWS_NB * ROWS_THREADS, "the skewed piece must fit s_l");
constexpr int SHIFT_THREADS = 256;
constexpr int MOM_THREADS = 256;  // outputs per workgroup of k_mvn_moments
constexpr int MOM_TILE = 128;     // steps it stages in LDS at a time
constexpr int MOM_MAX_GROUPS = 2048; // partials per output at most

// doubles of one state's whitening table
__host__ __device__ inline size_t factor_size(int D, bool diag) { return diag ? (size_t)D : (size_t)D * (D + 1) / 2; }
// doubles of one state's packed moments: S0 | S1 [D] | S2
__host__ __device__ inline size_t moment_stride(int D, bool diag) { return 1 + (size_t)D + factor_size(D, diag); }

// NaN stays; a NaN l makes m NaN
__device__ inline double nan_max(double m, double l) { return m != m ? m : ((l > m || l != l) ? l : m); }

// tab: [mu n*D | W n*factor_size | c n].  rows [total][n] and m [total], or both nullptr (only l is wanted); logp
// [total][n] or nullptr.
template <int DMAX, bool DIAG>
__global__ __launch_bounds__(ROWS_THREADS) void k_mvn_rows(const double *__restrict__ X, int64_t total, int D, int n,
                                                           const double *__restrict__ tab, double *rows,
                                                           double *__restrict__ m_out, double *__restrict__ logp)
{
    __shared__ double s_l[ROWS_NB * ROWS_THREADS];
    __shared__ double s_m[ROWS_THREADS];
    const size_t fs = factor_size(D, DIAG);
    const double *mu = tab, *W = tab + (size_t)n * D, *cst = W + (size_t)n * fs;
    const int64_t t0 = (int64_t)blockIdx.x * ROWS_THREADS;
    const int64_t t = t0 + threadIdx.x;
    const int steps = (int)(total - t0 < ROWS_THREADS ? total - t0 : ROWS_THREADS);
    const bool active = t < total;
    const bool park = rows && n > ROWS_NB; // the raw l waits in the row until m_t is known
    double m = -INFINITY;

    // the lane's observation, in registers for every state.  The tile's rows are contiguous in X: they come through
    // LDS (s_l, free until the first state) in coalesced pieces, skewed by one double per 32 so that the lanes' reads
    // at a stride of D doubles spread over the banks
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

    for (int i0 = 0; i0 < n; i0 += ROWS_NB) {
        const int nb = n - i0 < ROWS_NB ? n - i0 : ROWS_NB;
        for (int j = 0; j < nb; ++j) {
            const int i = i0 + j;
            const double *mui = mu + (size_t)i * D;
            const double *Wi = W + (size_t)i * fs;
            double d[DMAX];
#pragma unroll
            for (int a = 0; a < DMAX; ++a)
                d[a] = a < D ? x[a] - mui[a] : 0.0;
            double q = 0.0;
#pragma unroll
            for (int a = 0; a < DMAX; ++a) {
                if (a < D) { // (uniform)
                    double z;
                    if constexpr (DIAG) {
                        z = Wi[a] * d[a];
                    } else {
                        const double *Wa = Wi + a * (a + 1) / 2;
                        z = 0.0;
#pragma unroll
                        for (int b = 0; b <= a; ++b)
                            z = fma(Wa[b], d[b], z);
                    }
                    q = fma(z, z, q);
                }
            }
            const double l = fma(-0.5, q, cst[i]);
            s_l[j * ROWS_THREADS + threadIdx.x] = l;
            m = nan_max(m, l);
        }
        if (!park)
            s_m[threadIdx.x] = m;
        __syncthreads();
        // the block's [steps][nb] values, nb contiguous doubles per step
        for (int e = threadIdx.x; e < steps * nb; e += ROWS_THREADS) {
            const int s = e / nb, j = e - s * nb;
            const size_t at = (size_t)(t0 + s) * n + i0 + j;
            const double l = s_l[j * ROWS_THREADS + s];
            if (logp)
                logp[at] = l;
            if (rows)
                rows[at] = park ? l : exp(l - s_m[s]);
        }
        __syncthreads(); // (s_l is written again)
    }
    if (park) { // the workgroup's own rows again: l -> exp(l - m_t)
        s_m[threadIdx.x] = m;
        __syncthreads(); // (also orders the rows written above before the reads below, within the workgroup)
        double *r = rows + (size_t)t0 * n;
        for (size_t e = threadIdx.x; e < (size_t)steps * n; e += ROWS_THREADS)
            r[e] = exp(r[e] - s_m[e / n]);
    }
    if (active && m_out)
        m_out[t] = m;
}

// shift[k] = sum of m over the steps of trajectory k (0.0 for an empty one)
__global__ __launch_bounds__(SHIFT_THREADS) void k_mvn_shift(const double *__restrict__ m,
                                                             const int64_t *__restrict__ off, int K,
                                                             double *__restrict__ shift)
{
    __shared__ double s[SHIFT_THREADS];
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int64_t a = off[k], b = off[k + 1];
        double acc = 0.0;
        for (int64_t t = a + threadIdx.x; t < b; t += SHIFT_THREADS)
            acc += m[t];
        s[threadIdx.x] = acc;
        __syncthreads();
        for (int w = SHIFT_THREADS / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w)
                s[threadIdx.x] += s[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0)
            shift[k] = s[0];
        __syncthreads();
    }
}

// (a, b) of the q-th entry of a lower triangle stored row-major
__device__ inline void tri_index(int q, int &a, int &b)
{
    a = 0;
    while ((a + 1) * (a + 2) / 2 <= q)
        ++a;
    b = q - a * (a + 1) / 2;
}

// Output e = i * moment_stride + p of the packed moments; workgroup (g, y) owns the outputs y * epb .. and the steps
// [g * span, (g + 1) * span); slices = MOM_THREADS / epb >= 1 threads share an output (step s of a tile goes to slice
// s % slices) and are added in ascending slice order at the end.  part: [gridDim.x][E].
// LDS: x tile [MOM_TILE][D] | gamma tile [MOM_TILE][nsi] (the states i_lo .. i_lo + nsi - 1 its outputs belong to) |
// MOM_THREADS doubles for the slices.
template <bool DIAG>
__global__ __launch_bounds__(MOM_THREADS) void k_mvn_moments(const double *__restrict__ X,
                                                             const double *__restrict__ gam, int64_t total, int D,
                                                             int n, const double *__restrict__ mu, int64_t span,
                                                             int epb, int nsi_max, double *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *s_x = reinterpret_cast<double *>(smem);
    double *s_g = s_x + (size_t)MOM_TILE * D;
    double *s_red = s_g + (size_t)MOM_TILE * nsi_max;
    const int ms = (int)moment_stride(D, DIAG);
    const int64_t E = (int64_t)n * ms;
    const int slices = MOM_THREADS / epb;
    const int le = threadIdx.x % epb, slice = threadIdx.x / epb;
    const int64_t e_lo = (int64_t)blockIdx.y * epb;
    const int64_t e_hi = e_lo + epb < E ? e_lo + epb : E; // (exclusive)
    const int64_t e = e_lo + le;
    const bool owner = e < e_hi && slice < slices;
    const int i_lo = (int)(e_lo / ms);
    const int nsi = (int)((e_hi - 1) / ms) - i_lo + 1; // <= nsi_max (host: the same arithmetic)
    // what this thread's output multiplies: gamma of state i, (x_a - mu_a) when wa, (x_b - mu_b) when wb
    int i = i_lo, a = 0, b = 0;
    bool wa = false, wb = false;
    double mua = 0.0, mub = 0.0;
    if (owner) {
        i = (int)(e / ms);
        const int p = (int)(e - (int64_t)i * ms);
        if (p >= 1 && p <= D) {
            a = p - 1;
            wa = true;
        } else if (p > D) {
            if (DIAG)
                a = b = p - 1 - D;
            else
                tri_index(p - 1 - D, a, b);
            wa = wb = true;
        }
        mua = mu[(size_t)i * D + a];
        mub = mu[(size_t)i * D + b];
    }
    const int gi = i - i_lo;
    const int64_t r0 = (int64_t)blockIdx.x * span;
    const int64_t r1 = r0 + span < total ? r0 + span : total;
    double acc = 0.0;
    for (int64_t t0 = r0; t0 < r1; t0 += MOM_TILE) {
        const int steps = (int)(r1 - t0 < MOM_TILE ? r1 - t0 : MOM_TILE);
        __syncthreads(); // (the tile before has been read)
        for (int k = threadIdx.x; k < steps * D; k += MOM_THREADS)
            s_x[k] = X[(size_t)t0 * D + k];
        for (int k = threadIdx.x; k < steps * nsi; k += MOM_THREADS) {
            const int s = k / nsi, j = k - s * nsi;
            s_g[s * nsi_max + j] = gam[(size_t)(t0 + s) * n + i_lo + j];
        }
        __syncthreads();
        if (owner)
            for (int s = slice; s < steps; s += slices) {
                const double g = s_g[s * nsi_max + gi];
                const double da = wa ? s_x[s * D + a] - mua : 1.0;
                const double db = wb ? s_x[s * D + b] - mub : 1.0;
                acc = fma(g * da, db, acc);
            }
    }
    if (slices > 1) {
        __syncthreads();
        s_red[threadIdx.x] = acc;
        __syncthreads();
        if (owner && slice == 0)
            for (int q = 1; q < slices; ++q)
                acc += s_red[q * epb + le];
    }
    if (owner && slice == 0)
        part[(size_t)blockIdx.x * E + e] = acc;
}

__global__ __launch_bounds__(256) void k_mvn_moments_finish(const double *__restrict__ part, int G, int64_t E,
                                                            double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E)
        return;
    double acc = part[e];
    for (int g = 1; g < G; ++g)
        acc += part[(size_t)g * E + e];
    out[e] = acc;
}

} // namespace mvn
} // namespace bhmm
