// mvn_kernels.hpp -- multivariate gaussian emissions: the passes over D-dimensional observations around the
// recursions, which run on explicit emission rows (mvn_api.hip, DESIGN.md sections 23 and 24).
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
//   k_mvn_path_moments    the same moments of a hidden path (one state per step): arithmetic per step independent of
//                         n, described where it stands below.
//
// k_mvn_rows: one lane per step, ROWS_THREADS steps per workgroup.  A lane keeps x_t and d = x_t - mu_i in registers
// (DMAX of each: the kernel is instantiated per dimension class and its loops over the dimensions are fully unrolled;
// x_t arrives through LDS, so the tile is read from memory once and in whole cache lines); the
// per-state tables are read at addresses that are uniform over the wavefront, so they arrive as scalar loads and the
// FMA takes its table operand from a scalar register -- no per-lane gather, no LDS.  The l of ROWS_NB states at a
// time go through LDS so that rows (and l) are written in whole cache lines by the workgroup, not one state per lane
// and instruction.  With more than ROWS_NB states the raw l of a block of states is parked in the row itself and the
// workgroup rescales its own rows once every block is done and m_t is known.
// The shape constants of the rows kernel and the arithmetic of one log-density (mvn::log_density) are in
// mvn_density.hpp, which k_gmm_rows (gmm_kernels.hpp) shares.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "mvn_density.hpp"

namespace bhmm {
namespace mvn {

constexpr int SHIFT_THREADS = 256;
constexpr int MOM_THREADS = 256;  // outputs per workgroup of k_mvn_moments
constexpr int MOM_TILE = 128;     // steps it stages in LDS at a time
constexpr int MOM_MAX_GROUPS = 2048; // partials per output at most

// doubles of one state's packed moments: S0 | S1 [D] | S2
__host__ __device__ inline size_t moment_stride(int D, bool diag) { return 1 + (size_t)D + factor_size(D, diag); }

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
            const double l = log_density<DMAX, DIAG>(x, D, mu + (size_t)i * D, W + (size_t)i * fs, cst[i]);
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

// ---- moments of a hidden path (bhmm_mvn_path_moments) ----
// The same packed moments for a hard assignment: S0_i = #{t : s_t = i}, S1_i = sum_{s_t = i} (x_t - mu_i),
// S2_i = sum_{s_t = i} (x_t - mu_i)(x_t - mu_i)^T.  A step touches one state, so the arithmetic per step is the
// stride of one state whatever n is.
//
// A workgroup owns the steps [g * span, (g + 1) * span) and walks them in tiles of pl.tile <= 256 steps, one step per
// thread while a tile is staged:
//   1. the tile's path entries; one outside [0, n) sets *status and takes no further part (nothing is indexed by it);
//   2. the centred differences x_t - mu_{s_t}, once per step, into LDS rows of pl.Dp doubles;
//   3. a stable counting sort of the tile's steps by state: the rank of a step among the earlier steps of its state
//      comes from wave ballots (one round per distinct state of a wavefront; up to PM_WAVE_COUNTS_MAX_N states every
//      wavefront at once in counts of its own, which are then offset by those of the wavefronts before it, beyond
//      that the wavefronts in turn on one array), the start of every state's run from a scan of the counts --
//      integers only, and a function of the path's values alone, so the order of every sum below is too;
//   4. the runs of the sorted list, one state after the other: a lane owns one item of the state's moments (below)
//      and keeps it in plain registers; pl.S lanes of one wavefront share an item, lane j of them takes the steps
//      j, j + S, ... of the run in ascending order and a fixed butterfly adds the S registers at the end of the run;
//   5. the first of the S lanes adds the run's sum into the workgroup's slab [n][stride] -- in LDS while it fits, else
//      the workgroup's own slab of `part` in global memory (zeroed by the host).  An element of the slab has one
//      owning thread for the whole launch: plain load, add, store, no atomics.
// S0 is the count of the sort, added as it is.  Items -- PM_ELEM_FULL / PM_ELEM_DIAG: one entry of S1 or S2 (two LDS
// reads for one FMA); PM_BLOCK (full covariances, D >= PM_BLOCK_MIN_D): a 4 x 4 block (a, b) of the lower triangle
// of S2 -- two rows of four doubles read for 16 FMAs -- or four entries of S1; at D = 64 that is 136 + 16 items.
// The slabs go to part[g][n * stride]; k_mvn_moments_finish adds them in ascending g.
constexpr int PM_THREADS = 256;
constexpr int PM_MAX_TILE = 256;       // one step per thread while a tile is staged and sorted
constexpr int PM_BLOCK_MIN_D = 13;     // full covariances from here on: 4 x 4 blocks
constexpr size_t PM_DIFF_BYTES = 34 * 1024; // LDS the centred differences of a tile may take
constexpr int PM_WAVE_COUNTS_MAX_N = 256; // up to here every wavefront ranks its steps at once, in counts of its own
constexpr unsigned int PM_BAD_STATE = 1u;
enum { PM_ELEM_FULL = 0, PM_ELEM_DIAG = 1, PM_BLOCK = 2 };

struct PmPlan {   // made by pm_plan (host), read by the kernel
    int tile;     // steps per tile: a multiple of 32, <= PM_MAX_TILE
    int Dp;       // doubles per row of centred differences (PM_BLOCK: D rounded up to 4, the rest zeros; else D | 1)
    int S;        // lanes of a wavefront that share an item: a power of two, 4 * (64 / S) >= items
    int slab_lds; // the slab sits in LDS
    int wc;       // count arrays of the sort: one per wavefront (PM_THREADS / 64) or one for all (1)
    int64_t span; // steps per workgroup: a multiple of tile
    int groups;   // workgroups
    size_t lds;   // bytes of dynamic LDS
};

// items a workgroup's lanes own
__host__ __device__ inline int pm_items(int D, int mode)
{
    if (mode == PM_BLOCK) {
        const int nb = (D + 3) / 4;
        return nb * (nb + 1) / 2 + nb;
    }
    return (int)moment_stride(D, mode == PM_ELEM_DIAG) - 1;
}

// LDS: diffs [tile][Dp] | slab [n * stride] (slab_lds) | state [PM_MAX_TILE] | sorted [PM_MAX_TILE] | counts per
// wavefront [wc][n] | count [n] | start [n + 1] | wavefront totals [4] (ints)
inline PmPlan pm_plan(int64_t total, int D, int n, int mode)
{
    // kernel experiments: BHMM_AMD_PM_TILE caps the tile, BHMM_AMD_PM_SLAB_KB is the largest slab kept in LDS
    static const int tile_env = getenv("BHMM_AMD_PM_TILE") ? atoi(getenv("BHMM_AMD_PM_TILE")) : 0;
    static const int slab_env = getenv("BHMM_AMD_PM_SLAB_KB") ? atoi(getenv("BHMM_AMD_PM_SLAB_KB")) : -1;
    PmPlan pl;
    const size_t E = (size_t)n * moment_stride(D, mode == PM_ELEM_DIAG);
    pl.wc = n <= PM_WAVE_COUNTS_MAX_N ? PM_THREADS / 64 : 1;
    const size_t ints = ((size_t)2 * PM_MAX_TILE + (size_t)(pl.wc > 1 ? pl.wc : 0) * n + 2 * (size_t)n + 1 + 4 + 1) / 2 *
                        2 * sizeof(int);
    const size_t budget = 64 * 1024;
    const size_t slab_max = slab_env >= 0 ? (size_t)slab_env * 1024 : budget / 2;
    pl.Dp = mode == PM_BLOCK ? (D + 3) / 4 * 4 : (D | 1);
    const size_t row = (size_t)pl.Dp * sizeof(double);
    pl.slab_lds = E * sizeof(double) <= slab_max && ints + E * sizeof(double) + 64 * row <= budget;
    const size_t avail = budget - ints - (pl.slab_lds ? E * sizeof(double) : 0);
    // (>= 32: n <= 4096 and D <= 64 leave 30 KiB.)  At most PM_DIFF_BYTES of rows: measured at D = 32, N = 8, a tile of
    // 128 steps -- more workgroups per CU -- takes two thirds of the time of 224; below D = 16 the rows are short and
    // the fixed work per tile decides, so the tile stays at PM_MAX_TILE
    pl.tile = (int)std::min<size_t>(PM_MAX_TILE, std::min<size_t>(avail, PM_DIFF_BYTES) / row / 32 * 32);
    if (tile_env >= 32)
        pl.tile = std::min(pl.tile, tile_env / 32 * 32);
    const int items = pm_items(D, mode);
    pl.S = 64;
    while (pl.S > 1 && 4 * (64 / pl.S) < items)
        pl.S >>= 1;
    const int64_t tiles = (total + pl.tile - 1) / pl.tile;
    int64_t G = std::max<int64_t>(1, std::min<int64_t>(tiles, MOM_MAX_GROUPS));
    if (!pl.slab_lds) // (slabs in global memory: at most 64 MiB of them)
        G = std::max<int64_t>(1, std::min<int64_t>(G, (int64_t)((size_t)(64 << 20) / (E * sizeof(double)))));
    pl.span = ((total + G - 1) / G + pl.tile - 1) / pl.tile * pl.tile;
    pl.groups = (int)((total + pl.span - 1) / pl.span);
    pl.lds = (size_t)pl.tile * row + (pl.slab_lds ? E * sizeof(double) : 0) + ints;
    return pl;
}

template <typename PT, int MODE>
__global__ __launch_bounds__(PM_THREADS) void k_mvn_path_moments(const double *__restrict__ X,
                                                                 const PT *__restrict__ path, int64_t total, int D,
                                                                 int n, const double *__restrict__ mu, PmPlan pl,
                                                                 double *part, unsigned int *status)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool DIAG = MODE == PM_ELEM_DIAG;
    const int ms = (int)moment_stride(D, DIAG);
    const size_t E = (size_t)n * ms;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Dp = pl.Dp, S = pl.S;
    double *s_d = reinterpret_cast<double *>(smem);
    double *s_slab = s_d + (size_t)pl.tile * Dp;
    int *s_st = reinterpret_cast<int *>(s_slab + (pl.slab_lds ? E : 0));
    int *s_sorted = s_st + PM_MAX_TILE;
    int *s_cntw = s_sorted + PM_MAX_TILE;
    int *s_cnt = s_cntw + (pl.wc > 1 ? (size_t)pl.wc * n : 0);
    int *s_off = s_cnt + n;
    int *s_wtot = s_off + n + 1;
    double *g_slab = part + (size_t)blockIdx.x * E;

    // zeros: the padding columns of the rows (never written again), the slab
    for (int k = tid; k < pl.tile * Dp; k += PM_THREADS)
        s_d[k] = 0.0;
    if (pl.slab_lds)
        for (size_t e = tid; e < E; e += PM_THREADS)
            s_slab[e] = 0.0;

    // the item this lane owns, with the S - 1 lanes next to it
    const int sl = lane & (S - 1), item = wave * (64 / S) + lane / S;
    const bool active = item < pm_items(D, MODE);
    int ia = 0, ib = 0;   // PM_ELEM_*: the entry (a, b) of S2, or a of S1; PM_BLOCK: the block (ia, ib), or four of S1
    bool second = false;  // an item of S2
    if (MODE == PM_BLOCK) {
        const int nb = Dp / 4;
        second = item < nb * (nb + 1) / 2;
        if (second)
            tri_index(item, ia, ib);
        else
            ia = item - nb * (nb + 1) / 2;
    } else if (active) {
        second = item >= D;
        if (!second)
            ia = item;
        else if (DIAG)
            ia = ib = item - D;
        else
            tri_index(item - D, ia, ib);
    }

    const int64_t r0 = (int64_t)blockIdx.x * pl.span;
    const int64_t r1 = r0 + pl.span < total ? r0 + pl.span : total;
    for (int64_t t0 = r0; t0 < r1; t0 += pl.tile) {
        const int steps = (int)(r1 - t0 < pl.tile ? r1 - t0 : pl.tile);
        __syncthreads(); // (the tile before has been read; the zeros above are written)
        // 1. the path of the tile
        int st = -1;
        if (tid < steps) {
            const int64_t v = (int64_t)path[t0 + tid];
            if (v >= 0 && v < n)
                st = (int)v;
            else
                *status = PM_BAD_STATE; // (every writer stores the same word)
        }
        s_st[tid] = st;
        for (int i = tid; i < (pl.wc > 1 ? pl.wc : 1) * n; i += PM_THREADS)
            s_cntw[i] = 0; // (the counts per wavefront, or -- pl.wc == 1: the same address -- the counts)
        __syncthreads();
        // 2. centred differences; four loads in flight per thread
        {
            const int lim = steps * D;
            const double *Xt = X + (size_t)t0 * D;
            for (int e0 = tid; e0 < lim; e0 += 4 * PM_THREADS) {
                double xv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    xv[k] = e0 + k * PM_THREADS < lim ? Xt[e0 + k * PM_THREADS] : 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = e0 + k * PM_THREADS;
                    if (e < lim) {
                        const int s = e / D, a = e - s * D;
                        const int i = s_st[s];
                        if (i >= 0)
                            s_d[s * Dp + a] = xv[k] - mu[(size_t)i * D + a];
                    }
                }
            }
        }
        // 3. rank of every step among the earlier steps of its state, a round per distinct state of a wavefront:
        // every wavefront at once in counts of its own, which then become what the wavefronts before it hold ...
        int pos = 0;
        const int nw = (steps + 63) / 64;
        if (pl.wc > 1) {
            unsigned long long rem = __ballot(st >= 0);
            while (rem) {
                const int leader = __ffsll((long long)rem) - 1;
                const int ls = __shfl(st, leader);
                const unsigned long long m = __ballot(st == ls);
                if (lane == leader)
                    s_cntw[(size_t)wave * n + ls] = __popcll(m);
                if (st == ls)
                    pos = __popcll(m & ((1ull << lane) - 1ull));
                rem &= ~m;
            }
            __syncthreads();
            for (int i = tid; i < n; i += PM_THREADS) {
                int before = 0;
                for (int w = 0; w < pl.wc; ++w) {
                    const int c = s_cntw[(size_t)w * n + i];
                    s_cntw[(size_t)w * n + i] = before;
                    before += c;
                }
                s_cnt[i] = before;
            }
            __syncthreads();
            if (st >= 0)
                pos += s_cntw[(size_t)wave * n + st];
        }
        // ... or (many states) the wavefronts in turn on one array of counts
        for (int w = 0; pl.wc == 1 && w < nw; ++w) {
            if (wave == w) {
                unsigned long long rem = __ballot(st >= 0);
                while (rem) {
                    const int leader = __ffsll((long long)rem) - 1;
                    const int ls = __shfl(st, leader);
                    const unsigned long long m = __ballot(st == ls);
                    int base = 0;
                    if (lane == leader) { // (the one lane that touches the count of ls)
                        base = s_cnt[ls];
                        s_cnt[ls] = base + __popcll(m);
                    }
                    base = __shfl(base, leader);
                    if (st == ls)
                        pos = base + __popcll(m & ((1ull << lane) - 1ull));
                    rem &= ~m;
                }
            }
            __syncthreads();
        }
        // start of every state's run: exclusive scan of the counts, c consecutive states per thread
        {
            const int c = (n + PM_THREADS - 1) / PM_THREADS;
            int sum = 0;
            for (int j = 0; j < c; ++j)
                if (tid * c + j < n)
                    sum += s_cnt[tid * c + j];
            int inc = sum;
            for (int d = 1; d < 64; d <<= 1) {
                const int v = __shfl_up(inc, d);
                if (lane >= d)
                    inc += v;
            }
            if (lane == 63)
                s_wtot[wave] = inc;
            __syncthreads();
            int base = inc - sum;
            for (int w = 0; w < wave; ++w)
                base += s_wtot[w];
            for (int j = 0; j < c; ++j)
                if (tid * c + j < n) {
                    s_off[tid * c + j] = base;
                    base += s_cnt[tid * c + j];
                }
            if (tid == PM_THREADS - 1)
                s_off[n] = base; // (steps of the tile with a state)
        }
        __syncthreads();
        if (st >= 0)
            s_sorted[s_off[st] + pos] = tid;
        // S0: the counts themselves (thread i % PM_THREADS owns the element of state i)
        for (int i = tid; i < n; i += PM_THREADS)
            if (s_cnt[i]) {
                if (pl.slab_lds)
                    s_slab[(size_t)i * ms] += (double)s_cnt[i];
                else
                    g_slab[(size_t)i * ms] += (double)s_cnt[i];
            }
        __syncthreads();
        // 4. the runs
        const int nv = s_off[n];
        for (int q0 = 0; q0 < nv;) {
            const int i = s_st[s_sorted[q0]];
            const int q1 = s_off[i + 1];
            if constexpr (MODE == PM_BLOCK) {
                double acc[16];
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    acc[k] = 0.0;
                if (active)
                    for (int q = q0 + sl; q < q1; q += S) {
                        const double *row = s_d + (size_t)s_sorted[q] * Dp;
                        const double4 da = *reinterpret_cast<const double4 *>(row + 4 * ia);
                        if (second) {
                            const double4 db = *reinterpret_cast<const double4 *>(row + 4 * ib);
                            const double va[4] = {da.x, da.y, da.z, da.w}, vb[4] = {db.x, db.y, db.z, db.w};
#pragma unroll
                            for (int r = 0; r < 4; ++r)
#pragma unroll
                                for (int cc = 0; cc < 4; ++cc)
                                    acc[4 * r + cc] = fma(va[r], vb[cc], acc[4 * r + cc]);
                        } else {
                            acc[0] += da.x;
                            acc[1] += da.y;
                            acc[2] += da.z;
                            acc[3] += da.w;
                        }
                    }
                for (int d = S >> 1; d >= 1; d >>= 1) // (every lane: a butterfly over the S lanes of an item)
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        acc[k] += __shfl_xor(acc[k], d);
                if (active && sl == 0) {
                    double *dst = (pl.slab_lds ? s_slab : g_slab) + (size_t)i * ms;
                    if (second) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int cc = 0; cc < 4; ++cc) {
                                const int a = 4 * ia + r, b = 4 * ib + cc;
                                if (a < D && b <= a)
                                    dst[1 + D + a * (a + 1) / 2 + b] += acc[4 * r + cc];
                            }
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (4 * ia + r < D)
                                dst[1 + 4 * ia + r] += acc[r];
                    }
                }
            } else {
                double acc = 0.0;
                if (active)
                    for (int q = q0 + sl; q < q1; q += S) {
                        const double *row = s_d + (size_t)s_sorted[q] * Dp;
                        const double da = row[ia];
                        acc = second ? fma(da, row[ib], acc) : acc + da;
                    }
                for (int d = S >> 1; d >= 1; d >>= 1)
                    acc += __shfl_xor(acc, d);
                if (active && sl == 0) {
                    double *dst = (pl.slab_lds ? s_slab : g_slab) + (size_t)i * ms + 1 + item;
                    *dst += acc;
                }
            }
            q0 = q1;
        }
    }
    if (pl.slab_lds) {
        __syncthreads();
        for (size_t e = tid; e < E; e += PM_THREADS)
            g_slab[e] = s_slab[e];
    }
}

} // namespace mvn
} // namespace bhmm
