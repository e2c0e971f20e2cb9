// score_kernels.hpp -- forward-only log-likelihood of several models on the loaded observations
// (bhmm_score, score_api.hip).  Nothing of the E-step's state is read or written: the kernels take
// the context's chunk plan and observation layouts and write to buffers of their own.
//
//   k_score_fwd    (N <= 8, gaussian / discrete) one lane per chunk, the whole N-vector in
//                  registers; grid (chunk groups of 64, models), so a workgroup is one CI record
//                  group of ONE model and the model is uniform (scalar loads).  Per chunk:
//                    warm-up  W steps before the chunk from the uniform vector on the
//                             trajectory-major observations -- or from pi at the start of the
//                             trajectory when that is closer (then exact); none for a first chunk
//                    sweep    alpha_t = (alpha_{t-1} A) o p_t, rescaled every step by the power of
//                             two that puts its largest entry in [0.5, 1) (exact)
//                  and writes per (model, chunk) only its log-normaliser
//                    removed exponents * ln 2 + log sum(alpha_end) - log sum(alpha_entry)
//                  (first chunk: no entry term, the reference does not normalise pi), the entry
//                  vector it assumed and the exit vector it computed.  No alpha rows, no statistics.
//   k_score_check  each assumed entry against its predecessor's exit: componentwise relative after
//                  normalisation (the rule of k_spec_check), one failure counter per model.
//   k_score_logl   per (trajectory, model) the fixed-order chunk sum of k_logl.
//   k_score_serial the exact path: one workgroup per (trajectory, model), the serial recursion over
//                  the whole trajectory with the states spread over the threads.  Any N and explicit
//                  pobs; for N <= 8 the fallback after two failed boundary checks.
//
// A probability that is exactly zero gives alpha = 0 from that step on and log 0 = -inf; the
// support of a warm-up vector from the uniform vector contains the support of the true one, so a
// chunk that reaches zero from an assumed entry reaches zero from the true one as well, and its
// boundaries need no check.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "estep_sweep.hpp" // gauss_pdf (and estep_kernels.hpp: Model, Chunks, ci_rec, logl_one)

namespace bhmm {

constexpr int SCORE_MAX_MODELS = 64; // models per launch (the host splits longer lists)
constexpr int SCORE_PF = 8;          // observations loaded this many steps ahead of their use

template <int KIND>
using score_obs_t = typename std::conditional<KIND == EMIT_DISC, int32_t, double>::type;

// emission row of one observation; *pexp: exponent folded into the row (exact power of two)
// row stride (doubles) of B^T staged in LDS: a row of 8 doubles at a 64-byte stride starts at one of only 4
// bank offsets, so random symbols collide; 2 doubles of padding spread the rows over 16 (aligned for 16-byte reads)
__host__ __device__ constexpr int score_bt_stride(int N) { return N % 2 == 0 ? N + 2 : N + 1; }

template <int N, int KIND, int BS = N>
__device__ __forceinline__ void score_emit(const Model<N> &m, const double *Bt, score_obs_t<KIND> o,
                                           double (&p)[N], int &pexp)
{
    pexp = 0;
    if constexpr (KIND == EMIT_DISC) {
#pragma unroll
        for (int j = 0; j < N; ++j)
            p[j] = Bt[(int64_t)o * BS + j];
        // a column of B in the denormal range: times 2^900, exactly (its product with the vector would round on the
        // denormal grid)
        double mx = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j)
            mx = fmax(mx, p[j]);
        if (__builtin_expect(mx < 0x1p-959 && mx > 0.0, 0)) {
#pragma unroll
            for (int j = 0; j < N; ++j)
                p[j] = ldexp(p[j], 900);
            pexp = -900;
        }
    } else {
        double mx = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            p[j] = gauss_pdf<true>(o - m.e0[j], m.e4[j], m.e5[j], m.emg);
            mx = fmax(mx, p[j]);
        }
        if (mx < 0x1p-959) {
            // an all-zero row (outliers, a NaN observation) is a row of ones (outputmodel.py:126-130);
            // a row in the denormal range is scaled up by 2^900 and the exponent counted
            const bool zero = mx == 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j)
                p[j] = zero ? 1.0 : ldexp(p[j], 900);
            pexp = zero ? 0 : -900;
        }
    }
}

// steps 0 .. n-1 (n >= 1) of one lane: load(i) gives the observation of step i, step(o, i) consumes
// it; loads run SCORE_PF steps ahead, every index they use is inside [0, n)
template <class Load, class Step>
__device__ __forceinline__ void score_steps(int64_t n, Load load, Step step)
{
    using T = decltype(load(int64_t(0)));
    T cur[SCORE_PF], nxt[SCORE_PF];
#pragma unroll
    for (int u = 0; u < SCORE_PF; ++u)
        cur[u] = load(min((int64_t)u, n - 1));
    for (int64_t i0 = 0; i0 < n; i0 += SCORE_PF) {
#pragma unroll
        for (int u = 0; u < SCORE_PF; ++u)
            nxt[u] = load(min(i0 + SCORE_PF + u, n - 1));
#pragma unroll
        for (int u = 0; u < SCORE_PF; ++u)
            if (i0 + u < n)
                step(cur[u], i0 + u);
#pragma unroll
        for (int u = 0; u < SCORE_PF; ++u)
            cur[u] = nxt[u];
    }
}

// models: [S] (blockIdx.y); Ws: [S] warm-up lengths; Bt_all: [S][M][N] (discrete); outputs [S][Gp] /
// [S][Gp][N].  BT_LDS: the model's B^T is staged in LDS (M * N doubles of dynamic LDS).
template <int N, int KIND, bool BT_LDS>
__global__ __launch_bounds__(64) void k_score_fwd(const Model<N> *__restrict__ models, const int32_t *__restrict__ Ws,
                                                  const Chunks ch, int G, int Gp, const void *obs_ci,
                                                  const void *obs_rm, const double *Bt_all, int M, double *logLc,
                                                  double *a_entry, double *a_exit)
{
    using T = score_obs_t<KIND>;
    extern __shared__ double sBt[];
    const int s = blockIdx.y;
    const Model<N> &m = models[s];
    const double *Bt = nullptr;
    if constexpr (KIND == EMIT_DISC) {
        Bt = Bt_all + (size_t)s * M * N;
        if constexpr (BT_LDS) {
            for (int e = threadIdx.x; e < M * N; e += blockDim.x)
                sBt[(e / N) * score_bt_stride(N) + e % N] = Bt[e];
            __syncthreads();
            Bt = sBt;
        }
    }
    constexpr int BS = BT_LDS ? score_bt_stride(N) : N; // row stride of B^T
    const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= G)
        return;
    const int len = ch.len[g];
    if (len <= 0)
        return;
    const int64_t t0 = ch.t0[g];
    const int64_t tstart = ch.goff[g] - t0; // first step of the trajectory in the concatenated arrays
    const T *rm = static_cast<const T *>(obs_rm);
    const T *ci = static_cast<const T *>(obs_ci);

    double a[N];
    double esum = 0.0;
    bool init = false; // the next step starts the trajectory: alpha_0 = pi o p_0
    auto step = [&](T o, int64_t) {
        double p[N];
        int pe;
        score_emit<N, KIND, BS>(m, Bt, o, p, pe);
        double v[N];
        if (init) {
#pragma unroll
            for (int j = 0; j < N; ++j)
                v[j] = m.pi[j] * p[j];
            init = false;
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int i = 0; i < N; ++i)
                    acc = fma(a[i], m.A[i * N + j], acc);
                v[j] = acc * p[j];
            }
        }
        double mx = v[0];
#pragma unroll
        for (int j = 1; j < N; ++j)
            mx = fmax(mx, v[j]);
        const int e = exponent_of(mx); // (0 for an all-zero vector, which stays zero)
#pragma unroll
        for (int j = 0; j < N; ++j)
            a[j] = ldexp(v[j], -e);
        esum += (double)(e + pe);
    };

    // ---- entry vector ----
    double ent[N];
    if (t0 == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j)
            ent[j] = m.pi[j];
        init = true;
    } else {
        const int W = Ws[s];
        const int64_t w0 = t0 > W ? t0 - W : 0;
#pragma unroll
        for (int j = 0; j < N; ++j)
            a[j] = 1.0 / N;
        init = w0 == 0;
        score_steps(t0 - w0, [&](int64_t i) { return rm[tstart + w0 + i]; }, step);
#pragma unroll
        for (int j = 0; j < N; ++j)
            ent[j] = a[j];
    }

    // ---- sweep over the chunk (CI observations: one record per step and group of 64 chunks) ----
    esum = 0.0;
    const int lane = (int)(g & 63);
    score_steps((int64_t)len, [&](int64_t i) { return ci[ci_rec(g, (int)i, ch.Lmax) * 64 + lane]; }, step);

    double se = 0.0, sx = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        se += ent[j];
        sx += a[j];
    }
    double lc;
    if (!(se > 0.0) || !(sx > 0.0))
        lc = -INFINITY;
    else
        lc = esum * 0.6931471805599453 + log(sx) - (t0 == 0 ? 0.0 : log(se));
    const int64_t r = (int64_t)s * Gp + g;
    logLc[r] = lc;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        a_entry[r * N + j] = ent[j];
        a_exit[r * N + j] = a[j];
    }
}

// The same pass with P1's lane layout: H = N/2 lanes per chunk (N padded to 2, 4, 8), lane q owns the
// state pair (2q, 2q+1), 64 chunks per workgroup of 32 N threads.  A lane computes the emissions of its
// own two states only (a gaussian density per state instead of N; a discrete lane reads 16 bytes of the row)
// and holds the two columns of A it needs; the vector is all-gathered by DPP quad permutes in the
// lane-relative slot order of grp_gather (slot i = state i ^ 2q).  Rescaling: the group's largest exponent.
// Outputs as k_score_fwd (vectors of N padded entries, padding zero).
template <int N, int KIND, bool BT_LDS>
__global__ __launch_bounds__(32 * N) void k_score_pair(const Model<N> *__restrict__ models,
                                                       const int32_t *__restrict__ Ws, const Chunks ch, int G, int Gp,
                                                       const void *obs_ci, const void *obs_rm, const double *Bt_all,
                                                       int M, double *logLc, double *a_entry, double *a_exit)
{
    using T = score_obs_t<KIND>;
    constexpr int H = N / 2;
    constexpr int ZERO_EXP = -(1 << 20);
    extern __shared__ double sBt[];
    const int s = blockIdx.y;
    const Model<N> &m = models[s];
    const double *Bt = nullptr;
    if constexpr (KIND == EMIT_DISC) {
        Bt = Bt_all + (size_t)s * M * N;
        if constexpr (BT_LDS) {
            for (int e = threadIdx.x; e < M * N; e += blockDim.x)
                sBt[(e / N) * score_bt_stride(N) + e % N] = Bt[e];
            __syncthreads();
            Bt = sBt;
        }
    }
    constexpr int BS = BT_LDS ? score_bt_stride(N) : N;
    const int cl = threadIdx.x / H, q = threadIdx.x % H;
    const int64_t g = (int64_t)blockIdx.x * 64 + cl;
    if (g >= G) // (every lane of a chunk leaves together: the group exchanges below stay within live lanes)
        return;
    const int len = ch.len[g];
    if (len <= 0)
        return;
    const int64_t t0 = ch.t0[g];
    const int64_t tstart = ch.goff[g] - t0;
    const T *rm = static_cast<const T *>(obs_rm);
    const T *ci = static_cast<const T *>(obs_ci);
    const int nreal = m.nreal;

    double Ac[N][2]; // Ac[i][b] = A[state of slot i][2q + b]
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int b = 0; b < 2; ++b)
            Ac[i][b] = m.A[slot_state(i, q) * N + 2 * q + b];
    const double pi0 = m.pi[2 * q], pi1 = m.pi[2 * q + 1];
    double mu[2] = {0.0, 0.0}, ea[2] = {0.0, 0.0}, eb[2] = {1.0, 1.0};
    if constexpr (KIND == EMIT_GAUSS)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            mu[b] = m.e0[2 * q + b];
            ea[b] = m.e4[2 * q + b];
            eb[b] = m.e5[2 * q + b];
        }
    const bool real0 = 2 * q < nreal, real1 = 2 * q + 1 < nreal;

    double a[2];
    double esum = 0.0;
    bool init = false;
    auto step = [&](T o, int64_t) {
        double p[2];
        int pe = 0;
        if constexpr (KIND == EMIT_DISC) {
            const double2 r = *reinterpret_cast<const double2 *>(Bt + (int64_t)o * BS + 2 * q);
            p[0] = r.x;
            p[1] = r.y;
            double mx = fmax(p[0], p[1]); // (padded states: zero)
            if constexpr (H >= 2)
                mx = fmax(mx, grp_xor<1>(mx));
            if constexpr (H >= 4)
                mx = fmax(mx, grp_xor<2>(mx));
            if (__builtin_expect(mx < 0x1p-959 && mx > 0.0, 0)) { // (group-uniform) as score_emit
                p[0] = ldexp(p[0], 900);
                p[1] = ldexp(p[1], 900);
                pe = -900;
            }
        } else {
            p[0] = real0 ? gauss_pdf<true>(o - mu[0], ea[0], eb[0], m.emg) : 0.0;
            p[1] = real1 ? gauss_pdf<true>(o - mu[1], ea[1], eb[1], m.emg) : 0.0;
            double mx = fmax(p[0], p[1]);
            if constexpr (H >= 2)
                mx = fmax(mx, grp_xor<1>(mx));
            if constexpr (H >= 4)
                mx = fmax(mx, grp_xor<2>(mx));
            if (mx < 0x1p-959) { // (group-uniform) the outlier rule / a row in the denormal range, as score_emit
                const bool zero = mx == 0.0;
                p[0] = zero ? (real0 ? 1.0 : 0.0) : ldexp(p[0], 900);
                p[1] = zero ? (real1 ? 1.0 : 0.0) : ldexp(p[1], 900);
                pe = zero ? 0 : -900;
            }
        }
        double v[2];
        if (init) {
            v[0] = pi0 * p[0];
            v[1] = pi1 * p[1];
            init = false;
        } else {
            double full[N];
            grp_gather<N>(a, full);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                double acc = 0.0;
#pragma unroll
                for (int i = 0; i < N; ++i)
                    acc = fma(full[i], Ac[i][b], acc);
                v[b] = acc * p[b];
            }
        }
        const double mx = fmax(v[0], v[1]);
        int e = grp_max_i32<H>(mx > 0.0 ? exponent_of(mx) : ZERO_EXP);
        e = e == ZERO_EXP ? 0 : e; // (an all-zero vector stays zero)
        a[0] = ldexp(v[0], -e);
        a[1] = ldexp(v[1], -e);
        esum += (double)(e + pe);
    };

    double ent[2];
    if (t0 == 0) {
        ent[0] = pi0;
        ent[1] = pi1;
        init = true;
    } else {
        const int W = Ws[s];
        const int64_t w0 = t0 > W ? t0 - W : 0;
        a[0] = real0 ? 1.0 / nreal : 0.0;
        a[1] = real1 ? 1.0 / nreal : 0.0;
        init = w0 == 0;
        score_steps(t0 - w0, [&](int64_t i) { return rm[tstart + w0 + i]; }, step);
        ent[0] = a[0];
        ent[1] = a[1];
    }
    esum = 0.0;
    const int lane = (int)(g & 63);
    score_steps((int64_t)len, [&](int64_t i) { return ci[ci_rec(g, (int)i, ch.Lmax) * 64 + lane]; }, step);

    const double se = grp_sum<H>(ent[0] + ent[1]), sx = grp_sum<H>(a[0] + a[1]);
    double lc;
    if (!(se > 0.0) || !(sx > 0.0))
        lc = -INFINITY;
    else
        lc = esum * 0.6931471805599453 + log(sx) - (t0 == 0 ? 0.0 : log(se));
    const int64_t r = (int64_t)s * Gp + g;
    if (q == 0)
        logLc[r] = lc;
    *reinterpret_cast<double2 *>(a_entry + r * N + 2 * q) = make_double2(ent[0], ent[1]);
    *reinterpret_cast<double2 *>(a_exit + r * N + 2 * q) = make_double2(a[0], a[1]);
}

// boundary check: fails[s] counts the boundaries of model s out of tolerance
template <int N>
__global__ __launch_bounds__(256) void k_score_check(const Chunks ch, int G, int Gp, const double *logLc,
                                                     const double *a_entry, const double *a_exit, double tol,
                                                     unsigned int *fails)
{
    const int s = blockIdx.y;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G || ch.len[g] <= 0 || ch.t0[g] == 0)
        return;
    const int64_t r = (int64_t)s * Gp + g;
    if (logLc[r] == -INFINITY || logLc[r - 1] == -INFINITY)
        return; // (the trajectory's probability is zero: -inf whatever the boundary)
    const double *x = a_entry + r * N, *y = a_exit + (r - 1) * N;
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        sx += x[j];
        sy += y[j];
    }
    double dev = 0.0;
    if (!(sx > 0.0) || !(sy > 0.0)) {
        dev = 1.0;
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double xs = x[j] / sx, ys = y[j] / sy;
            const double d = fabs(xs - ys);
            const double rel = (ys > 1e-280) ? d / ys : (d > 1e-280 ? 1.0 : 0.0);
            dev = fmax(dev, rel);
        }
    }
    if (!(dev <= tol))
        atomicAdd(&fails[s], 1u);
}

// per (trajectory, model): the fixed-order sum of its chunks (k_logl)
[[maybe_unused]] static __global__ __launch_bounds__(64) void k_score_logl(const int32_t *traj_c0, int K, int Gp,
                                                                          const double *logLc, double *logLk)
{
    logl_one(blockIdx.x, traj_c0, logLc + (size_t)blockIdx.y * Gp, logLk + (size_t)blockIdx.y * K);
}

// ---- exact path ----------------------------------------------------------------------------
constexpr int SCORE_SERIAL_R = 4; // states per thread (n <= 4 * 1024)

__device__ __forceinline__ double score_block_reduce(double v, bool is_max, double *red)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        const double o = __shfl_xor(v, h, 64);
        v = is_max ? fmax(v, o) : v + o;
    }
    const int nw = (blockDim.x + 63) / 64;
    __syncthreads(); // (red is reused by consecutive reductions)
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x / 64] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < nw; ++w)
        r = is_max ? fmax(r, red[w]) : r + red[w];
    return r;
}

// grid (K, S), blockDim a multiple of 64 with n <= SCORE_SERIAL_R * blockDim; LDS: n + 16 doubles.
// Model s: A_all + s n^2, pi_all + s n, par0_all + s n (gaussian mu) / s n M (discrete B), par1_all + s n.
// Explicit pobs: obs_rm holds n doubles per step.
template <int KIND>
__global__ __launch_bounds__(1024) void k_score_serial(int n, int M, int K, const int64_t *offsets, const void *obs_rm,
                                                       const double *A_all, const double *pi_all,
                                                       const double *par0_all, const double *par1_all, double *logLk)
{
    extern __shared__ double sh[];
    double *alpha = sh, *red = sh + n;
    const int s = blockIdx.y, k = blockIdx.x;
    const double *A = A_all + (size_t)s * n * n;
    const double *pi = pi_all + (size_t)s * n;
    const double *par0 = par0_all ? par0_all + (size_t)s * n * (KIND == EMIT_DISC ? M : 1) : nullptr;
    const double *par1 = par1_all ? par1_all + (size_t)s * n : nullptr;
    const int64_t base = offsets[k], T = offsets[k + 1] - base;
    const int bd = blockDim.x, tid = threadIdx.x;
    double esum = 0.0;
    bool zero = false;
    for (int64_t t = 0; t < T && !zero; ++t) {
        double p[SCORE_SERIAL_R], v[SCORE_SERIAL_R];
        double pmx = 0.0;
#pragma unroll
        for (int r = 0; r < SCORE_SERIAL_R; ++r) {
            const int j = tid + r * bd;
            p[r] = 0.0;
            if (j < n) {
                if constexpr (KIND == EMIT_GAUSS) {
                    const double z = (static_cast<const double *>(obs_rm)[base + t] - par0[j]) / par1[j];
                    p[r] = 1.0 / (sqrt(2.0 * M_PI) * par1[j]) * exp(-0.5 * z * z);
                    if (!(p[r] > 0.0))
                        p[r] = 0.0; // (a NaN observation is an outlier)
                } else if constexpr (KIND == EMIT_DISC) {
                    p[r] = par0[(size_t)j * M + static_cast<const int32_t *>(obs_rm)[base + t]];
                } else {
                    p[r] = static_cast<const double *>(obs_rm)[(base + t) * n + j];
                }
            }
            pmx = fmax(pmx, p[r]);
        }
        // a row in the denormal range, of any kind (entries of B, explicit pobs): times 2^900, exactly -- the
        // product with alpha would round on the denormal grid.  An all-zero gaussian row is a row of ones
        int pe = 0;
        pmx = score_block_reduce(pmx, true, red);
        if (pmx < 0x1p-959 && (KIND == EMIT_GAUSS || pmx > 0.0)) {
#pragma unroll
            for (int r = 0; r < SCORE_SERIAL_R; ++r)
                p[r] = tid + r * bd < n ? (pmx == 0.0 ? 1.0 : ldexp(p[r], 900)) : 0.0;
            pe = pmx == 0.0 ? 0 : -900;
        }
        double mx = 0.0;
#pragma unroll
        for (int r = 0; r < SCORE_SERIAL_R; ++r) {
            const int j = tid + r * bd;
            v[r] = 0.0;
            if (j < n) {
                if (t == 0) {
                    v[r] = pi[j] * p[r];
                } else {
                    double acc = 0.0;
                    for (int i = 0; i < n; ++i)
                        acc = fma(alpha[i], A[(size_t)i * n + j], acc);
                    v[r] = acc * p[r];
                }
            }
            mx = fmax(mx, v[r]);
        }
        mx = score_block_reduce(mx, true, red); // (its barriers also end every read of alpha)
        if (mx == 0.0) {
            zero = true;
            break;
        }
        const int e = exponent_of(mx);
        esum += (double)(e + pe);
#pragma unroll
        for (int r = 0; r < SCORE_SERIAL_R; ++r)
            if (tid + r * bd < n)
                alpha[tid + r * bd] = ldexp(v[r], -e);
        __syncthreads();
    }
    double part = 0.0;
    if (!zero && T > 0)
        for (int j = tid; j < n; j += bd)
            part += alpha[j];
    const double sum = score_block_reduce(part, false, red);
    if (tid == 0)
        logLk[(size_t)s * K + k] = T == 0 ? 0.0 : (zero ? -INFINITY : esum * 0.6931471805599453 + log(sum));
}

} // namespace bhmm
