// filter_kernels.hpp -- filtered state probabilities and one-step predictive log-densities of every step
// (bhmm_filter, filter_api.hip): rows[(offset_k + t) * Q' + q] and logc[offset_k + t], double or float.
// Without a projection Q' = n and the row is alpha^_t(.) = P(s_t = . | o_0 .. o_t); with V ([n][Q] row-major,
// Q <= 8) Q' = Q and the row is sum_i alpha^_t(i) V[i][q], accumulated over i in ascending order in fp64 (fma).
// logc[offset_k + t] = log p(o_t | o_0 .. o_{t-1}); their sum over a trajectory is its log-likelihood.  The
// conversion to float is the last operation.
//
//   k_filter_sweep  (N <= 8, gaussian / discrete) the layout, warm-up, loads and recursion of k_score_fwd
//                   (score_kernels.hpp): one lane per chunk of the E-step's chunk plan, the N-vector in registers,
//                   the model as uniform operands, score_steps prefetch, score_emit, B^T in padded LDS rows,
//                   power-of-two rescale.  New is the last stage of every step of the chunk: the rescaled
//                   vector times the reciprocal of its sum, stored as one record (marg_store) or projected
//                   (marg_project), and
//                       log c_t = (e + pe) ln 2 + log sum(a_t) - log sum(a_{t-1})
//                   with the previous logarithm kept (one log per step).  A vector that is all zero gives a
//                   zero row and -inf from then on.  Per chunk: the entry vector it assumed, the exit vector it
//                   computed, and whether either is all zero.
//   k_filter_check  the rule of k_score_check on these vectors; all-zero vectors are not compared.
//   k_filter_first_dead / k_filter_bury   a chunk that starts more than W steps after its trajectory reached
//                   probability zero warms up from the uniform vector and emits rows that are not zero: per
//                   trajectory the first chunk whose exit vector is all zero, then every LATER chunk of that
//                   trajectory is overwritten with zero rows and -inf.
//   k_filter_seg_check / k_filter_seg_bury   the same two rules over the segment plan of the 9..64-state path
//                   (k_filter_wide, filter_wide_kernels.hpp); k_filter_first_dead serves both plans.
//   k_filter_serial the exact path: one workgroup per trajectory, the serial recursion of k_score_serial with the
//                   states spread over the threads; writes the normalised row (or its projection) and log c_t
//                   every step.  Any n and explicit pobs; for N <= 8 the fallback after two failed checks.  With a
//                   table `only`: the marked trajectories alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marg_kernels.hpp" // marg_store, marg_project, MARG_QMAX (and score_kernels.hpp through post_kernels.hpp)
#include "score_kernels.hpp"

namespace bhmm {

constexpr double FILTER_LN2 = 0.6931471805599453;

// rows == nullptr: no rows; WANT_LOGC false: logc is not touched.  out rows: [total][PROJ ? Q : N].
template <int N, int KIND, bool BT_LDS, typename OT, bool PROJ, bool WANT_LOGC>
__global__ __launch_bounds__(64) void k_filter_sweep(const Model<N> *__restrict__ mp, int W, const Chunks ch, int G,
                                                     const void *__restrict__ obs_ci, const void *__restrict__ obs_rm,
                                                     const double *__restrict__ Bt_g, int M, OT *__restrict__ rows,
                                                     const double *__restrict__ V, int Q, OT *__restrict__ logc,
                                                     double *__restrict__ a_entry, double *__restrict__ a_exit,
                                                     uint8_t *__restrict__ dead)
{
    using T = score_obs_t<KIND>;
    extern __shared__ double sBt[];
    const Model<N> &m = *mp;
    const double *Bt = Bt_g;
    if constexpr (KIND == EMIT_DISC && BT_LDS) {
        for (int e = threadIdx.x; e < M * N; e += blockDim.x)
            sBt[(e / N) * score_bt_stride(N) + e % N] = Bt_g[e];
        __syncthreads();
        Bt = sBt;
    }
    constexpr int BS = BT_LDS ? score_bt_stride(N) : N; // row stride of B^T
    const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= G)
        return;
    const int len = ch.len[g];
    if (len <= 0)
        return;
    const int64_t t0 = ch.t0[g];
    const int64_t goff = ch.goff[g];
    const int64_t tstart = goff - t0; // first step of the trajectory in the concatenated arrays
    const T *rm = static_cast<const T *>(obs_rm);
    const T *ci = static_cast<const T *>(obs_ci);

    double a[N];
    double lp = 0.0;   // log of the sum of the previous step's rescaled vector (0: the step starts the trajectory)
    bool init = false; // the next step starts the trajectory: alpha_0 = pi o p_0
    auto step = [&](T o, int64_t i, bool emit) {
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
                for (int i2 = 0; i2 < N; ++i2)
                    acc = fma(a[i2], m.A[i2 * N + j], acc);
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
        if (emit) {
            double s = a[0];
#pragma unroll
            for (int j = 1; j < N; ++j)
                s += a[j];
            const bool live = s > 0.0;
            if (rows) {
                const double r = live ? 1.0 / s : 0.0; // (probability zero: a row of zeros)
                double row[N];
#pragma unroll
                for (int j = 0; j < N; ++j)
                    row[j] = a[j] * r;
                if constexpr (PROJ)
                    marg_project<N, OT>(rows + (goff + i) * Q, row, N, V, Q);
                else
                    marg_store<N, OT>(rows + (goff + i) * N, row);
            }
            if constexpr (WANT_LOGC) {
                const double ls = log(s);
                logc[goff + i] = (OT)(live ? (double)(e + pe) * FILTER_LN2 + ls - lp : -INFINITY);
                lp = ls;
            }
        }
    };

    // ---- entry vector ----
    double ent[N];
    if (t0 == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j)
            ent[j] = m.pi[j];
        init = true;
    } else {
        const int64_t w0 = t0 > W ? t0 - W : 0;
#pragma unroll
        for (int j = 0; j < N; ++j)
            a[j] = 1.0 / N;
        init = w0 == 0;
        score_steps(t0 - w0, [&](int64_t i) { return rm[tstart + w0 + i]; },
                    [&](T o, int64_t i) { step(o, i, false); });
#pragma unroll
        for (int j = 0; j < N; ++j)
            ent[j] = a[j];
    }
    double se = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j)
        se += ent[j];
    if constexpr (WANT_LOGC)
        lp = t0 == 0 ? 0.0 : log(se); // (ent is then the rescaled vector of step t0 - 1, summed in the same order)

    // ---- sweep over the chunk (CI observations: one record per step and group of 64 chunks) ----
    const int lane = (int)(g & 63);
    score_steps((int64_t)len, [&](int64_t i) { return ci[ci_rec(g, (int)i, ch.Lmax) * 64 + lane]; },
                [&](T o, int64_t i) { step(o, i, true); });

    double sx = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        sx += a[j];
        a_entry[g * N + j] = ent[j];
        a_exit[g * N + j] = a[j];
    }
    dead[g] = sx > 0.0 ? 0 : 1; // the exit vector is all zero
}

// boundary check: *fails counts the boundaries out of tolerance.  Componentwise relative after normalisation
// (k_score_check).  The chunks after the first dead one of a trajectory have no boundary to check: the
// probability is zero there and k_filter_bury rewrites them.  An all-zero entry after a live exit is a failure
template <int N>
__global__ __launch_bounds__(256) void k_filter_check(const Chunks ch, int G, const double *__restrict__ a_entry,
                                                      const double *__restrict__ a_exit,
                                                      const int32_t *__restrict__ first_dead, double tol,
                                                      unsigned int *fails)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G || ch.len[g] <= 0 || ch.t0[g] == 0)
        return;
    if (g > first_dead[ch.traj[g]])
        return;
    const double *x = a_entry + g * N, *y = a_exit + (g - 1) * N;
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
        atomicAdd(fails, 1u);
}

// per trajectory: first_dead[k] = its first chunk whose exit vector is all zero, or INT32_MAX.  One wavefront
// per trajectory; traj_c0: [K + 1] first chunk of each trajectory
[[maybe_unused]] static __global__ __launch_bounds__(64) void k_filter_first_dead(const int32_t *__restrict__ traj_c0,
                                                                                 const uint8_t *__restrict__ dead,
                                                                                 int32_t *__restrict__ first_dead)
{
    const int k = blockIdx.x;
    int best = INT32_MAX;
    for (int g = traj_c0[k] + (int)threadIdx.x; g < traj_c0[k + 1]; g += 64)
        if (dead[g]) {
            best = g; // (ascending per lane: the first hit is the lane's smallest)
            break;
        }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        best = min(best, __shfl_xor(best, h, 64));
    if (threadIdx.x == 0)
        first_dead[k] = best;
}

// every chunk after the first dead one of its trajectory: zero rows and -inf.  One lane per chunk
template <typename OT>
__global__ __launch_bounds__(256) void k_filter_bury(const Chunks ch, int G, const int32_t *__restrict__ first_dead,
                                                     OT *__restrict__ rows, int Qp, OT *__restrict__ logc)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G)
        return;
    const int len = ch.len[g];
    if (len <= 0 || g <= first_dead[ch.traj[g]])
        return;
    const int64_t goff = ch.goff[g];
    for (int s = 0; s < len; ++s) {
        if (rows)
            for (int q = 0; q < Qp; ++q)
                rows[(goff + s) * Qp + q] = (OT)0.0;
        if (logc)
            logc[goff + s] = (OT)-INFINITY;
    }
}

// ---- the same two rules over a segment plan (9..64 states, k_filter_wide in filter_wide_kernels.hpp) ---------
// k_filter_first_dead serves both plans as it is (traj_c0: the plan's first segment of each trajectory).
struct FiltSegs {
    const int32_t *traj; // trajectory of the segment
    const int64_t *t0;   // first step inside the trajectory
    const int32_t *len;
    const int64_t *off;  // [K + 1] trajectory offsets
    int nseg;
};

// k_filter_check on segment records of n doubles: one lane per boundary (the segments of a trajectory are
// consecutive, so the predecessor of a segment with t0 != 0 is s - 1)
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_filter_seg_check(const FiltSegs sg, int n,
                                                                                const double *__restrict__ a_entry,
                                                                                const double *__restrict__ a_exit,
                                                                                const int32_t *__restrict__ first_dead,
                                                                                double tol, unsigned int *fails)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= sg.nseg || sg.len[s] <= 0 || sg.t0[s] == 0)
        return;
    if (s > first_dead[sg.traj[s]])
        return;
    const double *x = a_entry + s * n, *y = a_exit + (s - 1) * n;
    double sx = 0.0, sy = 0.0;
    for (int j = 0; j < n; ++j) {
        sx += x[j];
        sy += y[j];
    }
    double dev = 0.0;
    if (!(sx > 0.0) || !(sy > 0.0)) {
        dev = 1.0;
    } else {
        for (int j = 0; j < n; ++j) {
            const double xs = x[j] / sx, ys = y[j] / sy;
            const double d = fabs(xs - ys);
            const double rel = (ys > 1e-280) ? d / ys : (d > 1e-280 ? 1.0 : 0.0);
            dev = fmax(dev, rel == rel ? rel : 1.0);
        }
    }
    if (!(dev <= tol))
        atomicAdd(fails, 1u);
}

// k_filter_bury over segments: one wavefront per segment (a segment is thousands of steps long)
template <typename OT>
__global__ __launch_bounds__(64) void k_filter_seg_bury(const FiltSegs sg, const int32_t *__restrict__ first_dead,
                                                        OT *__restrict__ rows, int Qp, OT *__restrict__ logc)
{
    const int s = blockIdx.x;
    const int len = sg.len[s];
    if (len <= 0 || s <= first_dead[sg.traj[s]])
        return;
    const int64_t g0 = sg.off[sg.traj[s]] + sg.t0[s];
    if (rows)
        for (int64_t e = threadIdx.x; e < (int64_t)len * Qp; e += 64)
            rows[g0 * Qp + e] = (OT)0.0;
    if (logc)
        for (int e = threadIdx.x; e < len; e += 64)
            logc[g0 + e] = (OT)-INFINITY;
}

// ---- exact path ----------------------------------------------------------------------------
// grid K, blockDim a multiple of 64 with n <= SCORE_SERIAL_R * blockDim; LDS: n + 16 doubles.  Model: A [n][n],
// pi [n], par0 [n] (gaussian mu) / [n][M] (discrete B), par1 [n] (gaussian sigma).  Explicit pobs: obs_rm holds
// n doubles per step, read as given.  rows: [total][Q > 0 ? Q : n] or nullptr; logc: [total] or nullptr.
// only: nullptr (every trajectory), or one byte per trajectory -- a workgroup whose trajectory is not marked returns
// at once (filter_path 3: the trajectories with a segment outside the range of k_filter_tile)
template <int KIND, typename OT>
__global__ __launch_bounds__(1024) void k_filter_serial(int n, int M, const int64_t *__restrict__ offsets,
                                                        const void *__restrict__ obs_rm, const double *__restrict__ A,
                                                        const double *__restrict__ pi, const double *__restrict__ par0,
                                                        const double *__restrict__ par1, const double *__restrict__ V,
                                                        int Q, OT *__restrict__ rows, OT *__restrict__ logc,
                                                        const uint8_t *__restrict__ only)
{
    extern __shared__ double sh[];
    double *alpha = sh, *red = sh + n;
    const int k = blockIdx.x;
    if (only != nullptr && only[k] == 0) // (uniform over the workgroup)
        return;
    const int64_t base = offsets[k], T = offsets[k + 1] - base;
    const int bd = blockDim.x, tid = threadIdx.x;
    const int Qp = Q > 0 ? Q : n;
    double lp = 0.0;
    int64_t t = 0;
    for (; t < T; ++t) {
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
        int pe = 0;
        if constexpr (KIND == EMIT_GAUSS) {
            pmx = score_block_reduce(pmx, true, red);
            if (pmx < 0x1p-959) {
#pragma unroll
                for (int r = 0; r < SCORE_SERIAL_R; ++r)
                    p[r] = tid + r * bd < n ? (pmx == 0.0 ? 1.0 : ldexp(p[r], 900)) : 0.0;
                pe = pmx == 0.0 ? 0 : -900;
            }
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
        if (mx == 0.0)
            break; // (block-uniform) probability zero from this step on
        const int e = exponent_of(mx);
        double part = 0.0;
#pragma unroll
        for (int r = 0; r < SCORE_SERIAL_R; ++r)
            if (tid + r * bd < n) {
                const double x = ldexp(v[r], -e);
                alpha[tid + r * bd] = x;
                part += x;
            }
        const double s = score_block_reduce(part, false, red); // (its barriers publish alpha)
        const double rs = 1.0 / s;
        if (rows) {
            OT *dst = rows + (base + t) * Qp;
            if (Q > 0) {
                if (tid < Q) {
                    double acc = 0.0;
                    for (int i = 0; i < n; ++i)
                        acc = fma(alpha[i] * rs, V[i * Q + tid], acc);
                    dst[tid] = (OT)acc;
                }
            } else {
                for (int j = tid; j < n; j += bd)
                    dst[j] = (OT)(alpha[j] * rs);
            }
        }
        if (logc) {
            const double ls = log(s);
            if (tid == 0)
                logc[base + t] = (OT)((double)(e + pe) * FILTER_LN2 + ls - lp);
            lp = ls;
        }
        __syncthreads(); // (the next step overwrites alpha)
    }
    // the steps from the first one of probability zero on
    for (int64_t u = t; u < T; ++u) {
        if (rows)
            for (int q = tid; q < Qp; q += bd)
                rows[(base + u) * Qp + q] = (OT)0.0;
        if (logc && tid == 0)
            logc[base + u] = (OT)-INFINITY;
    }
}

} // namespace bhmm
