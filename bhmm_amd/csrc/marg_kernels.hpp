// marg_kernels.hpp -- posterior state probabilities of every step (bhmm_posterior_marginals, marg_api.hip):
// out[(offset_k + t) * Q' + q], trajectory-major rows of Q' values, double or float.  Without a projection
// Q' = n and the row is gamma_t(.); with V ([n][Q] row-major, Q <= 8) Q' = Q and the row is
// sum_i gamma_t(i) V[i][q], accumulated over i in ascending order in fp64 (fma).  The conversion to float is
// the last operation.
//
//   k_marg_sweep   (N <= 8, gaussian / discrete) the sweep of k_post_sweep (post_kernels.hpp: same chunk plan,
//                  warm-ups, workspace, prefetch, boundary vectors) restated as the device template
//                  marg_sweep_lane with an emit policy as last stage -- a sibling, not a shared template:
//                  sharing it changed k_post_sweep's register allocation.  MargRow: per
//                  step alpha_t o beta_t times the reciprocal of its sum, written as one contiguous record of
//                  Q' values at its trajectory-major position (16-byte stores where the record's size allows).
//                  V is read through a uniform pointer (all lanes the same address: scalar loads).
//   k_marg_rows_rm / k_marg_rows_ci   the generic path: convert / project gamma rows an E-step stored
//                  (trajectory-major rows of n / CI records of N padded).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "post_kernels.hpp"

namespace bhmm {

constexpr int MARG_QMAX = 8; // columns of a projection

// NV values to dst as OT in the widest stores the record's size keeps aligned (dst: record NV * sizeof(OT)
// bytes into a 16-byte aligned array)
template <int NV, typename OT>
__device__ __forceinline__ void marg_store(OT *__restrict__ dst, const double (&v)[NV])
{
    constexpr int BYTES = NV * (int)sizeof(OT);
    if constexpr (sizeof(OT) == 8 && BYTES % 16 == 0) {
#pragma unroll
        for (int q = 0; q < NV / 2; ++q)
            reinterpret_cast<double2 *>(dst)[q] = make_double2(v[2 * q], v[2 * q + 1]);
    } else if constexpr (sizeof(OT) == 4 && BYTES % 16 == 0) {
#pragma unroll
        for (int q = 0; q < NV / 4; ++q)
            reinterpret_cast<float4 *>(dst)[q] =
                make_float4((float)v[4 * q], (float)v[4 * q + 1], (float)v[4 * q + 2], (float)v[4 * q + 3]);
    } else if constexpr (sizeof(OT) == 4 && BYTES % 8 == 0) {
#pragma unroll
        for (int q = 0; q < NV / 2; ++q)
            reinterpret_cast<float2 *>(dst)[q] = make_float2((float)v[2 * q], (float)v[2 * q + 1]);
    } else {
#pragma unroll
        for (int q = 0; q < NV; ++q)
            dst[q] = (OT)v[q];
    }
}

// row of a projection: acc_q = sum_i g[i] V[i][q], i ascending
template <int N, typename OT>
__device__ __forceinline__ void marg_project(OT *__restrict__ dst, const double (&g)[N], int nreal,
                                             const double *__restrict__ V, int Q)
{
    for (int q = 0; q < Q; ++q) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (i < nreal)
                acc = fma(g[i], V[i * Q + q], acc);
        dst[q] = (OT)acc;
    }
}

// The sweep of one lane (one chunk): k_post_sweep's (post_kernels.hpp), statement for statement, up to the last
// stage of the backward sweep, which is the emit policy: emit(a, b, idx, s) is called once per step with the
// rescaled alpha and beta rows of the step, its position idx in the concatenated arrays and its position s in
// the chunk (the steps arrive in DESCENDING order).  The record groups [grp0, grp0 + gridDim.x) of the chunk
// plan; ws holds the rows of these groups only (gridDim.x * Lmax * N * 64 doubles).  offsets: [K + 1] trajectory
// offsets.  Bt: the table the sweep reads (LDS or global).
// Boundary vectors [Gp][N]; dead[g] != 0: a vector of chunk g is all zero (probability zero: no check).
template <int N, int KIND, bool BT_LDS, class Emit>
__device__ __forceinline__ void marg_sweep_lane(const Model<N> &m, int W, const Chunks &ch, int G, int grp0,
                                                const int64_t *__restrict__ offsets,
                                                const void *__restrict__ obs_ci, const void *__restrict__ obs_rm,
                                                const double *Bt, double *__restrict__ ws, Emit &emit,
                                                double *__restrict__ a_entry, double *__restrict__ a_exit,
                                                double *__restrict__ b_assumed, double *__restrict__ b_out,
                                                uint8_t *__restrict__ dead)
{
    using T = score_obs_t<KIND>;
    constexpr int BS = BT_LDS ? score_bt_stride(N) : N; // row stride of B^T
    const int lane = threadIdx.x;
    const int64_t g = ((int64_t)grp0 + blockIdx.x) * 64 + lane;
    if (g >= G)
        return;
    const int len = ch.len[g];
    if (len <= 0)
        return;
    const int64_t t0 = ch.t0[g];
    const int64_t tstart = ch.goff[g] - t0; // first step of the trajectory in the concatenated arrays
    const int k = ch.traj[g];
    const int64_t Tk = offsets[k + 1] - offsets[k];
    const T *rm = static_cast<const T *>(obs_rm);
    const T *ci = static_cast<const T *>(obs_ci);
    double *wsl = ws + (int64_t)blockIdx.x * ch.Lmax * (N * 64) + lane; // this lane's rows: + (step * N + state) * 64

    // ---------------------------------------- forward ----------------------------------------
    double a[N];
    bool init = false; // the next step starts the trajectory: alpha_0 = pi o p_0
    auto fstep = [&](T o, int64_t i, bool keep) {
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
        if (keep) {
#pragma unroll
            for (int j = 0; j < N; ++j)
                wsl[(i * N + j) * 64] = a[j];
        }
    };

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
                    [&](T o, int64_t i) { fstep(o, i, false); });
#pragma unroll
        for (int j = 0; j < N; ++j)
            ent[j] = a[j];
    }
    score_steps((int64_t)len, [&](int64_t i) { return ci[ci_rec(g, (int)i, ch.Lmax) * 64 + lane]; },
                [&](T o, int64_t i) { fstep(o, i, true); });

    double se = 0.0, sx = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        se += ent[j];
        sx += a[j];
        a_entry[g * N + j] = ent[j];
        a_exit[g * N + j] = a[j];
    }

    // ---------------------------------------- backward ---------------------------------------
    // b = beta of the step whose observation the next bstep consumes: beta_t = A (p_{t+1} o beta_{t+1})
    double b[N];
    auto bstep = [&](T o) {
        double p[N];
        int pe;
        score_emit<N, KIND, BS>(m, Bt, o, p, pe);
        double pb[N];
#pragma unroll
        for (int j = 0; j < N; ++j)
            pb[j] = p[j] * b[j];
        double v[N];
#pragma unroll
        for (int i2 = 0; i2 < N; ++i2) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j)
                acc = fma(m.A[i2 * N + j], pb[j], acc);
            v[i2] = acc;
        }
        double mx = v[0];
#pragma unroll
        for (int j = 1; j < N; ++j)
            mx = fmax(mx, v[j]);
        const int e = exponent_of(mx);
#pragma unroll
        for (int j = 0; j < N; ++j)
            b[j] = ldexp(v[j], -e);
    };

    const int64_t tend = t0 + len - 1;                          // last step of the chunk
    const int64_t u = tend + W < Tk - 1 ? tend + W : Tk - 1;    // the warm-up starts with beta_u = 1
#pragma unroll
    for (int j = 0; j < N; ++j)
        b[j] = 1.0;
    if (u > tend) // steps u - 1 .. tend; step i consumes the observation of step u - i
        score_steps(u - tend, [&](int64_t i) { return rm[tstart + u - i]; }, [&](T o, int64_t) { bstep(o); });
    double sb = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        sb += b[j];
        b_assumed[g * N + j] = b[j];
    }

    // sweep back: item i is step s = len - 1 - i of the chunk
    const int64_t goff = ch.goff[g];
    post_steps<POST_PF>(
        (int64_t)len,
        [&](int64_t i) {
            const int64_t s = len - 1 - i;
            PostIn<N, KIND> in;
            in.o = ci[ci_rec(g, (int)s, ch.Lmax) * 64 + lane];
#pragma unroll
            for (int j = 0; j < N; ++j)
                in.a[j] = wsl[(s * N + j) * 64];
            return in;
        },
        [&](const PostIn<N, KIND> &in, int64_t i) {
            const int64_t s = len - 1 - i;
            emit(in.a, b, goff + s, s);
            bstep(in.o); // (after step 0: beta of the step before the chunk)
        });
    double so = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        so += b[j];
        b_out[g * N + j] = b[j];
    }
    dead[g] = !(se > 0.0 && sx > 0.0 && sb > 0.0 && so > 0.0);
}

// emit policy of marg_sweep_lane: the normalised row, or its projection
template <int N, typename OT, bool PROJ>
struct MargRow {
    OT *__restrict__ out;
    const double *__restrict__ V;
    int Q;
    __device__ __forceinline__ MargRow(OT *o, const double *v, int q) : out(o), V(v), Q(q) {}
    __device__ __forceinline__ void operator()(const double (&a)[N], const double (&b)[N], int64_t idx, int64_t)
    {
        double g[N];
        g[0] = a[0] * b[0];
        double sum = g[0];
#pragma unroll
        for (int j = 1; j < N; ++j) {
            g[j] = a[j] * b[j];
            sum += g[j];
        }
        const double r = 1.0 / sum; // (a trajectory of probability zero: 0 * inf, NaN rows as the E-step's)
#pragma unroll
        for (int j = 0; j < N; ++j)
            g[j] *= r;
        if constexpr (PROJ)
            marg_project<N, OT>(out + idx * Q, g, N, V, Q);
        else
            marg_store<N, OT>(out + idx * N, g);
    }
};

// OT: double or float.  Arguments as k_post_sweep; out: [total][PROJ ? Q : N], 16-byte aligned.
template <int N, int KIND, bool BT_LDS, typename OT, bool PROJ>
__global__ __launch_bounds__(64) void k_marg_sweep(const Model<N> *__restrict__ mp, int W, const Chunks ch, int G,
                                                   int grp0, const int64_t *__restrict__ offsets,
                                                   const void *__restrict__ obs_ci, const void *__restrict__ obs_rm,
                                                   const double *__restrict__ Bt_g, int M, double *__restrict__ ws,
                                                   OT *__restrict__ out, const double *__restrict__ V, int Q,
                                                   double *__restrict__ a_entry, double *__restrict__ a_exit,
                                                   double *__restrict__ b_assumed, double *__restrict__ b_out,
                                                   uint8_t *__restrict__ dead)
{
    extern __shared__ double sBt[];
    const double *Bt = Bt_g;
    if constexpr (KIND == EMIT_DISC && BT_LDS) {
        for (int e = threadIdx.x; e < M * N; e += blockDim.x)
            sBt[(e / N) * score_bt_stride(N) + e % N] = Bt_g[e];
        __syncthreads();
        Bt = sBt;
    }
    MargRow<N, OT, PROJ> emit(out, V, Q);
    marg_sweep_lane<N, KIND, BT_LDS>(*mp, W, ch, G, grp0, offsets, obs_ci, obs_rm, Bt, ws, emit, a_entry, a_exit,
                                     b_assumed, b_out, dead);
}

// ---- generic path: over gamma rows an E-step stored ---------------------------------------------
// rows of n doubles, trajectory-major (9 states and more).  Q == 0: one thread per element; else one thread
// per step
template <typename OT>
__global__ __launch_bounds__(256) void k_marg_rows_rm(const double *__restrict__ gamma, int n, int64_t total,
                                                      const double *__restrict__ V, int Q, OT *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (Q == 0) {
        if (e < total * n)
            out[e] = (OT)gamma[e];
        return;
    }
    if (e >= total)
        return;
    const double *row = gamma + e * n;
    double acc[MARG_QMAX];
#pragma unroll
    for (int q = 0; q < MARG_QMAX; ++q)
        acc[q] = 0.0;
    for (int i = 0; i < n; ++i) {
        const double g = row[i];
#pragma unroll
        for (int q = 0; q < MARG_QMAX; ++q)
            if (q < Q)
                acc[q] = fma(g, V[i * Q + q], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < MARG_QMAX; ++q)
        if (q < Q)
            out[e * Q + q] = (OT)acc[q];
}

// CI records of N padded doubles over the chunk plan (up to 8 states); one lane per chunk
template <int N, typename OT>
__global__ __launch_bounds__(256) void k_marg_rows_ci(const Chunks ch, int G, const double *__restrict__ gamma_ci,
                                                      int nreal, const double *__restrict__ V, int Q,
                                                      OT *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G)
        return;
    const int lane = threadIdx.x & 63;
    const int len = ch.len[g];
    const int64_t off = ch.goff[g];
    for (int s = 0; s < len; ++s) {
        double v[N];
        ci_load<N>(gamma_ci, ci_rec(g, s, ch.Lmax), lane, v);
        if (Q > 0) {
            marg_project<N, OT>(out + (off + s) * Q, v, nreal, V, Q);
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (j < nreal)
                    out[(off + s) * nreal + j] = (OT)v[j];
        }
    }
}

} // namespace bhmm
