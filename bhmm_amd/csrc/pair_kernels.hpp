// pair_kernels.hpp -- pair posteriors of every step (bhmm_posterior_transitions, pair_api.hip):
// xi_t(i,j) = P(s_t = i, s_t+1 = j | O) of the transition t -> t+1, handed out as out[(offset_k + t) * Q' + q],
// trajectory-major rows, double or float; the last row of every trajectory (t = T_k - 1) is zero.
//   jump form      (no weights, Q' = 1): sum_{i != j} xi_t(i,j)
//   projected form (W[n][n][Q] row-major, Q' = Q <= 8): sum_i sum_j xi_t(i,j) W[i][j][q]
// Both accumulate the unnormalised pairs x_ij in fp64 with i the outer and j the inner loop, both ascending
// (fma for the projection), and normalise with ONE multiplication by the reciprocal of sum_ij x_ij (summed in
// the same order).  The jump form is the projection on the off-diagonal 0/1 mask with the loads of W left out:
// fma(x, 1, acc) = acc + x and fma(x, 0, acc) = acc, so the two are bitwise equal.  The conversion to float is
// the last operation.
//
//   k_pair_sweep   (N <= 8, gaussian / discrete) the sweep of k_marg_sweep (marg_kernels.hpp: same chunk plan,
//                  warm-ups, workspace, prefetch, boundary vectors) restated as pair_sweep_lane -- a sibling, not a
//                  parameter of marg_sweep_lane, so that the existing kernels stay what they are.  The pair stage
//                  hangs off the backward sweep: bstep at step s forms pb_s = p_s o beta_s before it applies A and
//                  keeps it; at the next item, step s - 1, the stored alpha_(s-1) arrives and
//                  x_ij = alpha_(s-1)(i) A_ij pb_s(j) goes to row goff + s - 1.  The pair that straddles a chunk
//                  edge, (t0 - 1, t0), is written by the chunk that owns t0 from its entry vector ent (alpha of
//                  t0 - 1: the vector k_post_check verifies against the neighbour's exit) and its own pb_0, never
//                  from a pb of the backward warm-up.  The chunk that holds t = T_k - 1 writes the zero row.  Every
//                  row is written exactly once per pass, nothing is read back.
//   k_pair_rows    the generic path, any n: from the filtered rows f_t and the posterior rows gamma_(t+1),
//                  x_ij = f_t(i) A_ij gamma_(t+1)(j) / pred_j with pred_j = sum_i f_t(i) A_ij.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marg_kernels.hpp"

namespace bhmm {

constexpr int PAIR_QMAX = 8; // columns of a projection

// up to four values of one record, columns [q0, q0 + cnt) of Q, in marg_store's widths where the record's size
// keeps them aligned (dst: the record's column q0 in a 16-byte aligned array)
template <typename OT>
__device__ __forceinline__ void pair_store4(OT *__restrict__ dst, const double (&v)[4], int cnt, int Q)
{
    if (cnt == 4 && (sizeof(OT) == 8 ? Q % 2 == 0 : Q % 4 == 0)) {
        marg_store<4, OT>(dst, v);
    } else if (cnt >= 2 && Q % 2 == 0) { // (then cnt is 2 or 4)
        const double lo[2] = {v[0], v[1]}, hi[2] = {v[2], v[3]};
        marg_store<2, OT>(dst, lo);
        if (cnt == 4)
            marg_store<2, OT>(dst + 2, hi);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u < cnt)
                dst[u] = (OT)v[u];
    }
}

// one row from the vector of step t (a: alpha_t up to a factor) and pb = p_(t+1) o beta_(t+1) (up to a factor)
template <int N, typename OT, bool PROJ>
struct PairRow {
    OT *__restrict__ out;
    const double *__restrict__ Wt; // [N][N][PAIR_QMAX]: the Q columns padded with zeros, uniform
    int Q;
    __device__ __forceinline__ PairRow(OT *o, const double *w, int q) : out(o), Wt(w), Q(q) {}

    __device__ __forceinline__ void operator()(const Model<N> &m, const double (&a)[N], const double (&pb)[N],
                                               int64_t idx) const
    {
        // no contraction here: x_ij is the rounded product in both forms, whatever else it feeds
#pragma clang fp contract(off)
        double sum = 0.0;
        if constexpr (PROJ) {
            // four columns at a time (one or two trips; x_ij and their sum are formed again in the second, the
            // same values): every column is one chain over the pairs in the stated order
            for (int q0 = 0; q0 < Q; q0 += 4) {
                double acc[4] = {0.0, 0.0, 0.0, 0.0};
                sum = 0.0;
#pragma unroll
                for (int i = 0; i < N; ++i) {
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        const double x = (a[i] * m.A[i * N + j]) * pb[j];
                        sum += x;
                        const double *w = Wt + (i * N + j) * PAIR_QMAX + q0;
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            acc[u] = fma(x, w[u], acc[u]);
                    }
                }
                const double r = 1.0 / sum; // (a trajectory of probability zero: 0 * inf, NaN rows as the marginals')
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    acc[u] *= r;
                pair_store4<OT>(out + idx * Q + q0, acc, Q - q0 < 4 ? Q - q0 : 4, Q);
            }
        } else {
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const double x = (a[i] * m.A[i * N + j]) * pb[j];
                    sum += x;
                    if (i != j)
                        acc += x;
                }
            }
            const double r = 1.0 / sum;
            out[idx] = (OT)(acc * r);
        }
    }

    // the row of a trajectory's last step
    __device__ __forceinline__ void zero(int64_t idx) const
    {
        if constexpr (PROJ) {
            for (int q = 0; q < Q; ++q)
                out[idx * Q + q] = (OT)0.0;
        } else {
            out[idx] = (OT)0.0;
        }
    }
};

// The sweep of one lane (one chunk): marg_sweep_lane's (marg_kernels.hpp), statement for statement, up to the
// backward sweep, whose bstep keeps pb = p o beta of the step it consumed and whose last stage is the pair row
// (header comment).  Arguments as marg_sweep_lane.
template <int N, int KIND, bool BT_LDS, class Row>
__device__ __forceinline__ void pair_sweep_lane(const Model<N> &m, int W, const Chunks &ch, int G, int grp0,
                                                const int64_t *__restrict__ offsets,
                                                const void *__restrict__ obs_ci, const void *__restrict__ obs_rm,
                                                const double *Bt, double *__restrict__ ws, const Row &row,
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
    // b = beta of the step whose observation the next bstep consumes: beta_t = A (p_{t+1} o beta_{t+1});
    // pb = p o beta of the step the last bstep consumed
    double b[N], pb[N];
    auto bstep = [&](T o) {
        double p[N];
        int pe;
        score_emit<N, KIND, BS>(m, Bt, o, p, pe);
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
    for (int j = 0; j < N; ++j) {
        b[j] = 1.0;
        pb[j] = 0.0;
    }
    if (u > tend) // steps u - 1 .. tend; step i consumes the observation of step u - i
        score_steps(u - tend, [&](int64_t i) { return rm[tstart + u - i]; }, [&](T o, int64_t) { bstep(o); });
    double sb = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        sb += b[j];
        b_assumed[g * N + j] = b[j];
    }

    // sweep back: item i is step s = len - 1 - i of the chunk.  Item 0 has no pb of this sweep: its pair
    // (tend, tend + 1) is the next chunk's, or tend is the trajectory's last step and its row is zero
    const int64_t goff = ch.goff[g];
    if (tend == Tk - 1)
        row.zero(goff + len - 1);
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
            if (i > 0)
                row(m, in.a, pb, goff + (len - 1 - i)); // alpha_s with pb of step s + 1
            bstep(in.o); // (after step 0: beta of the step before the chunk, pb of step 0)
        });
    if (t0 > 0)
        row(m, ent, pb, goff - 1); // the straddling pair (t0 - 1, t0)
    double so = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        so += b[j];
        b_out[g * N + j] = b[j];
    }
    dead[g] = !(se > 0.0 && sx > 0.0 && sb > 0.0 && so > 0.0);
}

// OT: double or float.  Arguments as k_marg_sweep; out: [total][PROJ ? Q : 1], 16-byte aligned; Wt: [N][N][PAIR_QMAX],
// the Q columns of the weights padded with zeros.
template <int N, int KIND, bool BT_LDS, typename OT, bool PROJ>
__global__ __launch_bounds__(64) void k_pair_sweep(const Model<N> *__restrict__ mp, int W, const Chunks ch, int G,
                                                   int grp0, const int64_t *__restrict__ offsets,
                                                   const void *__restrict__ obs_ci, const void *__restrict__ obs_rm,
                                                   const double *__restrict__ Bt_g, int M, double *__restrict__ ws,
                                                   OT *__restrict__ out, const double *__restrict__ Wt, int Q,
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
    const PairRow<N, OT, PROJ> row(out, Wt, Q);
    pair_sweep_lane<N, KIND, BT_LDS>(*mp, W, ch, G, grp0, offsets, obs_ci, obs_rm, Bt, ws, row, a_entry, a_exit,
                                     b_assumed, b_out, dead);
}

// ---- generic path: over filtered rows and posterior rows -----------------------------------------
// One thread per step e of the concatenated arrays.  filt: [total][n] filtered rows; gam: [total][n] posterior
// rows, of which row e + 1 belongs to thread e alone and is overwritten with gamma_(e+1)(j) / pred_j (0 where
// pred_j == 0: gamma is zero there as well).  A: [n][n] row-major.  Wt: [n][n][PAIR_QMAX], padded; Q == 0: the
// jump form.
template <typename OT>
__global__ __launch_bounds__(64) void k_pair_rows(const double *__restrict__ filt, double *gam,
                                                  const double *__restrict__ A, int n, int64_t total, int K,
                                                  const int64_t *__restrict__ offsets,
                                                  const double *__restrict__ Wt, int Q, OT *__restrict__ out)
{
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total)
        return;
    const int Qp = Q > 0 ? Q : 1;
    // the trajectory of step e: the last k with offsets[k] <= e
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= e)
            lo = mid;
        else
            hi = mid;
    }
    if (e == offsets[lo + 1] - 1) { // the last step of its trajectory
        for (int q = 0; q < Qp; ++q)
            out[e * Qp + q] = (OT)0.0;
        return;
    }
    const double *f = filt + e * n;
    double *c = gam + (e + 1) * n;
    for (int j0 = 0; j0 < n; j0 += 8) { // pred_j over i ascending, eight columns at a time
        double pred[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            pred[u] = 0.0;
        for (int i = 0; i < n; ++i) {
            const double fi = f[i];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 + u < n)
                    pred[u] = fma(fi, A[(int64_t)i * n + j0 + u], pred[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (j0 + u < n)
                c[j0 + u] = pred[u] > 0.0 ? c[j0 + u] / pred[u] : 0.0;
    }
    double sum = 0.0;
    double acc[PAIR_QMAX];
#pragma unroll
    for (int q = 0; q < PAIR_QMAX; ++q)
        acc[q] = 0.0;
    for (int i = 0; i < n; ++i) {
        const double fi = f[i];
        for (int j = 0; j < n; ++j) {
            const double x = (fi * A[(int64_t)i * n + j]) * c[j];
            sum += x;
            if (Q == 0) {
                if (i != j)
                    acc[0] += x;
            } else {
                const double *w = Wt + ((int64_t)i * n + j) * PAIR_QMAX;
#pragma unroll
                for (int q = 0; q < PAIR_QMAX; ++q)
                    if (q < Q)
                        acc[q] = fma(x, w[q], acc[q]);
            }
        }
    }
    const double r = 1.0 / sum;
#pragma unroll
    for (int q = 0; q < PAIR_QMAX; ++q)
        if (q < Qp)
            out[e * Qp + q] = (OT)(acc[q] * r);
}

} // namespace bhmm
