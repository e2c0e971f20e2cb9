// post_kernels.hpp -- posterior (maximum-posterior-marginal) decoding on the loaded observations
// (bhmm_posterior_decode, post_api.hip): path[t] = argmax_i gamma_t(i) (lowest index on equal gamma) and
// conf[t] = max_i gamma_t(i), without a gamma row in memory.  Nothing of the E-step's state is read or
// written: the kernels take the context's chunk plan and observation layouts and write to buffers of
// their own.
//
//   k_post_sweep   (N <= 8, gaussian / discrete) scoring's layout 1: one lane per chunk, the whole
//                  N-vector in registers, N instantiated exactly, the model uniform (scalar loads), B^T
//                  staged in LDS rows of score_bt_stride.  A workgroup is one record group of 64 chunks.
//                  Per lane:
//                    forward   warm-up of W steps before the chunk from the uniform vector (exactly from
//                              pi when the trajectory starts within W steps); sweep over the chunk with
//                              the power-of-two rescale; every rescaled alpha row goes to the workspace,
//                              ws[((group * Lmax + step) * N + state) * 64 + lane] (each store of a
//                              wavefront is one 512-byte line)
//                    backward  warm-up of W steps beyond the chunk end from the all-ones vector (exact
//                              when the trajectory ends within W steps: beta_{T-1} = 1, and the uniform
//                              vector is the same direction); sweep back over the chunk: alpha_t o beta_t,
//                              its argmax and max / sum, one byte (or int) and optionally one float per
//                              step.  The alpha rows come back from the workspace POST_PF steps ahead of
//                              their use.  No gamma row, no beta row, no statistics.
//                  and writes the alpha vector it assumed at the chunk's entry and the one it computed at its
//                  exit, the beta vector it assumed at the chunk's last step and the one it computed for
//                  the step before the chunk.
//   k_post_check   each assumed vector against the one its neighbour computed, both directions:
//                  componentwise relative after normalisation (the rule of k_score_check), one counter.
//   k_post_gamma_rm / k_post_gamma_ci   the generic path: argmax and max over gamma rows an E-step stored
//                  (trajectory-major rows of n / CI records of N padded), same tie rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "score_kernels.hpp" // score_emit, score_steps, score_bt_stride (and Model, Chunks, ci_rec)

namespace bhmm {

constexpr int POST_PF = 4; // backward sweep: observation and alpha row loaded this many steps ahead

template <int N, int KIND>
struct PostIn {
    score_obs_t<KIND> o;
    double a[N];
};

// score_steps with a prefetch distance of its own (the items carry an alpha row: 2 * PF * (N + 1) doubles)
template <int PF, class Load, class Step>
__device__ __forceinline__ void post_steps(int64_t n, Load load, Step step)
{
    using T = decltype(load(int64_t(0)));
    T cur[PF], nxt[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u)
        cur[u] = load(min((int64_t)u, n - 1));
    for (int64_t i0 = 0; i0 < n; i0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u)
            nxt[u] = load(min(i0 + PF + u, n - 1));
#pragma unroll
        for (int u = 0; u < PF; ++u)
            if (i0 + u < n)
                step(cur[u], i0 + u);
#pragma unroll
        for (int u = 0; u < PF; ++u)
            cur[u] = nxt[u];
    }
}

// grid: the record groups [grp0, grp0 + gridDim.x) of the chunk plan; ws holds the rows of these groups only
// (gridDim.x * Lmax * N * 64 doubles).  PT: uint8_t or int32_t.  offsets: [K + 1] trajectory offsets.
// Boundary vectors [Gp][N]; dead[g] != 0: a vector of chunk g is all zero (probability zero: no check).
template <int N, int KIND, bool BT_LDS, typename PT>
__global__ __launch_bounds__(64) void k_post_sweep(const Model<N> *__restrict__ mp, int W, const Chunks ch, int G,
                                                   int grp0, const int64_t *__restrict__ offsets,
                                                   const void *__restrict__ obs_ci, const void *__restrict__ obs_rm,
                                                   const double *__restrict__ Bt_g, int M, double *__restrict__ ws,
                                                   PT *__restrict__ path, float *__restrict__ conf,
                                                   double *__restrict__ a_entry, double *__restrict__ a_exit,
                                                   double *__restrict__ b_assumed, double *__restrict__ b_out,
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
    uint64_t acc8 = 0; // one byte per step: the states of up to 8 consecutive steps, lowest address in the low byte
    int cnt8 = 0;
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
            const int64_t s = len - 1 - i, idx = goff + s;
            double best = in.a[0] * b[0], sum = best;
            int arg = 0;
#pragma unroll
            for (int j = 1; j < N; ++j) {
                const double q = in.a[j] * b[j];
                sum += q;
                if (q > best) { // (strictly: the lowest index wins on equal gamma)
                    best = q;
                    arg = j;
                }
            }
            if (conf)
                conf[idx] = (float)(best / sum);
            if constexpr (sizeof(PT) == 1) {
                acc8 = (acc8 << 8) | (uint64_t)arg;
                ++cnt8;
                if ((idx & 7) == 0 || s == 0) {
                    if (cnt8 == 8) { // (then idx is a multiple of 8: a run is cut at every one)
                        *reinterpret_cast<uint64_t *>(path + idx) = acc8;
                    } else {
                        for (int q = 0; q < cnt8; ++q)
                            path[idx + q] = (PT)((acc8 >> (8 * q)) & 0xff);
                    }
                    acc8 = 0;
                    cnt8 = 0;
                }
            } else {
                path[idx] = (PT)arg;
            }
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

// x: assumed, y: computed by the neighbour
template <int N>
__device__ __forceinline__ double post_dev(const double *x, const double *y)
{
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        sx += x[j];
        sy += y[j];
    }
    if (!(sx > 0.0) || !(sy > 0.0))
        return 1.0;
    double dev = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double xs = x[j] / sx, ys = y[j] / sy;
        const double d = fabs(xs - ys);
        const double rel = (ys > 1e-280) ? d / ys : (d > 1e-280 ? 1.0 : 0.0);
        dev = fmax(dev, rel);
    }
    return dev;
}

// boundary check, both directions: *fails counts the boundaries out of tolerance
template <int N>
__global__ __launch_bounds__(256) void k_post_check(const Chunks ch, int G, const double *a_entry,
                                                    const double *a_exit, const double *b_assumed,
                                                    const double *b_out, const uint8_t *dead, double tol,
                                                    unsigned int *fails)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G || g == 0 || ch.len[g] <= 0 || ch.t0[g] == 0)
        return;
    if (dead[g] || dead[g - 1])
        return; // (the trajectory's probability is zero)
    const double da = post_dev<N>(a_entry + g * N, a_exit + (g - 1) * N);
    const double db = post_dev<N>(b_assumed + (g - 1) * N, b_out + g * N);
    if (!(da <= tol) || !(db <= tol))
        atomicAdd(fails, 1u);
}

// ---- generic path: over gamma rows an E-step stored ---------------------------------------------
// rows of n doubles, trajectory-major (9 states and more)
template <typename PT>
__global__ __launch_bounds__(256) void k_post_gamma_rm(const double *__restrict__ gamma, int n, int64_t total,
                                                       PT *__restrict__ path, float *__restrict__ conf)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total)
        return;
    const double *row = gamma + t * n;
    double best = row[0];
    int arg = 0;
    for (int j = 1; j < n; ++j) {
        const double q = row[j];
        if (q > best) {
            best = q;
            arg = j;
        }
    }
    path[t] = (PT)arg;
    if (conf)
        conf[t] = (float)best;
}

// CI records of N padded doubles over the chunk plan (up to 8 states); one lane per chunk
template <int N, typename PT>
__global__ __launch_bounds__(256) void k_post_gamma_ci(const Chunks ch, int G, const double *__restrict__ gamma_ci,
                                                       int nreal, PT *__restrict__ path, float *__restrict__ conf)
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
        double best = v[0];
        int arg = 0;
#pragma unroll
        for (int j = 1; j < N; ++j)
            if (j < nreal && v[j] > best) {
                best = v[j];
                arg = j;
            }
        path[off + s] = (PT)arg;
        if (conf)
            conf[off + s] = (float)best;
    }
}

} // namespace bhmm
