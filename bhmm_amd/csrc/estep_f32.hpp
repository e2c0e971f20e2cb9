// estep_f32.hpp -- single-precision E-step for up to 8 states (BHMM_FLAG_SINGLE, estep_f32.hip).
//
// Same chunk plan and observations as the fp64 sweep (estep_sweep.hpp): H = N/2 lanes per chunk,
// lane q owns the state pair (2q, 2q+1) as one packed float pair, 64 chunks per workgroup.  One
// launch per E-step does, per chunk:
//   forward warm-up  W steps before the chunk from the uniform vector (or the exact start of the
//                    trajectory when it is closer) on the trajectory-major observations -> a_entry
//   forward sweep    alpha_t = (alpha_{t-1} A) o p_t, rescaled every step by the power of two that
//                    puts the group's largest entry in [0.5, 1); rows stored to the CI workspace
//                    (fp32); log-likelihood = exponent sum * ln 2 + log sum(alpha_end)
//                    - log sum(a_entry), the logs in fp64
//   backward warm-up W steps after the chunk from ones (or the exact end of the trajectory)
//   backward sweep   w = p_t o beta_t, u = A w, Z = alpha_{t-1} . u: beta_{t-1} = u / Z, so that
//                    alpha_t . beta_t = 1 and gamma_t = alpha_t o beta_t needs no division;
//                    xi_{t-1,t} = A o (alpha_{t-1} / Z) (x) w, the factor A applied once at the end
// Statistics are summed in fp32 over blocks of F32_BLOCK steps and each block is added into fp64
// registers; discrete symbol counts go to an LDS table of 64-bit integers in units of 2^-31
// (integer atomics: the sum does not depend on the order of the additions).  Workgroup and grid
// reductions are fp64 in a fixed order (the fp64 path's k_finalize), so two calls agree bitwise.
// The chunk boundaries are verified by k_f32_check against the tolerance f32_tol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "estep_kernels.hpp"

namespace bhmm {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// fp32 statistics are added into the fp64 accumulators every so many backward steps
constexpr int F32_BLOCK = 64;
// a step whose largest forward entry (before rescaling) or backward normaliser falls below this
// leaves the range where fp32 products keep their relative accuracy: the call goes back to fp64
constexpr float F32_TINY = 0x1p-100f;
// words[1] flag bits
enum { F32_UNDERFLOW = 1, F32_NONFINITE = 2 };

template <int N>
struct ModelF {
    float A[N * N]; // row-major; padded rows / columns as the fp64 Model (identity on the padding)
    float pi[N];
    double mu[N];   // gaussian: means (o - mu is formed in fp64)
    float gk[N];    // gaussian: log2(e) / (2 sigma^2); padded state: 1
    float gc[N];    // gaussian: log2(1 / (sqrt(2 pi) sigma)); padded state: -inf   (p = 2^(gc - gk d^2))
    int nreal;
    int M;
    int W;          // warm-up length of the speculative chunk boundaries
};

// ---- cross-lane exchanges inside the H-lane group of a chunk (DPP quad permutes) --------
template <int CTRL>
__device__ __forceinline__ float dppf(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// value of lane q ^ K of my group
template <int K>
__device__ __forceinline__ float xorf(float v)
{
    if constexpr (K == 1)
        return dppf<0xB1>(v); // quad_perm [1,0,3,2]
    else if constexpr (K == 2)
        return dppf<0x4E>(v); // quad_perm [2,3,0,1]
    else
        return dppf<0x1B>(v); // quad_perm [3,2,1,0]
}
template <int K>
__device__ __forceinline__ f32x2 xorf2(f32x2 v)
{
    return f32x2{xorf<K>(v.x), xorf<K>(v.y)};
}
// (commutative pairwise steps: every lane of the group ends with the same bits)
template <int H>
__device__ __forceinline__ float gsumf(float x)
{
    if constexpr (H >= 2)
        x += xorf<1>(x);
    if constexpr (H >= 4)
        x += xorf<2>(x);
    return x;
}
template <int H>
__device__ __forceinline__ float gmaxf(float x)
{
    if constexpr (H >= 2)
        x = fmaxf(x, xorf<1>(x));
    if constexpr (H >= 4)
        x = fmaxf(x, xorf<2>(x));
    return x;
}
// g[k] = the pair of lane q ^ k
template <int H>
__device__ __forceinline__ void gather2(f32x2 own, f32x2 (&g)[H])
{
    g[0] = own;
    if constexpr (H >= 2)
        g[1] = xorf2<1>(own);
    if constexpr (H >= 4) {
        g[2] = xorf2<2>(own);
        g[3] = xorf2<3>(own);
    }
}

__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 splat(float x) { return f32x2{x, x}; }

// Per-lane constants of one chunk lane: the model's entries that lane q multiplies with.
template <int N, int KIND>
struct LaneF {
    static constexpr int H = N / 2;
    f32x2 Af[H][2]; // forward:  Af[k][b]  = A[2(q^k)+b][2q .. 2q+1]
    f32x2 Ab[H][2]; // backward: Ab[k][jj] = A[2q .. 2q+1][2(q^k)+jj]
    f32x2 pi, ones;
    double mu0, mu1;
    f32x2 gk, gc;
    __device__ __forceinline__ void load(const ModelF<N> &m, int q)
    {
#pragma unroll
        for (int k = 0; k < H; ++k) {
            const int r = 2 * (q ^ k);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                Af[k][b] = f32x2{m.A[(r + b) * N + 2 * q], m.A[(r + b) * N + 2 * q + 1]};
                Ab[k][b] = f32x2{m.A[(2 * q) * N + r + b], m.A[(2 * q + 1) * N + r + b]};
            }
        }
        pi = f32x2{m.pi[2 * q], m.pi[2 * q + 1]};
        ones = f32x2{2 * q < m.nreal ? 1.f : 0.f, 2 * q + 1 < m.nreal ? 1.f : 0.f};
        if constexpr (KIND == EMIT_GAUSS) {
            mu0 = m.mu[2 * q];
            mu1 = m.mu[2 * q + 1];
            gk = f32x2{m.gk[2 * q], m.gk[2 * q + 1]};
            gc = f32x2{m.gc[2 * q], m.gc[2 * q + 1]};
        }
    }
    // emission probabilities of my two states for observation o (gaussian) / symbol sym (discrete);
    // d = o - mu in fp32 (formed in fp64)
    __device__ __forceinline__ f32x2 emit(double o, int sym, const float *Bt, int q, f32x2 &d) const
    {
        if constexpr (KIND == EMIT_GAUSS) {
            d = f32x2{(float)(o - mu0), (float)(o - mu1)};
            const f32x2 x = fma2(-gk, d * d, gc);
            return f32x2{__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)};
        } else {
            return *reinterpret_cast<const f32x2 *>(Bt + sym * N + 2 * q);
        }
    }
    // (alpha A) restricted to my states
    __device__ __forceinline__ f32x2 fwd(f32x2 a) const
    {
        f32x2 g[H];
        gather2<H>(a, g);
        f32x2 nx = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < H; ++k) {
            nx = fma2(splat(g[k].x), Af[k][0], nx);
            nx = fma2(splat(g[k].y), Af[k][1], nx);
        }
        return nx;
    }
    // A w restricted to my states; g receives w of the whole group
    __device__ __forceinline__ f32x2 bwd(f32x2 w, f32x2 (&g)[H]) const
    {
        gather2<H>(w, g);
        f32x2 u = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < H; ++k) {
            u = fma2(Ab[k][0], splat(g[k].x), u);
            u = fma2(Ab[k][1], splat(g[k].y), u);
        }
        return u;
    }
};

// exact power-of-two rescaling: the group's largest entry into [0.5, 1); returns the exponent removed
template <int H>
__device__ __forceinline__ int rescale(f32x2 &v, float &vmin)
{
    const float mx = gmaxf<H>(fmaxf(v.x, v.y));
    vmin = fminf(vmin, mx);
    const int e = __builtin_amdgcn_frexp_expf(mx);
    v = f32x2{__builtin_amdgcn_ldexpf(v.x, -e), __builtin_amdgcn_ldexpf(v.y, -e)};
    return e;
}

template <int KIND>
__device__ __forceinline__ void obs_at(const void *base, int64_t idx, double &o, int &sym)
{
    if constexpr (KIND == EMIT_GAUSS)
        o = static_cast<const double *>(base)[idx];
    else
        sym = static_cast<const int32_t *>(base)[idx];
}

// dynamic LDS of k_estep_f32: [NW][S] fp64 reduction rows | (discrete) B^T [M][N] fp32 | counts [M][N] u64
template <int N, int KIND>
__host__ __device__ constexpr size_t f32_smem_bytes(int M)
{
    return (size_t)((N / 2 * 64 + 63) / 64) * StatLayout<N, KIND>::S * 8 +
           (KIND == EMIT_DISC ? (size_t)M * N * 12 : 0);
}

// One workgroup per CI record group (64 chunks), 32 N threads.
template <int N, int KIND>
__global__ __launch_bounds__(32 * N) void k_estep_f32(
    const ModelF<N> m, const Chunks ch, const void *obs_ci, const void *obs_rm,
    const int64_t *toff,     // [K+1] trajectory offsets (time steps)
    const float *Bt_g,       // discrete: [M][N] B^T in fp32
    float *ws,               // CI workspace: alpha rows (fp32, [record][64][N])
    float *bvec,             // [4][Gp][N]: a_entry, a_exit, b_exit, b_entry of every chunk (any scale)
    int Gp,
    double *logL_chunk,      // [Gp]
    double *gamma0,          // [K][N] gamma at t = 0 of every trajectory
    double *partials,        // [gridDim.x][S] register statistics per workgroup
    double *disc_partials,   // [gridDim.x][M N] discrete symbol counts per workgroup
    unsigned int *flags)     // |= F32_* flags
{
    using SL = StatLayout<N, KIND>;
    constexpr int H = N / 2;
    constexpr int NW = (64 * H + 63) / 64;
    constexpr int SS = SL::S;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double *red = smem;                                                    // [NW][SS]
    float *Bt = reinterpret_cast<float *>(smem + NW * SS);                 // [M][N]
    unsigned long long *cnt =
        reinterpret_cast<unsigned long long *>(Bt + (KIND == EMIT_DISC ? m.M * N : 0)); // [M][N]
    if constexpr (KIND == EMIT_DISC) {
        for (int i = threadIdx.x; i < m.M * N; i += blockDim.x) {
            Bt[i] = Bt_g[i];
            cnt[i] = 0ull;
        }
        __syncthreads();
    }
    const int cl = threadIdx.x / H;
    const int q = threadIdx.x % H;
    const int64_t g = (int64_t)blockIdx.x * 64 + cl;
    const int len = ch.len[g];
    LaneF<N, KIND> lf;
    lf.load(m, q);

    f32x2 Xf[H][2], Gf = {0.f, 0.f}, E1f = {0.f, 0.f}, E2f = {0.f, 0.f};
    double Xd[H][2][2], Gd[2] = {0.0, 0.0}, E1d[2] = {0.0, 0.0}, E2d[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < H; ++k)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            Xf[k][jj] = f32x2{0.f, 0.f};
            Xd[k][jj][0] = Xd[k][jj][1] = 0.0;
        }
    auto flush = [&]() {
#pragma unroll
        for (int k = 0; k < H; ++k)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                Xd[k][jj][0] += (double)Xf[k][jj].x;
                Xd[k][jj][1] += (double)Xf[k][jj].y;
                Xf[k][jj] = f32x2{0.f, 0.f};
            }
        Gd[0] += (double)Gf.x;
        Gd[1] += (double)Gf.y;
        Gf = f32x2{0.f, 0.f};
        if constexpr (KIND == EMIT_GAUSS) {
            E1d[0] += (double)E1f.x;
            E1d[1] += (double)E1f.y;
            E2d[0] += (double)E2f.x;
            E2d[1] += (double)E2f.y;
            E1f = E2f = f32x2{0.f, 0.f};
        }
    };

    if (len > 0) {
        const int64_t t0 = ch.t0[g];
        const int64_t goff = ch.goff[g];
        const int traj = ch.traj[g];
        const int64_t T = toff[traj + 1] - toff[traj];
        const int64_t tend = t0 + len - 1;
        const bool first = t0 == 0;
        const bool last = tend == T - 1;
        const int64_t rbase = (int64_t)blockIdx.x * ch.Lmax; // CI record of local step 0
        const double *ocd = static_cast<const double *>(obs_ci);
        const int32_t *oci = static_cast<const int32_t *>(obs_ci);
        auto ci_obs = [&](int s, double &o, int &sym) {
            const int64_t idx = (rbase + s) * 64 + cl;
            if constexpr (KIND == EMIT_GAUSS)
                o = ocd[idx];
            else
                sym = oci[idx];
        };
        f32x2 *wsp = reinterpret_cast<f32x2 *>(ws);
        auto ws_idx = [&](int s) { return ((rbase + s) * 64 + cl) * H + q; };
        f32x2 *bv = reinterpret_cast<f32x2 *>(bvec);
        const int64_t bstride = (int64_t)Gp * H;
        float vmin = 1.f;
        f32x2 d;
        double o = 0.0;
        int sym = 0;

        // ---- forward warm-up -> alpha one step before the chunk ----
        f32x2 aent = lf.ones;
        if (!first) {
            int64_t s0 = t0 - m.W;
            if (s0 <= 0) {
                s0 = 0;
                obs_at<KIND>(obs_rm, goff - t0, o, sym);
                aent = lf.pi * lf.emit(o, sym, Bt, q, d);
            } else {
                obs_at<KIND>(obs_rm, goff - t0 + s0, o, sym);
                aent = lf.ones * lf.emit(o, sym, Bt, q, d);
            }
            (void)rescale<H>(aent, vmin);
            for (int64_t t = s0 + 1; t < t0; ++t) {
                obs_at<KIND>(obs_rm, goff - t0 + t, o, sym);
                aent = lf.fwd(aent) * lf.emit(o, sym, Bt, q, d);
                (void)rescale<H>(aent, vmin);
            }
            bv[0 * bstride + g * H + q] = aent;
        }

        // ---- forward sweep ----
        int esum = 0;
        f32x2 a = aent;
        {
            double on = 0.0;
            int sn = 0;
            int s = 0;
            if (first) { // alpha_0 = pi o p_0
                ci_obs(0, o, sym);
                a = lf.pi * lf.emit(o, sym, Bt, q, d);
                esum += rescale<H>(a, vmin);
                wsp[ws_idx(0)] = a;
                s = 1;
            }
            if (s < len)
                ci_obs(s, on, sn);
            for (; s < len; ++s) {
                o = on;
                sym = sn;
                if (s + 1 < len)
                    ci_obs(s + 1, on, sn);
                a = lf.fwd(a) * lf.emit(o, sym, Bt, q, d);
                esum += rescale<H>(a, vmin);
                wsp[ws_idx(s)] = a;
            }
        }
        if (!last)
            bv[1 * bstride + g * H + q] = a;
        {
            const float sa = gsumf<H>(a.x + a.y);
            const float se = gsumf<H>(aent.x + aent.y);
            if (q == 0)
                logL_chunk[g] = (double)esum * 0.69314718055994530942 + log((double)sa) -
                                (first ? 0.0 : log((double)se));
        }

        // ---- backward warm-up -> beta at the chunk's last step ----
        f32x2 b = lf.ones;
        if (!last) {
            int64_t top = tend + m.W;
            if (top > T - 1)
                top = T - 1;
            f32x2 gw[H];
            for (int64_t t = top; t > tend; --t) {
                obs_at<KIND>(obs_rm, goff - t0 + t, o, sym);
                b = lf.bwd(lf.emit(o, sym, Bt, q, d) * b, gw);
                (void)rescale<H>(b, vmin);
            }
            bv[2 * bstride + g * H + q] = b;
        }

        // ---- backward sweep: statistics ----
        float zmin = 1.f;
        {
            const float z = gsumf<H>(a.x * b.x + a.y * b.y);
            zmin = fminf(zmin, z);
            b = b * splat(__builtin_amdgcn_rcpf(z));
        }
        double on = 0.0;
        int sn = 0;
        ci_obs(len - 1, on, sn);
        f32x2 an = len > 1 ? wsp[ws_idx(len - 2)] : aent;
        int blk = 0;
        for (int s = len - 1; s >= 0; --s) {
            o = on;
            sym = sn;
            const f32x2 ap = an; // alpha one step before s
            if (s > 0) {
                ci_obs(s - 1, on, sn);
                an = s > 1 ? wsp[ws_idx(s - 2)] : aent;
            }
            const f32x2 p = lf.emit(o, sym, Bt, q, d);
            const f32x2 gm = a * b;
            Gf += gm;
            if constexpr (KIND == EMIT_GAUSS) {
                const f32x2 gd = gm * d;
                E1f += gd;
                E2f = fma2(gd, d, E2f);
            } else {
                const unsigned int c0 = (unsigned int)__builtin_fmaf(gm.x, 0x1p31f, 0.5f);
                const unsigned int c1 = (unsigned int)__builtin_fmaf(gm.y, 0x1p31f, 0.5f);
                atomicAdd(&cnt[sym * N + 2 * q], (unsigned long long)c0);
                atomicAdd(&cnt[sym * N + 2 * q + 1], (unsigned long long)c1);
            }
            if (s == 0 && first) {
                gamma0[(int64_t)traj * N + 2 * q] = (double)gm.x;
                gamma0[(int64_t)traj * N + 2 * q + 1] = (double)gm.y;
                break;
            }
            f32x2 gw[H];
            const f32x2 u = lf.bwd(p * b, gw);
            const float z = gsumf<H>(ap.x * u.x + ap.y * u.y);
            zmin = fminf(zmin, z);
            const float r = __builtin_amdgcn_rcpf(z);
            const f32x2 v = ap * splat(r);
#pragma unroll
            for (int k = 0; k < H; ++k) {
                Xf[k][0] = fma2(v, splat(gw[k].x), Xf[k][0]);
                Xf[k][1] = fma2(v, splat(gw[k].y), Xf[k][1]);
            }
            b = u * splat(r);
            a = ap;
            if (++blk == F32_BLOCK) {
                blk = 0;
                flush();
            }
        }
        if (!first)
            bv[3 * bstride + g * H + q] = b; // beta one step before the chunk, as this chunk derived it
        flush();
        if (!(vmin >= F32_TINY) || !(zmin >= F32_TINY))
            atomicOr(flags, (unsigned int)F32_UNDERFLOW);
    }

    // ---- workgroup reduction (fixed order) ----
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    auto wred = [&](double x) {
#pragma unroll
        for (int h = H; h < 64; h <<= 1)
            x += __shfl_xor(x, h, 64);
        return x;
    };
#pragma unroll
    for (int k = 0; k < H; ++k)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const double x = wred(Xd[k][jj][bb]);
                if (lane < H)
                    red[wv * SS + (2 * q + bb) * N + 2 * (q ^ k) + jj] = x;
            }
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        const double x = wred(Gd[bb]);
        if (lane < H)
            red[wv * SS + SL::NC + 2 * q + bb] = x;
        if constexpr (KIND == EMIT_GAUSS) {
            const double x1 = wred(E1d[bb]);
            const double x2 = wred(E2d[bb]);
            if (lane < H) {
                red[wv * SS + SL::NC + N + 2 * q + bb] = x1;
                red[wv * SS + SL::NC + 2 * N + 2 * q + bb] = x2;
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SS; e += blockDim.x) {
        double s = red[e];
        for (int w = 1; w < NW; ++w)
            s += red[w * SS + e];
        partials[(int64_t)blockIdx.x * SS + e] = s;
    }
    if constexpr (KIND == EMIT_DISC) {
        for (int i = threadIdx.x; i < m.M * N; i += blockDim.x)
            disc_partials[(int64_t)blockIdx.x * m.M * N + i] = (double)cnt[i] * 0x1p-31;
    }
}

// largest componentwise relative deviation of two boundary vectors, each taken up to its scale
template <int N>
__device__ __forceinline__ float f32_vdev(const float *x, const float *y)
{
    float mx = 0.f, my = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        mx = fmaxf(mx, x[i]);
        my = fmaxf(my, y[i]);
    }
    const float sx = 1.f / mx, sy = 1.f / my;
    float dev = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float a = x[i] * sx, b = y[i] * sy;
        const float dv = fabsf(a - b) / fmaxf(fmaxf(a, b), 1e-20f);
        dev = (dv <= dev) ? dev : dv; // (NaN sticks)
    }
    return dev;
}

// Boundary check: alpha at each chunk's last step against its successor's warm-up, beta one step
// before the successor against this chunk's warm-up.  words[0]: largest deviation (float bits,
// integer maximum: order-independent), words[1] |= F32_NONFINITE for a vector that is not usable.
template <int N>
__global__ __launch_bounds__(256) void k_f32_check(const Chunks ch, int G, int Gp, const float *bvec,
                                                   unsigned int *words)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g + 1 >= G || ch.traj[g] != ch.traj[g + 1] || ch.len[g] <= 0 || ch.len[g + 1] <= 0)
        return;
    const float *aen = bvec, *aex = bvec + (int64_t)Gp * N, *bex = bvec + 2 * (int64_t)Gp * N,
                *ben = bvec + 3 * (int64_t)Gp * N;
    const float da = f32_vdev<N>(aex + (int64_t)g * N, aen + (int64_t)(g + 1) * N);
    const float db = f32_vdev<N>(bex + (int64_t)g * N, ben + (int64_t)(g + 1) * N);
    const float dev = fmaxf(da, db);
    if (!(da <= 3e38f) || !(db <= 3e38f))
        atomicOr(&words[1], (unsigned int)F32_NONFINITE);
    else
        atomicMax(&words[0], __float_as_uint(dev));
}

} // namespace bhmm
