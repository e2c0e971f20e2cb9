// smooth_wide_kernels.hpp -- bhmm_posterior_decode / bhmm_posterior_marginals for 9..64 states: the backward half of
// the time-segmented smoothing pass (smooth_wide.hip, post_path / marg_path 2).  The forward
// half is k_filter_wide (filter_wide_kernels.hpp, not changed), which leaves the normalised filtered row of every
// step of every segment in a workspace.
//
//   k_smooth_wide_bwd  the layout of k_filter_wide: grid (segment groups), one wavefront per workgroup, one lane per
//                  state, 64 / NP segments per wavefront.  Lane i holds ROW i of A in NP registers; the vector to
//                  multiply is v_j = p_{t+1}(j) b_{t+1}(j), one component per lane, and b_t(i) = sum_j A[i][j] v_j is
//                  formed by the DPP row broadcasts of the forward product (rows_of_group / dot16): no LDS exchange.
//                  A segment [t0, t1) of a trajectory of T steps starts at step min(T - 1, t1 - 1 + W) from the
//                  all-ones vector -- exact when that is T - 1, else the warm-up of section 14 -- and walks down to
//                  t0, and one step further when t0 > 0.  Emissions by k_filter_wide's rule (wide_emit<.., true>; a
//                  discrete row in the denormal range times 2^900), so both halves see the same p; b is normalised
//                  by its group sum every step (a sum in the denormal range: times 2^900); its exponent is never
//                  needed, nothing is counted.  Warm-up steps read no alpha row and emit nothing.  Inside the
//                  segment lane j forms g_j = a_t(j) b_t(j) and S = sum_j g_j (0 < S < 2^-959: times 2^900); the last
//                  stage is a template parameter:
//                      SMOOTH_DECODE  the lowest lane of the group with g == max g (the tie rule of
//                                     k_post_gamma_rm) and, with conf, (float)(max g / S); one lane per segment
//                                     stores, eight steps to one 64-bit store where the global index is aligned
//                                     and single bytes at a segment's ragged ends (k_post_sweep)
//                      SMOOTH_ROWS    lane j < n stores g_j / S (one reciprocal per step)
//                      SMOOTH_PROJ    column q is sum_j (g_j / S) V[j][q] formed by the fixed DPP tree of
//                                     wgroup_sum -- NOT in ascending j, as k_filter_wide's projection; lane q stores
//                  The segment writes the normalised b it assumed for step t1 - 1 (b_exit) and the one it computed
//                  for step t0 - 1 (b_entry; that step needs no alpha): k_wide_check compares them.  A NaN
//                  observation, or a b sum or S that is zero or not finite, sets the segment's trouble byte (the
//                  host then takes the generic path); the kernel never loops or faults on such input.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marg_kernels.hpp" // MARG_QMAX
#include "score_kernels.hpp"
#include "score_wide_kernels.hpp" // ScoreWideModel
#include "wide_kernels.hpp"

namespace bhmm {

enum { SMOOTH_DECODE = 0, SMOOTH_ROWS = 1, SMOOTH_PROJ = 2 };

// largest element of a group of NP lanes, in every lane of it (the butterfly of wgroup_sum)
template <int NP>
__device__ __forceinline__ double wgroup_fmax(double v)
{
    v = fmax(v, xchg_f64<1>(v));
    v = fmax(v, xchg_f64<2>(v));
    v = fmax(v, xchg_f64<4>(v));
    {
        const int lo = dpp_i32<0x140>(__double2loint(v)); // row_mirror: i <-> 15 - i
        const int hi = dpp_i32<0x140>(__double2hiint(v));
        v = fmax(v, __hiloint2double(hi, lo));
    }
    if constexpr (NP == 64) { // across the rows as wave64_sum does it
        double x = v, y = v;
        swap32_f64(x, y); // rows (0,1,0,1) / (2,3,2,3)
        x = fmax(x, y);
        y = x;
        swap16_f64(x, y); // all rows: 0+2 / 1+3
        return fmax(x, y);
    }
    if constexpr (NP >= 32)
        v = fmax(v, __shfl_xor(v, 16, 64));
    return v;
}

// ws: the filtered rows of the launch's segments, global step g at ws[(g - g_first) * n].  out: the paths (OT =
// uint8_t / int32_t, [total]) or the rows (OT = double / float, [total][STAGE == SMOOTH_PROJ ? Q : n]); conf: [total]
// or nullptr (a uniform branch; SMOOTH_DECODE only).  B^T in LDS: M rows of NP doubles (the image of k_filter_wide)
template <int NP, int KIND, bool BT_LDS, int STAGE, typename OT>
__global__ __launch_bounds__(64) void k_smooth_wide_bwd(const ScoreWideModel *__restrict__ mp, int W, const int64_t *off,
                                                        const Segs sg, const void *obs_rm,
                                                        const double *__restrict__ ws, int64_t g_first,
                                                        OT *__restrict__ out, float *__restrict__ conf,
                                                        const double *__restrict__ V, int Q, double *b_exit,
                                                        double *b_entry, uint8_t *trouble_out)
{
    constexpr int GP = 64 / NP;
    constexpr bool PROJ = STAGE == SMOOTH_PROJ;
    extern __shared__ double sBt[];
    const WideModel m = mp->w;
    const double *Bt = mp->Bt;
    const int lane = threadIdx.x;
    const int gi = lane / NP, j = lane % NP;
    const int n = m.n;
    __shared__ double sV[PROJ ? MARG_QMAX * NP : 1]; // the projection, [q][state]
    if constexpr (PROJ)
        for (int e = lane; e < MARG_QMAX * NP; e += 64)
            sV[e] = (e % NP < n && e / NP < Q) ? V[(e % NP) * Q + e / NP] : 0.0;
    if constexpr (KIND == EMIT_DISC && BT_LDS)
        for (int e = lane; e < m.M * NP; e += 64)
            sBt[e] = e % NP < n ? Bt[(int64_t)(e / NP) * n + e % NP] : 0.0;
    if constexpr (PROJ || (KIND == EMIT_DISC && BT_LDS))
        __syncthreads();
    const int s = (int)blockIdx.x * GP + gi;
    if (s >= sg.nseg)
        return;
    const bool real = j < n;
    const int k = sg.traj[s];
    const int64_t o0 = off[k], T = off[k + 1] - o0;
    const int64_t t0 = sg.t0[s], t1 = t0 + sg.len[s];
    if (t1 <= t0) {
        if (j == 0)
            trouble_out[s] = 0;
        return;
    }
    const unsigned long long gmask = wgroup_mask<NP>(lane);
    double Arow[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c)
        Arow[c] = (real && c < n) ? m.A[(int64_t)j * n + c] : 0.0;
    const double mu_j = (KIND == EMIT_GAUSS && real) ? m.mu[j] : 0.0;
    const double ga_j = (KIND == EMIT_GAUSS && real) ? m.ga[j] : 0.0;
    const double gb_j = (KIND == EMIT_GAUSS && real) ? m.gb[j] : 1.0;

    // step r of the loop is t = te - r: the stage of step t (inside the segment), then the recursion to t - 1
    const int64_t te = t1 - 1 + W < T - 1 ? t1 - 1 + W : T - 1; // warm-up start (T - 1: exact)
    const int nsteps = (int)(te - t0) + 1, r_in = (int)(te - (t1 - 1));
    const bool to_start = t0 == 0; // (the last step has no recursion)
    auto obs_of = [&](int r) { return wide_load<KIND>(m, j, real, o0 + te - (r < nsteps ? r : nsteps - 1), obs_rm); };
    // alpha row of my state, WIDE_PF steps ahead like the observation (warm-up steps: the segment's last row, not used)
    auto alpha_of = [&](int r) {
        const int64_t t = te - (r < nsteps ? r : nsteps - 1);
        return real ? ws[(o0 + (t < t1 ? t : t1 - 1) - g_first) * n + j] : 0.0;
    };
    // emission of my state; discrete rows too large for LDS are fetched WIDE_PF / 2 steps ahead of their use
    constexpr bool BT_RING = KIND == EMIT_DISC && !BT_LDS;
    auto bt_of = [&](const WideIn &in) { return real ? Bt[(int64_t)in.sym * n + j] : 0.0; };
    WideIn ring[WIDE_PF];
    double aring[WIDE_PF];
    double pring[BT_RING ? WIDE_PF : 1];
#pragma unroll
    for (int u = 0; u < WIDE_PF; ++u) {
        ring[u] = obs_of(u);
        aring[u] = alpha_of(u);
    }
    if constexpr (BT_RING)
#pragma unroll
        for (int u = 0; u < WIDE_PF / 2; ++u)
            pring[u] = bt_of(ring[u]);

    double b = real ? 1.0 : 0.0;
    bool trouble = false; // (group-uniform)
    uint64_t acc8 = 0;    // SMOOTH_DECODE, one byte per step: up to 8 consecutive steps, lowest address in the low byte
    int cnt8 = 0;
    for (int rb = 0; rb < nsteps; rb += WIDE_PF) {
#pragma unroll
        for (int u = 0; u < WIDE_PF; ++u) {
            const int r = rb + u;
            if (r >= nsteps)
                break;
            const WideIn in = ring[u];
            const double al = aring[u];
            double p;
            if constexpr (KIND == EMIT_DISC) {
                if constexpr (BT_LDS) {
                    p = sBt[in.sym * NP + j];
                } else {
                    p = pring[u];
                    pring[(u + WIDE_PF / 2) % WIDE_PF] = bt_of(ring[(u + WIDE_PF / 2) % WIDE_PF]);
                }
                // (the rule of wide_emit<.., RESCUE>: a row in the denormal range times 2^900)
                if ((__ballot(p >= 0x1p-959) & gmask) == 0ull && (__ballot(p != 0.0) & gmask) != 0ull)
                    p = ldexp(p, 900);
            } else {
                p = wide_emit<NP, KIND, true>(m, j, real, in, mu_j, ga_j, gb_j, gmask);
                trouble |= in.o != in.o; // (the observation is the same in every lane of the group)
            }
            ring[u] = obs_of(r + WIDE_PF);
            aring[u] = alpha_of(r + WIDE_PF);
            if (r >= r_in) {
                // ---- the stage of step t = te - r ----
                if (r == r_in && real)
                    b_exit[(int64_t)s * n + j] = b; // the vector this segment assumed for step t1 - 1
                const int64_t g = o0 + te - r;
                double gq = al * b, S = wgroup_sum<NP>(gq);
                if (__builtin_expect(!(S >= 0x1p-959 && S <= 0x1.fffffffffffffp+1023), 0)) {
                    if (S > 0.0 && S < 0x1p-959) { // a sum in the denormal range: times 2^900, exactly
                        gq = ldexp(gq, 900);
                        S = wgroup_sum<NP>(gq);
                    } else {
                        trouble = true;
                    }
                }
                if constexpr (STAGE == SMOOTH_DECODE) {
                    const double mx = wgroup_fmax<NP>(gq);
                    const unsigned long long hit = __ballot(gq == mx) & gmask;
                    const int arg = hit ? (__ffsll((long long)hit) - 1) - gi * NP : 0; // the lowest lane wins
                    if (conf) {
                        const float cf = (float)(mx * fast_rcp(S));
                        if (j == 0)
                            conf[g] = cf;
                    }
                    if constexpr (sizeof(OT) == 1) {
                        acc8 = (acc8 << 8) | (uint64_t)arg;
                        ++cnt8;
                        if ((g & 7) == 0 || r == nsteps - 1) {
                            if (j == 0) {
                                if (cnt8 == 8) { // (then g is a multiple of 8: a run is cut at every one)
                                    *reinterpret_cast<uint64_t *>(out + g) = acc8;
                                } else {
                                    for (int q = 0; q < cnt8; ++q)
                                        out[g + q] = (OT)((acc8 >> (8 * q)) & 0xff);
                                }
                            }
                            acc8 = 0;
                            cnt8 = 0;
                        }
                    } else {
                        if (j == 0)
                            out[g] = (OT)arg;
                    }
                } else if constexpr (STAGE == SMOOTH_ROWS) {
                    const double rS = fast_rcp(S);
                    if (real)
                        out[g * n + j] = (OT)(gq * rS);
                } else {
                    const double gam = gq * fast_rcp(S);
                    double mine = 0.0;
#pragma unroll
                    for (int q = 0; q < MARG_QMAX; ++q)
                        if (q < Q) { // (uniform)
                            const double sq = wgroup_sum<NP>(gam * sV[q * NP + j]);
                            mine = j == q ? sq : mine;
                        }
                    if (j < Q)
                        out[g * Q + j] = (OT)mine;
                }
            }
            if (!(to_start && r == nsteps - 1)) {
                // ---- b of step t - 1 ----
                double acc[4] = {0.0, 0.0, 0.0, 0.0};
                const Rows4 vr = rows_of_group<NP>(p * b);
                unrolled<NP / 16>([&](auto rc) {
                    constexpr int q = decltype(rc)::value;
                    dot16(acc, vr.r[q], [&](auto ic) -> const double & { return Arow[16 * q + decltype(ic)::value]; });
                });
                double nb = (acc[0] + acc[1]) + (acc[2] + acc[3]);
                double c = wgroup_sum<NP>(nb);
                if (__builtin_expect(!(c >= 0x1p-959 && c <= 0x1.fffffffffffffp+1023), 0)) {
                    if (c > 0.0 && c < 0x1p-959) { // a sum in the denormal range: times 2^900, exactly (k_filter_wide)
                        nb = ldexp(nb, 900);
                        c = wgroup_sum<NP>(nb);
                    } else {
                        trouble = true;
                    }
                }
                b = trouble ? 0.0 : nb * fast_rcp(c);
            }
        }
    }
    if (!to_start && real)
        b_entry[(int64_t)s * n + j] = b; // b of step t0 - 1, as derived here
    if (j == 0)
        trouble_out[s] = trouble ? 1 : 0;
}

// segments with a flag set (dead: the forward sum became exactly zero; trouble: see above)
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_smooth_flags(const uint8_t *dead, const uint8_t *trouble,
                                                                              int nseg, unsigned int *count)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nseg && (dead[s] | trouble[s]))
        atomicAdd(count, 1u);
}

} // namespace bhmm
