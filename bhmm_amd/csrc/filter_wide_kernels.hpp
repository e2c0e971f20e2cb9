// filter_wide_kernels.hpp -- bhmm_filter for 9..64 states: the time-segmented forward sweep with the filtered row
// and the increment as the last stage of every step (filter_api.hip, filter_path 2).
//
//   k_filter_wide  the layout, warm-up, loads and recursion of k_score_wide<.., LAZY = false>
//                  (score_wide_kernels.hpp, included and not changed) for ONE model: grid (segment groups), one
//                  wavefront per workgroup, one lane per state, 64 / NP segments per wavefront, lane j holds
//                  column j of A in NP registers, the product on DPP row broadcasts (rows_of_group / dot16).  A
//                  segment warms up for W steps from the uniform vector -- or starts exactly from pi when the
//                  trajectory start is closer -- and writes the entry vector it derived, the exit vector it
//                  computed and whether that one is all zero.  The vector is normalised by its sum c every step
//                  (a sum or an emission row in the denormal range times 2^900, the exponent counted in pexp; a
//                  sum of exactly zero: dead from there on).  With the previous vector normalised, c is the
//                  one-step predictive density times 2^pexp, so the last stage of every step of the segment is
//                      row       a_j = nj / c                       (lane j: its own component, one record per
//                                                                    step and segment; or its projection)
//                      increment log c - pexp ln 2                  (lane 0 of the segment)
//                  and zero rows / -inf once dead.  Warm-up steps emit nothing.
//                  Projection (PROJ): column q is sum_i a_i V[i][q] formed by the fixed DPP tree of wgroup_sum
//                  over the lanes' products, in fp64 -- NOT in ascending i (the bound of the tests holds, the
//                  summation order of marg_project does not); lane q < Q stores column q.
//   The boundary check, the first dead segment of every trajectory and the fix-up behind it:
//   k_filter_seg_check, k_filter_first_dead, k_filter_seg_bury (filter_kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marg_kernels.hpp" // MARG_QMAX
#include "score_kernels.hpp"
#include "score_wide_kernels.hpp" // ScoreWideModel
#include "wide_kernels.hpp"

namespace bhmm {

// rows == nullptr: no rows (a uniform branch); WANT_LOGC false: logc is not touched.  rows: [total][PROJ ? Q : n].
// B^T in LDS: M rows of NP doubles (the image of k_score_wide)
template <int NP, int KIND, bool BT_LDS, typename OT, bool PROJ, bool WANT_LOGC>
__global__ __launch_bounds__(64) void k_filter_wide(const ScoreWideModel *__restrict__ mp, int W, const int64_t *off,
                                                    const Segs sg, const void *obs_rm, OT *__restrict__ rows,
                                                    const double *__restrict__ V, int Q, OT *__restrict__ logc,
                                                    double *a_entry, double *a_exit, uint8_t *dead_out)
{
    constexpr int GP = 64 / NP;
    extern __shared__ double sBt[];
    const WideModel m = mp->w;
    const double *Bt = mp->Bt;
    const int lane = threadIdx.x;
    const int gi = lane / NP, j = lane % NP;
    const int n = m.n;
    // the projection in LDS, [q][state] (registers: lane j's row of V would cost the second wavefront per SIMD
    // at 64 states)
    __shared__ double sV[PROJ ? MARG_QMAX * NP : 1];
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
    const int64_t o0 = off[sg.traj[s]];
    const int64_t t0 = sg.t0[s], t1 = t0 + sg.len[s];
    if (t1 <= t0) {
        if (j == 0)
            dead_out[s] = 0;
        return;
    }
    const unsigned long long gmask = wgroup_mask<NP>(lane);
    double Acol[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i)
        Acol[i] = (real && i < n) ? m.A[(int64_t)i * n + j] : 0.0;
    const double mu_j = (KIND == EMIT_GAUSS && real) ? m.mu[j] : 0.0;
    const double ga_j = (KIND == EMIT_GAUSS && real) ? m.ga[j] : 0.0;
    const double gb_j = (KIND == EMIT_GAUSS && real) ? m.gb[j] : 1.0;
    const double pi_j = real ? m.pi[j] : 0.0;

    const int64_t tw = t0 > W ? t0 - W : 0; // warm-up start (0: exact start from pi)
    const int nsteps = (int)(t1 - tw), r0 = (int)(t0 - tw);
    const bool from_start = tw == 0;
    auto obs_of = [&](int r) { return wide_load<KIND>(m, j, real, o0 + tw + (r < nsteps ? r : nsteps - 1), obs_rm); };
    // emission of my state; discrete rows too large for LDS are fetched WIDE_PF / 2 steps ahead of their use
    constexpr bool BT_RING = KIND == EMIT_DISC && !BT_LDS;
    auto bt_of = [&](const WideIn &in) { return real ? Bt[(int64_t)in.sym * n + j] : 0.0; };
    WideIn ring[WIDE_PF];
    double pring[BT_RING ? WIDE_PF : 1];
#pragma unroll
    for (int u = 0; u < WIDE_PF; ++u)
        ring[u] = obs_of(u);
    if constexpr (BT_RING)
#pragma unroll
        for (int u = 0; u < WIDE_PF / 2; ++u)
            pring[u] = bt_of(ring[u]);

    constexpr double LN2 = 0.693147180559945309417232121458;
    double a = real ? 1.0 / (double)n : 0.0;
    bool dead = false; // the sum became exactly zero (group-uniform)
    for (int rb = 0; rb < nsteps; rb += WIDE_PF) {
#pragma unroll
        for (int u = 0; u < WIDE_PF; ++u) {
            const int r = rb + u;
            if (r >= nsteps)
                break;
            const WideIn in = ring[u];
            double p;
            int pexp = 0;
            if constexpr (KIND == EMIT_DISC) {
                if constexpr (BT_LDS) {
                    p = sBt[in.sym * NP + j];
                } else {
                    p = pring[u];
                    pring[(u + WIDE_PF / 2) % WIDE_PF] = bt_of(ring[(u + WIDE_PF / 2) % WIDE_PF]);
                }
                // (the rule of wide_emit<.., RESCUE>: a row in the denormal range times 2^900)
                if ((__ballot(p >= 0x1p-959) & gmask) == 0ull && (__ballot(p != 0.0) & gmask) != 0ull) {
                    p = ldexp(p, 900);
                    pexp = 900;
                }
            } else {
                p = wide_emit<NP, KIND, true>(m, j, real, in, mu_j, ga_j, gb_j, gmask, &pexp);
                // a NaN observation is an outlier here, a row of ones (k_filter_serial; section 16).  wide_emit
                // hands the NaN on, as the E-step wants it; the observation is the same in every lane of the group
                if (__builtin_expect(in.o != in.o, 0)) {
                    p = real ? 1.0 : 0.0;
                    pexp = 0;
                }
            }
            ring[u] = obs_of(r + WIDE_PF);
            double nj;
            if (from_start && r == 0) {
                nj = pi_j * p;
            } else {
                double acc[4] = {0.0, 0.0, 0.0, 0.0};
                const Rows4 ar = rows_of_group<NP>(a);
                unrolled<NP / 16>([&](auto rc) {
                    constexpr int q = decltype(rc)::value;
                    dot16(acc, ar.r[q], [&](auto ic) -> const double & { return Acol[16 * q + decltype(ic)::value]; });
                });
                nj = ((acc[0] + acc[1]) + (acc[2] + acc[3])) * p;
            }
            double c = wgroup_sum<NP>(nj);
            if (__builtin_expect(!(c >= 0x1p-959), 0)) {
                if (c > 0.0) { // a sum in the denormal range: times 2^900, exactly (k_score_wide)
                    nj = ldexp(nj, 900);
                    c = wgroup_sum<NP>(nj);
                    pexp += 900;
                } else {
                    dead = true; // probability zero from here on (a warm-up's support contains the true one)
                }
            }
            a = dead ? 0.0 : nj * fast_rcp(c);
            if (r >= r0) {
                // ---- last stage: the row (or its projection) and the increment of step tw + r ----
                const int64_t g = o0 + tw + r;
                if (rows) {
                    if constexpr (PROJ) {
                        double mine = 0.0;
#pragma unroll
                        for (int q = 0; q < MARG_QMAX; ++q)
                            if (q < Q) { // (uniform)
                                const double sq = wgroup_sum<NP>(a * sV[q * NP + j]);
                                mine = j == q ? sq : mine;
                            }
                        if (j < Q)
                            rows[g * Q + j] = (OT)mine;
                    } else {
                        if (real)
                            rows[g * n + j] = (OT)a;
                    }
                }
                if constexpr (WANT_LOGC) {
                    const double lc = dead ? -INFINITY : log(c) - (double)pexp * LN2;
                    if (j == 0)
                        logc[g] = (OT)lc;
                }
            } else if (r == r0 - 1 && real) {
                a_entry[(int64_t)s * n + j] = a;
            }
        }
    }
    if (real)
        a_exit[(int64_t)s * n + j] = a;
    if (j == 0)
        dead_out[s] = dead ? 1 : 0; // the exit vector is all zero
}

} // namespace bhmm
