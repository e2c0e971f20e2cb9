// score_wide_kernels.hpp -- bhmm_score for 9..64 states: the forward-only, time-segmented pass (score_api.hip).
// The lane layout and the cross-lane helpers are those of the E-step's k_wide_fwd (wide_kernels.hpp, included
// and not changed); nothing of the E-step's state is read or written.
//
//   k_score_wide   grid (segment groups, models of the batch), one wavefront per workgroup, ONE model per
//                  workgroup (blockIdx.y: its table entry is uniform).  One lane per state, 64 / NP segments
//                  per wavefront, lane j holds column j of A in NP registers, the matrix-vector product on
//                  DPP row broadcasts (rows_of_group / dot16).  A segment warms up for W[model] steps from the
//                  uniform vector -- or starts exactly from pi when the trajectory start is closer -- and
//                  writes per (model, segment) its log-normaliser, the entry vector it derived and the exit
//                  vector it computed.  No alpha rows.
//                  LAZY: the vector is carried up to a power of two that is refreshed every fourth step
//                  (k_wide_fwd<.., LAZY>); a vector that leaves the range between two refreshes -- an all-zero
//                  one and one that overflows included -- counts as a failure of the model (fails[model]),
//                  never as a number.  The refresh looks at the steps before it; the one to three steps between
//                  the last refresh and the segment's end (all of a segment of one to three steps) are held to
//                  the same bound after the loop: an exit sum, or an entry sum, below 2^-900 (WIDE_RANGE_MIN) is
//                  such a failure too -- a sum in the denormal range holds only a few bits.
//                  Otherwise: normalised by its sum every step, a sum in the denormal range is rescued by
//                  2^900, and a sum that is exactly zero makes the segment's log-normaliser -inf.
//   k_score_wide_check  the forward half of k_wide_check per model: every derived entry vector against the
//                  predecessor's exit vector, componentwise relative after normalisation; one failure
//                  counter per model.  Boundaries next to a -inf segment are not checked (score_kernels.hpp).
//   The per (model, trajectory) sum of the segment terms is k_score_logl over the plan's traj0 table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "score_kernels.hpp"
#include "wide_kernels.hpp"

namespace bhmm {

// one entry of the model table in device memory
struct ScoreWideModel {
    WideModel w;      // A, pi, the gaussian constants; B row-major [n][M] (what k_wide_probe reads)
    const double *Bt; // discrete: B transposed, [M][n] -- the NP lanes of a segment read one contiguous row
};

// LDS image of B^T: rows of NP doubles (columns n .. NP-1 zero).  No padding: with 8-byte reads the 64 banks
// are served in two groups of 32 lanes; at NP = 32 a group reads one whole row (all 64 banks once), at
// NP = 64 half a row, so no stride can conflict.  At NP = 16 a group reads two rows of 32 banks each: at the
// 128-byte stride they start at bank 0 or 32 and collide two-way for one pair of symbols in two, any padding
// makes them overlap for nearly every pair.
template <int NP, int KIND, bool LAZY, bool BT_LDS>
__global__ __launch_bounds__(64) void k_score_wide(const ScoreWideModel *__restrict__ models,
                                                   const int32_t *__restrict__ Ws, const int64_t *off,
                                                   const Segs sg, const void *obs_rm, double *logLc,
                                                   double *a_entry, double *a_exit, unsigned int *fails)
{
    constexpr int GP = 64 / NP;
    extern __shared__ double sBt[];
    const int ms = blockIdx.y;
    const WideModel m = models[ms].w;
    const double *Bt = models[ms].Bt;
    const int lane = threadIdx.x;
    const int gi = lane / NP, j = lane % NP;
    const int n = m.n;
    if constexpr (KIND == EMIT_DISC && BT_LDS) {
        for (int e = lane; e < m.M * NP; e += 64)
            sBt[e] = e % NP < n ? Bt[(int64_t)(e / NP) * n + e % NP] : 0.0;
        __syncthreads();
    }
    const int s = (int)blockIdx.x * GP + gi;
    if (s >= sg.nseg)
        return;
    const bool real = j < n;
    const int64_t rec = (int64_t)ms * sg.nseg + s;
    const int64_t o0 = off[sg.traj[s]];
    const int64_t t0 = sg.t0[s], t1 = t0 + sg.len[s];
    if (t1 <= t0) {
        if (j == 0)
            logLc[rec] = 0.0;
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

    // (segment starts and W are multiples of four: the lazy refresh falls on t % 4 == 3)
    const int W = Ws[ms];
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

    double a = real ? 1.0 / (double)n : 0.0, P = 1.0;
    double eP = 0.0;      // exponents removed inside the segment
    double S_start = 1.0; // LAZY: sum of the vector the segment starts from
    bool trouble = false; // LAZY: the vector left the range of the refresh
    bool dead = false;    // !LAZY: the sum became exactly zero (group-uniform)
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
            if constexpr (LAZY) {
                a = nj;
                if (r >= r0)
                    eP -= (double)pexp;
                if ((u & 3) == 3) {
                    const int E = wgroup_max<NP>(a > 0.0 ? exponent_of(a) : -(1 << 28));
                    trouble |= E < WIDE_TROUBLE_EXP;
                    a = ldexp(a, -E);
                    if (r >= r0)
                        eP += (double)E;
                }
                if (r == r0 - 1) {
                    if (real)
                        a_entry[rec * n + j] = a;
                    S_start = wgroup_sum<NP>(a);
                }
            } else {
                double c = wgroup_sum<NP>(nj);
                if (__builtin_expect(!(c >= 0x1p-959), 0)) {
                    if (c > 0.0) { // a sum in the denormal range: times 2^900, exactly (k_wide_fwd)
                        nj = ldexp(nj, 900);
                        c = wgroup_sum<NP>(nj);
                        pexp += 900;
                    } else {
                        dead = true; // probability zero from here on (a warm-up's support contains the true one)
                    }
                }
                a = dead ? 0.0 : nj * fast_rcp(c);
                if (r >= r0) {
                    if (!dead) {
                        int e;
                        P = frexp(P * c, &e);
                        eP += (double)(e - pexp);
                    }
                } else if (r == r0 - 1 && real) {
                    a_entry[rec * n + j] = a;
                }
            }
        }
    }
    if (real)
        a_exit[rec * n + j] = a;
    constexpr double LN2 = 0.693147180559945309417232121458;
    if constexpr (LAZY) {
        // the steps after the last refresh (all of them in a segment of one to three steps) are looked at here: an
        // exit sum below the refresh's range may have lost bits to the denormal grid.  The entry sum is taken right
        // after a refresh and is held to the same bound
        const double S_end = wgroup_sum<NP>(a);
        trouble |= !(S_end >= WIDE_RANGE_MIN) || !(S_start >= WIDE_RANGE_MIN) || !(S_end < INFINITY) ||
                   !(S_start < INFINITY);
        if (j == 0) {
            logLc[rec] = trouble ? 0.0 : (log(S_end) - log(S_start)) + eP * LN2;
            if (trouble)
                atomicAdd(&fails[ms], 1u);
        }
    } else {
        if (j == 0)
            logLc[rec] = dead ? -INFINITY : log(P) + eP * LN2;
    }
}

// sixteen lanes per boundary, 16 boundaries per workgroup of 256: grid ((nseg + 15) / 16, models)
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_score_wide_check(const Segs sg, int n,
                                                                                const double *logLc,
                                                                                const double *a_entry,
                                                                                const double *a_exit, double tol,
                                                                                unsigned int *fails)
{
    const int ms = blockIdx.y;
    const int s = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 4), l = threadIdx.x & 15;
    const int64_t rec = (int64_t)ms * sg.nseg + s;
    bool live = s < sg.nseg && sg.len[s] != 0 && sg.t0[s] != 0;
    if (live && (logLc[rec] == -INFINITY || logLc[rec - 1] == -INFINITY))
        live = false; // (the trajectory's probability is zero: -inf whatever the boundary)
    auto sum16 = [](double v) {
        v += __shfl_xor(v, 8, 16);
        v += __shfl_xor(v, 4, 16);
        v += __shfl_xor(v, 2, 16);
        return v + __shfl_xor(v, 1, 16);
    };
    const double *x = a_entry + rec * n, *y = a_exit + (rec - 1) * n;
    double sx = 0.0, sy = 0.0;
    if (live)
        for (int j = l; j < n; j += 16) {
            sx += x[j];
            sy += y[j];
        }
    sx = sum16(sx);
    sy = sum16(sy);
    double dev = 0.0;
    if (live) {
        if (!(sx > 0.0) || !(sy > 0.0)) {
            dev = 1.0;
        } else {
            for (int j = l; j < n; j += 16) {
                const double xs = x[j] / sx, ys = y[j] / sy;
                const double d = fabs(xs - ys);
                const double r = (ys > 1e-280) ? d / ys : (d > 1e-280 ? 1.0 : 0.0);
                dev = fmax(dev, r == r ? r : 1.0);
            }
        }
    }
    dev = fmax(dev, __shfl_xor(dev, 8, 16));
    dev = fmax(dev, __shfl_xor(dev, 4, 16));
    dev = fmax(dev, __shfl_xor(dev, 2, 16));
    dev = fmax(dev, __shfl_xor(dev, 1, 16));
    if (live && l == 0 && !(dev <= tol))
        atomicAdd(&fails[ms], 1u);
}

} // namespace bhmm
