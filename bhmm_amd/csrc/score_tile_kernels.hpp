// score_tile_kernels.hpp -- bhmm_score for 65..128 states: the forward-only, time-segmented pass on the fp64
// matrix cores (score_api.hip, launches in score_tile_nt.hip).  The tile geometry, the LDS row order and the
// emission helpers are those of the E-step's k_tile_fwd (tile_kernels.hpp, included and not changed); nothing
// of the E-step's state is read or written.
//
//   k_score_tile   grid (tiles, models of the batch), four wavefronts per workgroup, ONE model per workgroup
//                  (blockIdx.y: its table entry is uniform).  Sixteen segments form a tile; a step is
//                  [16 x NP] . [NP x NP] on v_mfma_f64_16x16x4_f64: wavefront w keeps column tiles w and w + 4
//                  of A in registers (B operand), the tile of the previous step is all-gathered through LDS at
//                  pitch TileGeo<NT>::PX.  Every wavefront takes both roles of k_tile_fwd<.., SPLIT = false>,
//                  and the emission row of the next step stays in registers (no hand-over through LDS).  The
//                  vectors are carried up to a power of two that is refreshed every fourth step.
//                  A row warms up for W (of the model) steps from the uniform vector -- or starts exactly from
//                  pi when the trajectory start is closer -- and the kernel writes per (model, segment) the
//                  log-normaliser, the entry vector it derived and the exit vector it computed.  Nothing per
//                  step goes to HBM.
//                  A row that leaves the range of the refresh (a vector below 2^-900, an all-zero one, a sum
//                  that is zero or not finite) counts in flags[3 model]: that model's numbers are not used.
//                  The exponent is measured on the step before the one that takes it off, so up to four steps
//                  lie between the last look and a segment's end; they are held to the same bound after the
//                  loop: an exit sum, or an entry sum, below 2^-900 (WIDE_RANGE_MIN) counts there as well.
//   k_score_tile_check  every derived entry vector against the predecessor's exit vector, componentwise
//                  relative after normalisation (k_score_wide_check); per model the failures in
//                  flags[3 model + 1] and the largest deviation, as the bits of a float, in flags[3 model + 2]
//                  (what the calibration of W reads).
//   The per (model, trajectory) sum of the segment terms is k_score_logl over the plan's traj0 table.
//
// Discrete emissions: B^T [M][n] of the model (made per call), read from global memory / L2 ONE STEP AHEAD of
// its use: the 16 lanes of a row read 128 consecutive bytes.  See DESIGN.md section 13 for why it is not in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "score_kernels.hpp"
#include "tile_kernels.hpp"

namespace bhmm {

// one entry of the model table in device memory
struct ScoreTileModel {
    WideModel w;      // A, pi, the gaussian constants
    const double *Bt; // discrete: B transposed, [M][n]
    int32_t W;        // warm-up of this model (a multiple of four)
};

constexpr int SCORE_TILE_THREADS = 256;
constexpr int SCORE_TILE_FLAGS = 3; // words per model: range flag, failed boundaries, largest deviation

template <int NT, int KIND, bool FULL>
__global__ __launch_bounds__(SCORE_TILE_THREADS) void k_score_tile(const ScoreTileModel *__restrict__ models,
                                                                   const int64_t *off, const Segs sg,
                                                                   const TilePlan tp, const void *obs_rm,
                                                                   double *logLc, double *a_entry, double *a_exit,
                                                                   unsigned int *flags)
{
    using G = TileGeo<NT>;
    constexpr int TPW = G::TPW, KK = G::KK, PX = G::PX, NP = G::NP;
    static_assert(NT >= 5 && NT <= 8 && TPW == 2, "65 .. 128 states: two column tiles per wavefront");
    static_assert(KIND == EMIT_GAUSS || KIND == EMIT_DISC, "explicit pobs take the serial recursion");
    __shared__ __attribute__((aligned(16))) double sX[2 * 16 * PX];
    __shared__ __attribute__((aligned(16))) double sObs[16 * 16]; // observations of 16 steps: [step & 15][4 q + r]
    __shared__ int sE[64];
    __shared__ double sEP[16]; // exponents removed in the main part of every row
    const int ms = blockIdx.y;
    const WideModel m = models[ms].w;
    const double *Bt = models[ms].Bt;
    const int W = models[ms].W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = lane & 15, q = lane >> 4;
    const int n = FULL ? NP : m.n;

    // ---- my four rows (lane (s, q), register r <-> row q + 4 r) ----------------------------------
    int nst[4], r0[4];
    bool fs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int sgi = tp.tile_seg[(int64_t)blockIdx.x * 16 + q + 4 * r];
        nst[r] = 0;
        r0[r] = 0;
        fs[r] = false;
        if (sgi >= 0 && sg.len[sgi] > 0) {
            const int64_t t0 = sg.t0[sgi], t1 = t0 + sg.len[sgi];
            const int64_t tw = (t0 - W > 0) ? t0 - W : 0;
            nst[r] = (int)(t1 - tw);
            r0[r] = (int)(t0 - tw);
            fs[r] = tw == 0;
        }
    }
    // (every wavefront holds all 16 rows: uniform over the workgroup, and said so to the compiler)
    const int nmax = __builtin_amdgcn_readfirstlane(tile_all_max(max(max(nst[0], nst[1]), max(nst[2], nst[3]))));
    const int g4 = (nmax + 3) & ~3;
    // steps [g2, g3): every row of the tile is inside its main part and not at its last step
    const int g2 = __builtin_amdgcn_readfirstlane(tile_all_max(max(max(r0[0], r0[1]), max(r0[2], r0[3]))));
    const int g3 = __builtin_amdgcn_readfirstlane(tile_all_min(min(min(nst[0], nst[1]), min(nst[2], nst[3])))) - 1;

    for (int e = tid; e < 16 * PX; e += SCORE_TILE_THREADS)
        sX[e] = (e % PX) < n ? 1.0 / (double)n : 0.0; // warm-ups start from the uniform vector
    bool real[TPW];
#pragma unroll
    for (int c = 0; c < TPW; ++c)
        real[c] = (w + 4 * c < NT) && (FULL || 16 * (w + 4 * c) + s < n);

    double Breg[TPW * KK], pi_j[TPW]; // my blocks of A (B operand)
    double mu_j[TPW], ga_j[TPW], gb_j[TPW];
#pragma unroll
    for (int c = 0; c < TPW; ++c) {
        const int j = 16 * (w + 4 * c) + s;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int i = q * KK + kk;
            Breg[c * KK + kk] = (real[c] && (FULL || i < n)) ? m.A[(int64_t)i * n + j] : 0.0;
        }
        pi_j[c] = real[c] ? m.pi[j] : 0.0;
        mu_j[c] = (KIND == EMIT_GAUSS && real[c]) ? m.mu[j] : 0.0;
        ga_j[c] = (KIND == EMIT_GAUSS && real[c]) ? m.ga[j] : 0.0;
        gb_j[c] = (KIND == EMIT_GAUSS && real[c]) ? m.gb[j] : 1.0;
    }
    int xw[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        xw[r] = tile_prow(q + 4 * r) * PX;
    const int xr = tile_prow(s) * PX + q * KK; // my operand: KK consecutive doubles of row s

    // ---- the observation stream: read ONCE per tile -- wavefront 0 loads, per group of four steps, one value
    // per (row, step), lane = 4 row + step, and passes them on through LDS (k_tile_fwd)
    const int lrow = lane >> 2, ldt = lane & 3;
    int64_t l_ob = 0;
    int l_last = 0;
    if (w == 0) {
        const int lgi = tp.tile_seg[(int64_t)blockIdx.x * 16 + lrow];
        if (lgi >= 0 && sg.len[lgi] > 0) {
            const int64_t o0 = off[sg.traj[lgi]], t0 = sg.t0[lgi], t1 = t0 + sg.len[lgi];
            const int64_t tw = (t0 - W > 0) ? t0 - W : 0;
            l_ob = o0 + tw;
            l_last = (int)(t1 - tw) - 1;
        }
    }
    const int lpos = 4 * (lrow & 3) + (lrow >> 2); // row q + 4 r sits at position 4 q + r
    auto obs_load = [&](int step) __attribute__((always_inline)) -> double {
        const int64_t g = l_ob + min(step, l_last);
        if constexpr (KIND == EMIT_DISC)
            return __hiloint2double(0, static_cast<const int32_t *>(obs_rm)[g]);
        else
            return static_cast<const double *>(obs_rm)[g];
    };
    double pend = 0.0; // the group two ahead, on its way
    // emission probabilities of my states for my four rows at step rs (discrete: the loads are issued here)
    auto emit = [&](double (&p)[TPW][4], int rs) __attribute__((always_inline)) {
        if constexpr (KIND == EMIT_GAUSS) {
            const tile_d2 lo = *reinterpret_cast<const tile_d2 *>(&sObs[(rs & 15) * 16 + 4 * q]);
            const tile_d2 hi = *reinterpret_cast<const tile_d2 *>(&sObs[(rs & 15) * 16 + 4 * q + 2]);
            const double o[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
            for (int c = 0; c < TPW; ++c) {
                double d[4];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    d[r] = o[r] - mu_j[c];
                gauss_pdf4_issue(d, ga_j[c], gb_j[c], m.gmg, p[c]); // (lanes without a state: a = 0, b = 1 -> 0)
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int sym = __double2loint(sObs[(rs & 15) * 16 + 4 * q + r]);
#pragma unroll
                for (int c = 0; c < TPW; ++c)
                    p[c][r] = real[c] ? Bt[(int64_t)sym * n + 16 * (w + 4 * c) + s] : 0.0;
            }
        }
    };

    // ---- entry and exit vectors: sixteen lanes per row, lane l takes states l + 16 e ---------------
    const int srow = tid >> 4, sl = tid & 15;
    int c_nst = 0, c_r0 = 0;
    int64_t c_rec = -1;
    {
        const int sgi = tp.tile_seg[(int64_t)blockIdx.x * 16 + srow];
        if (sgi >= 0 && sg.len[sgi] > 0) {
            const int64_t t0 = sg.t0[sgi], t1 = t0 + sg.len[sgi];
            const int64_t tw = (t0 - W > 0) ? t0 - W : 0;
            c_nst = (int)(t1 - tw);
            c_r0 = (int)(t0 - tw);
            c_rec = (int64_t)ms * sg.nseg + sgi;
        }
    }
    double S_start = 1.0, S_end = 0.0; // (a segment that starts its trajectory has no entry term)
    // the tile after step rs sits in LDS buffer (rs + 1) & 1
    auto capture = [&](int rs) __attribute__((always_inline)) {
        if (rs >= g2 && rs < g3) // (uniform: every row of the tile in its main part)
            return;
        if (rs < 0 || rs >= c_nst)
            return;
        const bool ent = rs == c_r0 - 1, ext = rs == c_nst - 1;
        if (!ent && !ext)
            return;
        const double *X = sX + ((rs + 1) & 1) * 16 * PX + tile_prow(srow) * PX;
        double *dst = (ent ? a_entry : a_exit) + c_rec * n;
        double sum = 0.0;
#pragma unroll
        for (int e = 0; e < NT; ++e) {
            const int j = sl + 16 * e;
            const double v = X[j]; // (padded states: zero)
            sum += v;
            if (FULL || j < n)
                dst[j] = v;
        }
        sum = row16_sum(sum); // (the sixteen lanes of a row take this branch together)
        if (ent)
            S_start = sum;
        else
            S_end = sum;
    };

    double pcur[TPW][4];                      // emission row of the step at hand
    double pld[KIND == EMIT_DISC ? TPW : 1][4]; // discrete: the next step's, on its way
    double eP[4] = {0.0, 0.0, 0.0, 0.0};
    bool trouble = false;

    auto step = [&](int rs, auto uc, auto mc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value, MODE = decltype(mc)::value;
        const double *X = sX + (u & 1) * 16 * PX; // (groups of four steps: the buffer is the step's parity)
        double *Xn = sX + ((u & 1) ^ 1) * 16 * PX;
        wide_d4 acc[TPW];
        constexpr int CH = KK % 8 == 0 ? 8 : (KK % 4 == 0 ? 4 : 2);
#pragma unroll
        for (int k0 = 0; k0 < KK; k0 += CH) {
            tile_d2 av[CH / 2];
#pragma unroll
            for (int k2 = 0; k2 < CH / 2; ++k2)
                av[k2] = *reinterpret_cast<const tile_d2 *>(X + xr + k0 + 2 * k2);
#pragma unroll
            for (int kk = k0; kk < k0 + CH; ++kk)
#pragma unroll
                for (int c = 0; c < TPW; ++c)
                    // (a column tile beyond NT: its block of A is zero, the product is computed all the same, see
                    // k_tile_fwd)
                    acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[(kk - k0) >> 1][(kk - k0) & 1], Breg[c * KK + kk],
                                                                  kk == 0 ? wide_d4{0.0, 0.0, 0.0, 0.0} : acc[c], 0, 0, 0);
        }
        // the exponent this step removes: row maxima of the step before, over the four wavefronts
        int E[4] = {0, 0, 0, 0};
        if constexpr (u == 3) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rho = q + 4 * r;
                E[r] = max(max(sE[rho], sE[16 + rho]), max(sE[32 + rho], sE[48 + rho]));
                const bool act = rs < nst[r];
                trouble |= act && E[r] < WIDE_TROUBLE_EXP;
                if (act && rs >= r0[r])
                    eP[r] += (double)E[r];
            }
        }
        int pm[4] = {-(1 << 28), -(1 << 28), -(1 << 28), -(1 << 28)};
#pragma unroll
        for (int c = 0; c < TPW; ++c) {
            if (NT % 4 == 0 || w + 4 * c < NT) {
                const int j = 16 * (w + 4 * c) + s;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double p = pcur[c][r];
                    double v = acc[c][r] * p;
                    if constexpr (MODE == TM_GEN)
                        if (fs[r] && rs == 0)
                            v = pi_j[c] * p;
                    if constexpr (u == 3)
                        v = ldexp(v, -E[r]);
                    Xn[xw[r] + j] = v;
                    if constexpr (u == 2)
                        pm[r] = max(pm[r], v > 0.0 ? exponent_of(v) : -(1 << 28));
                }
            }
        }
        if constexpr (u == 2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mx = row16_max_i32(pm[r]);
                if (s == 0)
                    sE[16 * w + q + 4 * r] = mx;
            }
        }
        // the vectors the previous step left at a segment's entry or exit
        capture(rs - 1);
        if constexpr (u == 0) {
            if (w == 0) { // the observations of the group two ahead go to LDS, the next ones are fetched
                sObs[((rs + 8 + ldt) & 15) * 16 + lpos] = pend;
                pend = obs_load(rs + 12 + ldt);
            }
        }
        // the emission row of the next step
        if constexpr (KIND == EMIT_DISC) {
#pragma unroll
            for (int c = 0; c < TPW; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pcur[c][r] = pld[c][r];
            emit(pld, rs + 2);
        } else {
            emit(pcur, rs + 1);
        }
        __syncthreads();
    };

    // ---- prologue: observations of the first two groups, the first emission rows ------------------
    if (w == 0) {
        sObs[ldt * 16 + lpos] = obs_load(ldt);
        sObs[(4 + ldt) * 16 + lpos] = obs_load(4 + ldt);
        pend = obs_load(8 + ldt);
    }
    __syncthreads();
    emit(pcur, 0);
    if constexpr (KIND == EMIT_DISC)
        emit(pld, 1);

    // groups of four steps; only the first step distinguishes rows that start their trajectory (pi o p_0
    // instead of the product)
    int rs = 0;
    if (g4 >= 4) {
        step(0, tile_ic<0>{}, tile_ic<TM_GEN>{});
        step(1, tile_ic<1>{}, tile_ic<TM_MAIN>{});
        step(2, tile_ic<2>{}, tile_ic<TM_MAIN>{});
        step(3, tile_ic<3>{}, tile_ic<TM_MAIN>{});
        rs = 4;
    }
    for (; rs + 4 <= g4; rs += 4) {
        step(rs, tile_ic<0>{}, tile_ic<TM_MAIN>{});
        step(rs + 1, tile_ic<1>{}, tile_ic<TM_MAIN>{});
        step(rs + 2, tile_ic<2>{}, tile_ic<TM_MAIN>{});
        step(rs + 3, tile_ic<3>{}, tile_ic<TM_MAIN>{});
    }
    capture(g4 - 1);

    // ---- per segment: log sum(exit) - log sum(entry) + ln 2 * removed exponents ---------------------
    if (w == 0 && s == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            sEP[q + 4 * r] = eP[r];
    }
    if (w == 0 && __any(trouble) && lane == 0)
        atomicAdd(&flags[SCORE_TILE_FLAGS * ms], 1u);
    __syncthreads();
    if (c_rec >= 0 && sl == 0) {
        // (the steps after the last refresh are looked at here: a sum below the refresh's range may have lost bits to
        // the denormal grid)
        const bool bad = !(S_end >= WIDE_RANGE_MIN) || !(S_start >= WIDE_RANGE_MIN) || !(S_end < INFINITY) ||
                         !(S_start < INFINITY);
        constexpr double LN2 = 0.693147180559945309417232121458;
        logLc[c_rec] = bad ? 0.0 : (log(S_end) - log(S_start)) + sEP[srow] * LN2;
        if (bad)
            atomicAdd(&flags[SCORE_TILE_FLAGS * ms], 1u);
    }
}

// sixteen lanes per boundary, 16 boundaries per workgroup of 256: grid ((nseg + 15) / 16, models)
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_score_tile_check(const Segs sg, int n,
                                                                                const double *a_entry,
                                                                                const double *a_exit, double tol,
                                                                                unsigned int *flags)
{
    const int ms = blockIdx.y;
    const int s = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 4), l = threadIdx.x & 15;
    const int64_t rec = (int64_t)ms * sg.nseg + s;
    const bool live = s < sg.nseg && sg.len[s] != 0 && sg.t0[s] != 0;
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
    if (live && l == 0) {
        if (!(dev <= tol))
            atomicAdd(&flags[SCORE_TILE_FLAGS * ms + 1], 1u);
        // (non-negative floats order like their bit patterns)
        atomicMax(&flags[SCORE_TILE_FLAGS * ms + 2], __float_as_uint((float)fmin(dev, 1e30)));
    }
}

} // namespace bhmm
