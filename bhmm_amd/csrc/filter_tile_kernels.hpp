// filter_tile_kernels.hpp -- bhmm_filter for 65..128 states: the time-segmented forward pass on the fp64 matrix
// cores with the filtered row and the increment as the last stage of every step (filter_api.hip, filter_path 3,
// launches in filter_tile_nt.hip).
//
//   k_filter_tile  k_score_tile (score_tile_kernels.hpp, included and not changed) for ONE model, no model
//                  dimension in the grid: grid (tiles), four wavefronts per workgroup, sixteen segments per tile;
//                  a step is [16 x NP] . [NP x NP] on v_mfma_f64_16x16x4_f64 with column tiles w and w + 4 of A in
//                  registers (B operand), the tile of the previous step all-gathered through LDS at pitch
//                  TileGeo<NT>::PX, the observation stream read once per tile by wavefront 0, B^T read one step
//                  ahead from global memory.  A row warms up for W steps from the uniform vector -- or starts
//                  exactly from pi when the trajectory start is closer -- and the kernel writes per segment the
//                  entry vector it derived and the exit vector it computed.  The vectors stay lazily scaled: a power
//                  of two refreshed every fourth step.
//                  The last stage runs for every step t of a row's main part in the thread layout of k_score_tile's
//                  capture (256 threads = 16 rows x 16 lanes; lane l takes states l + 16 e) on the tile X_t in LDS:
//                      S_t       the sum of the row (lane partials over e, then row16_sum)
//                      row       X_t[j] (1 / S_t): one division per step and row, every e stores 16 consecutive
//                                elements of the record; the conversion to OT is the last operation
//                      increment log S_t - log S_{t-1} + E_t ln 2, E_t the exponent the refresh removed at that
//                                step (non-zero on every fourth one); the previous logarithm is kept in a register
//                                (one log per step and row).  A segment's first main step takes S_{t-1} from its
//                                entry vector, a trajectory's first step has no previous term.
//                  Projection (PROJ): V staged in LDS as [q][state]; column q is the sum over the lane partials of
//                  a_i V[i][q] through row16_sum, in fp64 -- NOT in ascending i (the bound of the tests holds, the
//                  summation order of marg_project does not, as on the 9..64-state path); lane q < Q stores it.
//                  Warm-up steps emit nothing; rows == nullptr is a uniform branch; without WANT_LOGC logc is not
//                  touched.  rows == nullptr and no logc: only the entry and exit vectors (the calibration of W).
//                  Range: a segment sets its byte of seg_flag when k_score_tile's trouble condition holds for its
//                  row (exponent below WIDE_TROUBLE_EXP at a refresh, an all-zero vector) or when the sum of an
//                  emitted step, of the entry or of the exit vector is not a positive, normal, finite number
//                  (probability zero, an observation whose densities all underflow, a NaN observation).  The zero-row,
//                  -inf and row-of-ones rules are NOT reproduced here: the trajectories of such segments are done
//                  again, whole, on k_filter_serial.
//   k_filter_tile_redo   per trajectory: one byte, any of its segments flagged (over the plan's traj0 table, as
//                  k_filter_first_dead walks it); counts them in words[FILTER_TILE_REDONE].
//   k_filter_tile_check  k_score_tile_check on these vectors -- componentwise relative after normalisation --
//                  without the boundaries of a trajectory marked for redo: failures in words[FILTER_TILE_FAILS],
//                  the largest deviation as the bits of a float in words[FILTER_TILE_DEV].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marg_kernels.hpp" // MARG_QMAX
#include "score_kernels.hpp"
#include "score_tile_kernels.hpp" // ScoreTileModel, SCORE_TILE_THREADS
#include "tile_kernels.hpp"

namespace bhmm {

enum { FILTER_TILE_FAILS = 0, FILTER_TILE_DEV = 1, FILTER_TILE_REDONE = 2, FILTER_TILE_WORDS = 4 };

// rows: [total][PROJ ? Q : n] or nullptr; logc: [total], touched with WANT_LOGC only.  a_entry, a_exit: [nseg][n];
// seg_flag: [nseg]
template <int NT, int KIND, bool FULL, typename OT, bool PROJ, bool WANT_LOGC>
__global__ __launch_bounds__(SCORE_TILE_THREADS) void k_filter_tile(const ScoreTileModel *__restrict__ mp,
                                                                    const int64_t *off, const Segs sg,
                                                                    const TilePlan tp, const void *obs_rm,
                                                                    OT *__restrict__ rows,
                                                                    const double *__restrict__ V, int Q,
                                                                    OT *__restrict__ logc, double *a_entry,
                                                                    double *a_exit, uint8_t *seg_flag)
{
    using G = TileGeo<NT>;
    constexpr int TPW = G::TPW, KK = G::KK, PX = G::PX, NP = G::NP;
    static_assert(NT >= 5 && NT <= 8 && TPW == 2, "65 .. 128 states: two column tiles per wavefront");
    static_assert(KIND == EMIT_GAUSS || KIND == EMIT_DISC, "explicit pobs take the serial recursion");
    __shared__ __attribute__((aligned(16))) double sX[2 * 16 * PX];
    __shared__ __attribute__((aligned(16))) double sObs[16 * 16]; // observations of 16 steps: [step & 15][4 q + r]
    __shared__ double sV[PROJ ? MARG_QMAX * NP : 1];              // the projection, [q][state]
    __shared__ int sE[64];
    __shared__ int sTrouble[16]; // rows that left the range of the refresh
    const WideModel m = mp->w;
    const double *Bt = mp->Bt;
    const int W = mp->W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = lane & 15, q = lane >> 4;
    const int n = FULL ? NP : m.n;
    const bool quiet = !WANT_LOGC && rows == nullptr; // (uniform) boundary vectors only

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
    if constexpr (PROJ)
        for (int e = tid; e < MARG_QMAX * NP; e += SCORE_TILE_THREADS)
            sV[e] = (e % NP < n && e / NP < Q) ? V[(e % NP) * Q + e / NP] : 0.0;
    if (tid < 16)
        sTrouble[tid] = 0;
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
    // per (row, step), lane = 4 row + step, and passes them on through LDS (k_score_tile)
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

    // ---- the last stage: sixteen lanes per row, lane l takes states l + 16 e --------------------------
    const int srow = tid >> 4, sl = tid & 15;
    int c_nst = 0, c_r0 = 0, c_seg = -1;
    int64_t c_g0 = 0; // position of my row's step 0 in the concatenated arrays
    {
        const int sgi = tp.tile_seg[(int64_t)blockIdx.x * 16 + srow];
        if (sgi >= 0 && sg.len[sgi] > 0) {
            const int64_t t0 = sg.t0[sgi], t1 = t0 + sg.len[sgi];
            const int64_t tw = (t0 - W > 0) ? t0 - W : 0;
            c_nst = (int)(t1 - tw);
            c_r0 = (int)(t0 - tw);
            c_seg = sgi;
            c_g0 = off[sg.traj[sgi]] + tw;
        }
    }
    constexpr double LN2 = 0.693147180559945309417232121458;
    double lp = 0.0;  // log of the previous step's sum (0: the step starts its trajectory)
    bool bad = false; // a sum that is not positive, normal and finite (the same in the sixteen lanes of a row)
    // the tile after step rs sits in LDS buffer (rs + 1) & 1
    auto stage = [&](int rs) __attribute__((always_inline)) {
        if (quiet && rs >= g2 && rs < g3) // (uniform: every row of the tile in its main part)
            return;
        if (rs < 0 || rs >= c_nst || rs < c_r0 - 1) // (warm-up steps emit nothing)
            return;
        const bool ent = rs == c_r0 - 1, ext = rs == c_nst - 1;
        if (quiet && !ent && !ext)
            return;
        const double *X = sX + ((rs + 1) & 1) * 16 * PX + tile_prow(srow) * PX;
        double x[NT];
        double sum = 0.0;
#pragma unroll
        for (int e = 0; e < NT; ++e) {
            x[e] = X[sl + 16 * e]; // (padded states: zero)
            sum += x[e];
        }
        sum = row16_sum(sum); // (the sixteen lanes of a row take this branch together)
        bad |= !(sum >= 0x1p-1022 && sum < INFINITY);
        if (ent || ext) {
            double *dst = (ent ? a_entry : a_exit) + (int64_t)c_seg * n;
#pragma unroll
            for (int e = 0; e < NT; ++e)
                if (FULL || sl + 16 * e < n)
                    dst[sl + 16 * e] = x[e];
        }
        if (ent) { // the entry vector: what the first main step's increment is measured against
            if constexpr (WANT_LOGC)
                lp = log(sum);
            return;
        }
        const int64_t g = c_g0 + rs;
        if (rows) {
            const double rcp = 1.0 / sum;
            if constexpr (PROJ) {
                double mine = 0.0;
#pragma unroll
                for (int qq = 0; qq < MARG_QMAX; ++qq)
                    if (qq < Q) { // (uniform)
                        double part = 0.0;
#pragma unroll
                        for (int e = 0; e < NT; ++e)
                            part = fma(x[e] * rcp, sV[qq * NP + sl + 16 * e], part);
                        part = row16_sum(part);
                        mine = sl == qq ? part : mine;
                    }
                if (sl < Q)
                    rows[g * Q + sl] = (OT)mine;
            } else {
                OT *dst = rows + g * n;
#pragma unroll
                for (int e = 0; e < NT; ++e)
                    if (FULL || sl + 16 * e < n)
                        dst[sl + 16 * e] = (OT)(x[e] * rcp);
            }
        }
        if constexpr (WANT_LOGC) {
            // the exponent the refresh removed at this step: the row maxima of the step before, still in sE
            const int E = (rs & 3) == 3 ? max(max(sE[srow], sE[16 + srow]), max(sE[32 + srow], sE[48 + srow])) : 0;
            const double ls = log(sum);
            if (sl == 0)
                logc[g] = (OT)((ls - lp) + (double)E * LN2);
            lp = ls;
        }
    };

    double pcur[TPW][4];                      // emission row of the step at hand
    double pld[KIND == EMIT_DISC ? TPW : 1][4]; // discrete: the next step's, on its way
    int trouble = 0;                            // bit r: my row q + 4 r left the range

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
                trouble |= (rs < nst[r] && E[r] < WIDE_TROUBLE_EXP) ? (1 << r) : 0;
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
        // the row and the increment of the previous step (the tile it left is the one this step reads)
        stage(rs - 1);
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
    stage(g4 - 1);

    // ---- per segment: did its row stay inside the range ---------------------------------------------
    if (w == 0 && s == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if ((trouble >> r) & 1)
                sTrouble[q + 4 * r] = 1;
    }
    __syncthreads();
    if (c_seg >= 0 && sl == 0)
        seg_flag[c_seg] = (bad || sTrouble[srow] != 0) ? 1 : 0;
}

// one wavefront per trajectory; traj0: [K + 1] first segment of each trajectory
[[maybe_unused]] static __global__ __launch_bounds__(64) void k_filter_tile_redo(const int32_t *__restrict__ traj0,
                                                                                const uint8_t *__restrict__ seg_flag,
                                                                                uint8_t *__restrict__ redo,
                                                                                unsigned int *words)
{
    const int k = blockIdx.x;
    int any = 0;
    for (int g = traj0[k] + (int)threadIdx.x; g < traj0[k + 1]; g += 64)
        any |= seg_flag[g];
    const bool marked = __any(any != 0);
    if (threadIdx.x == 0) {
        redo[k] = marked ? 1 : 0;
        if (marked)
            atomicAdd(&words[FILTER_TILE_REDONE], 1u);
    }
}

// sixteen lanes per boundary, 16 boundaries per workgroup of 256: grid ((nseg + 15) / 16)
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_filter_tile_check(const Segs sg, int n,
                                                                                 const double *a_entry,
                                                                                 const double *a_exit,
                                                                                 const uint8_t *__restrict__ redo,
                                                                                 double tol, unsigned int *words)
{
    const int s = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 4), l = threadIdx.x & 15;
    const bool live = s < sg.nseg && sg.len[s] != 0 && sg.t0[s] != 0 && redo[sg.traj[s]] == 0;
    const double *x = a_entry + (int64_t)s * n, *y = a_exit + ((int64_t)s - 1) * n;
    double sx = 0.0, sy = 0.0;
    if (live)
        for (int j = l; j < n; j += 16) {
            sx += x[j];
            sy += y[j];
        }
    sx = row16_sum(sx);
    sy = row16_sum(sy);
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
            atomicAdd(&words[FILTER_TILE_FAILS], 1u);
        // (non-negative floats order like their bit patterns)
        atomicMax(&words[FILTER_TILE_DEV], __float_as_uint((float)fmin(dev, 1e30)));
    }
}

} // namespace bhmm
