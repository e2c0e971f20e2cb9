// smooth_tile_kernels.hpp -- bhmm_posterior_decode / bhmm_posterior_marginals for 65..128 states: the backward half
// of the time-segmented smoothing pass on the fp64 matrix cores (smooth_tile.hip, post_path / marg_path 3, launches in
// smooth_tile_nt.hip).  The forward half is k_filter_tile<NT, KIND, FULL, double, false, false>
// (filter_tile_kernels.hpp, included and not changed), which leaves the normalised filtered row a^_t of every step
// of a range of segments in a workspace.
//
//   k_smooth_tile_bwd  the geometry of k_filter_tile: grid (tiles), four wavefronts per workgroup, sixteen segments
//                  per tile, the same observation stream through sObs (read downwards), the same emit and the same
//                  lazy power-of-two refresh every fourth step.  A row walks time downwards: the B operand of
//                  v_mfma_f64_16x16x4_f64 holds the blocks of A^T (A[j][i] where the forward kernel holds A[i][j]),
//                  the tile multiplied is v_{t+1} = p_{t+1} o b_{t+1} (LDS, pitch TileGeo<NT>::PX), the product is
//                  b_t -- lazily scaled, its scale is never needed and nothing is counted -- and v_t = p_t o b_t goes
//                  to the other buffer.  b_t itself is kept in a second pair of LDS tiles next to the v tiles: the
//                  last stage forms gamma from b_t, never from v_t / p_t.
//                  A segment [t0, t1) of a trajectory of T steps starts at step min(T - 1, t1 - 1 + W) from the
//                  all-ones vector -- exact when that is T - 1, else a warm-up -- and walks down to t0, and one
//                  recursion step further when t0 > 0.  Warm-up steps read no a^ row and emit nothing.  Per segment
//                  the kernel writes the b vector it assumed for step t1 - 1 (b_exit) and the one it computed for
//                  step t0 - 1 (b_entry; that step needs no a^), both divided by their sum: the pair that
//                  k_smooth_wide_bwd writes.
//                  The last stage runs in k_filter_tile's stage layout (256 threads = 16 rows x 16 lanes; lane l
//                  takes states l + 16 e) for every step of a row's main part: g_j = a^_t(j) b_t(j), the a^ elements
//                  read straight from the workspace row one step ahead (16 lanes x 8 bytes = one 128-byte line per
//                  e), S = row16_sum of the lane partials, then by FORM
//                      decode u8 / i32   the row maximum of g and the LOWEST state with g == max (the tie rule of
//                                        k_post_gamma_rm: within a lane ascending e with a strict >, then the
//                                        smallest index among the lanes that hold the maximum); with conf (a
//                                        uniform branch) (float)(max / S); one thread per row stores
//                      rows f64 / f32    g_j / S with one reciprocal per step and row, every e stores 16
//                                        consecutive elements; the conversion is the last operation
//                      projection        V staged in LDS as [q][state]; column q is row16_sum of the lane partials
//                                        of gamma_j V[j][q], in fp64 -- the order of that tree, NOT ascending j (the
//                                        bound of the tests holds, the summation order of marg_project does not, as
//                                        in sections 16 and 17); lane q < Q stores it
//                  out == nullptr (uniform): the two boundary vectors only, no a^ is read (the calibration of W).
//                  Range: a segment sets its byte of seg_flag when k_filter_tile's trouble condition holds for its
//                  row (exponent below WIDE_TROUBLE_EXP at a refresh, an all-zero vector), when S of an emitted
//                  step is not a positive, normal, finite number, or when the sum of a boundary vector is not one
//                  (so that it cannot be normalised).  NaN, zero-probability and outlier input only ever sets that
//                  byte: every loop bound and every address is a function of the plan alone.
//   k_smooth_tile_flags   counts the segments either direction flagged.
//   k_smooth_tile_check   k_filter_tile_check's rule (componentwise relative after normalisation) on the boundary
//                  vectors of both directions, failures and the largest deviation per direction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "filter_tile_kernels.hpp"
#include "marg_kernels.hpp" // MARG_QMAX
#include "score_tile_kernels.hpp" // ScoreTileModel, SCORE_TILE_THREADS
#include "tile_kernels.hpp"

namespace bhmm {

enum {
    SMT_DECODE_U8 = 0,
    SMT_DECODE_I32 = 1,
    SMT_ROWS_F64 = 2,
    SMT_ROWS_F32 = 3,
    SMT_PROJ_F64 = 4,
    SMT_PROJ_F32 = 5,
    SMT_FORMS = 6
};
// the words of a pass: boundaries out of tolerance and the largest deviation (bits of a float) per direction,
// segments flagged by either direction
enum { SMT_FAILS_F = 0, SMT_DEV_F = 1, SMT_FAILS_B = 2, SMT_DEV_B = 3, SMT_FLAGGED = 4, SMT_WORDS = 8 };

// largest element / smallest integer of the 16 lanes of a row, in every lane (the butterfly of row16_sum)
__device__ __forceinline__ double row16_fmax(double v)
{
    v = fmax(v, dpp_f64<0xB1>(v));
    v = fmax(v, dpp_f64<0x4E>(v));
    v = fmax(v, dpp_f64<0x141>(v));
    v = fmax(v, dpp_f64<0x140>(v));
    return v;
}
__device__ __forceinline__ int row16_min_i32(int v)
{
    v = min(v, dpp_i32<0xB1>(v));
    v = min(v, dpp_i32<0x4E>(v));
    v = min(v, dpp_i32<0x141>(v));
    v = min(v, dpp_i32<0x140>(v));
    return v;
}

// ws: the filtered rows of the launch's segments, global step g at ws[(g - g_first) * n].  out: the paths ([total]
// of uint8_t / int32_t), the rows ([total][n] of double / float) or their projection ([total][Q]), or nullptr; conf:
// [total] or nullptr (decode only).  b_exit, b_entry: [nseg][n]; seg_flag: [nseg]
template <int NT, int KIND, bool FULL, int FORM>
__global__ __launch_bounds__(SCORE_TILE_THREADS) void k_smooth_tile_bwd(const ScoreTileModel *__restrict__ mp,
                                                                        const int64_t *off, const Segs sg,
                                                                        const TilePlan tp, const void *obs_rm,
                                                                        const double *__restrict__ ws,
                                                                        int64_t g_first, void *__restrict__ out,
                                                                        float *__restrict__ conf,
                                                                        const double *__restrict__ V, int Q,
                                                                        double *b_exit, double *b_entry,
                                                                        uint8_t *seg_flag)
{
    using G = TileGeo<NT>;
    constexpr int TPW = G::TPW, KK = G::KK, PX = G::PX, NP = G::NP;
    constexpr bool PROJ = FORM == SMT_PROJ_F64 || FORM == SMT_PROJ_F32;
    constexpr bool DECODE = FORM == SMT_DECODE_U8 || FORM == SMT_DECODE_I32;
    static_assert(NT >= 5 && NT <= 8 && TPW == 2, "65 .. 128 states: two column tiles per wavefront");
    static_assert(KIND == EMIT_GAUSS || KIND == EMIT_DISC, "explicit pobs take the generic route");
    static_assert(FORM >= 0 && FORM < SMT_FORMS, "six forms");
    __shared__ __attribute__((aligned(16))) double sX[2 * 16 * PX]; // v = p o b: the operand of the product
    __shared__ __attribute__((aligned(16))) double sB[2 * 16 * PX]; // b itself: what the last stage reads
    __shared__ __attribute__((aligned(16))) double sObs[16 * 16];   // observations of 16 steps: [step & 15][4 q + r]
    __shared__ double sV[PROJ ? MARG_QMAX * NP : 1];                // the projection, [q][state]
    __shared__ int sE[64];
    __shared__ int sTrouble[16]; // rows that left the range of the refresh
    const WideModel m = mp->w;
    const double *Bt = mp->Bt;
    const int W = mp->W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = lane & 15, q = lane >> 4;
    const int n = FULL ? NP : m.n;
    const bool quiet = out == nullptr; // (uniform) boundary vectors only

    // one row: the segment of tile row rho walks the steps te, te - 1, ...; step index k is time te - k.  rin: the
    // first index of the main part (the warm-up before it), nst: the index behind it, ntot: with the recursion step
    // to t0 - 1 when there is one.  gt: the global position of index 0
    auto row_of = [&](int rho, int &rin, int &nst, int &ntot, int64_t &gt) __attribute__((always_inline)) -> int {
        const int sgi = tp.tile_seg[(int64_t)blockIdx.x * 16 + rho];
        rin = nst = ntot = 0;
        gt = 0;
        if (sgi < 0 || sg.len[sgi] <= 0)
            return -1;
        const int k = sg.traj[sgi];
        const int64_t o0 = off[k], T = off[k + 1] - o0;
        const int64_t t0 = sg.t0[sgi], t1 = t0 + sg.len[sgi];
        const int64_t te = t1 - 1 + W < T - 1 ? t1 - 1 + W : T - 1; // (T - 1: exact)
        rin = (int)(te - (t1 - 1));
        nst = (int)(te - t0) + 1;
        ntot = nst + (t0 > 0 ? 1 : 0);
        gt = o0 + te;
        return sgi;
    };

    // ---- my four rows (lane (s, q), register r <-> row q + 4 r) ----------------------------------
    int ntot[4];
    int rin_mx = 0, nst_mn = 1 << 30, ntot_mx = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int rin, nst;
        int64_t gt;
        row_of(q + 4 * r, rin, nst, ntot[r], gt);
        rin_mx = max(rin_mx, rin);
        nst_mn = min(nst_mn, nst);
        ntot_mx = max(ntot_mx, ntot[r]);
    }
    // (every wavefront holds all 16 rows: uniform over the workgroup, and said so to the compiler)
    const int nmax = __builtin_amdgcn_readfirstlane(tile_all_max(ntot_mx));
    const int g4 = (nmax + 3) & ~3;
    // indices (g2, g3): every row of the tile is inside its main part, behind its first step there
    const int g2 = __builtin_amdgcn_readfirstlane(tile_all_max(rin_mx));
    const int g3 = __builtin_amdgcn_readfirstlane(tile_all_min(nst_mn));

    for (int e = tid; e < 2 * 16 * PX; e += SCORE_TILE_THREADS) {
        sX[e] = 0.0; // (index 0 takes the all-ones vector instead of the product)
        sB[e] = 0.0;
    }
    if constexpr (PROJ)
        for (int e = tid; e < MARG_QMAX * NP; e += SCORE_TILE_THREADS)
            sV[e] = (e % NP < n && e / NP < Q) ? V[(e % NP) * Q + e / NP] : 0.0;
    if (tid < 16)
        sTrouble[tid] = 0;
    bool real[TPW];
#pragma unroll
    for (int c = 0; c < TPW; ++c)
        real[c] = (w + 4 * c < NT) && (FULL || 16 * (w + 4 * c) + s < n);

    double Breg[TPW * KK]; // my blocks of A^T (B operand)
    double mu_j[TPW], ga_j[TPW], gb_j[TPW];
#pragma unroll
    for (int c = 0; c < TPW; ++c) {
        const int j = 16 * (w + 4 * c) + s;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int i = q * KK + kk;
            Breg[c * KK + kk] = (real[c] && (FULL || i < n)) ? m.A[(int64_t)j * n + i] : 0.0;
        }
        mu_j[c] = (KIND == EMIT_GAUSS && real[c]) ? m.mu[j] : 0.0;
        ga_j[c] = (KIND == EMIT_GAUSS && real[c]) ? m.ga[j] : 0.0;
        gb_j[c] = (KIND == EMIT_GAUSS && real[c]) ? m.gb[j] : 1.0;
    }
    int xw[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        xw[r] = tile_prow(q + 4 * r) * PX;
    const int xr = tile_prow(s) * PX + q * KK; // my operand: KK consecutive doubles of row s

    // ---- the observation stream: read ONCE per tile -- wavefront 0 loads, per group of four indices, one value
    // per (row, index), lane = 4 row + index, and passes them on through LDS (k_filter_tile, downwards in time)
    const int lrow = lane >> 2, ldt = lane & 3;
    int64_t l_ob = 0;
    int l_last = 0;
    if (w == 0) {
        int rin, nst, nt;
        if (row_of(lrow, rin, nst, nt, l_ob) >= 0)
            l_last = nt - 1;
    }
    const int lpos = 4 * (lrow & 3) + (lrow >> 2); // row q + 4 r sits at position 4 q + r
    auto obs_load = [&](int k) __attribute__((always_inline)) -> double {
        const int64_t g = l_ob - min(k, l_last);
        if constexpr (KIND == EMIT_DISC)
            return __hiloint2double(0, static_cast<const int32_t *>(obs_rm)[g]);
        else
            return static_cast<const double *>(obs_rm)[g];
    };
    double pend = 0.0; // the group two ahead, on its way
    // emission probabilities of my states for my four rows at index rs (discrete: the loads are issued here)
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
    int c_rin, c_nst, c_ntot;
    int64_t c_gt;
    const int c_seg = row_of(srow, c_rin, c_nst, c_ntot, c_gt);
    bool bad = false; // a sum that is not positive, normal and finite (the same in the sixteen lanes of a row)
    double apf[NT];   // a^ of my row's next emitted step, on its way
#pragma unroll
    for (int e = 0; e < NT; ++e)
        apf[e] = 0.0;
    // b of index k sits in LDS buffer (k + 1) & 1
    auto stage = [&](int k) __attribute__((always_inline)) {
        double a[NT];
#pragma unroll
        for (int e = 0; e < NT; ++e)
            a[e] = apf[e];
        if (!quiet && k + 1 >= c_rin && k + 1 < c_nst) { // (warm-up steps read no a^ row)
            const double *src = ws + (c_gt - (k + 1) - g_first) * n;
#pragma unroll
            for (int e = 0; e < NT; ++e)
                apf[e] = (FULL || sl + 16 * e < n) ? src[sl + 16 * e] : 0.0;
        }
        if (quiet && k > g2 && k < g3) // (uniform: every row of the tile inside its main part)
            return;
        if (k < c_rin || k >= c_ntot) // (warm-up steps emit nothing; k < 0 and empty rows: c_ntot == 0)
            return;
        const bool ext = k == c_rin, ent = k == c_nst;
        if (quiet && !ext && !ent)
            return;
        const double *X = sB + ((k + 1) & 1) * 16 * PX + tile_prow(srow) * PX;
        double x[NT];
#pragma unroll
        for (int e = 0; e < NT; ++e)
            x[e] = X[sl + 16 * e]; // (padded states: zero)
        if (ext || ent) { // (the sixteen lanes of a row take these branches together)
            double sum = 0.0;
#pragma unroll
            for (int e = 0; e < NT; ++e)
                sum += x[e];
            sum = row16_sum(sum);
            bad |= !(sum >= 0x1p-1022 && sum < INFINITY);
            const double rcp = 1.0 / sum;
            double *dst = (ent ? b_entry : b_exit) + (int64_t)c_seg * n;
#pragma unroll
            for (int e = 0; e < NT; ++e)
                if (FULL || sl + 16 * e < n)
                    dst[sl + 16 * e] = x[e] * rcp;
        }
        if (ent || quiet)
            return;
        double S = 0.0;
#pragma unroll
        for (int e = 0; e < NT; ++e) {
            x[e] *= a[e]; // g_j = a^_t(j) b_t(j)
            S += x[e];
        }
        S = row16_sum(S);
        bad |= !(S >= 0x1p-1022 && S < INFINITY);
        const int64_t g = c_gt - k;
        if constexpr (DECODE) {
            using PT = std::conditional_t<FORM == SMT_DECODE_U8, uint8_t, int32_t>;
            double best = x[0];
            int bi = sl;
#pragma unroll
            for (int e = 1; e < NT; ++e)
                if (x[e] > best) {
                    best = x[e];
                    bi = sl + 16 * e;
                }
            const double mx = row16_fmax(best);
            const int arg = row16_min_i32(best == mx ? bi : (1 << 20)); // (no lane holds it: NaN, flagged above)
            if (sl == 0) {
                static_cast<PT *>(out)[g] = (PT)(arg < NP ? arg : 0);
                if (conf)
                    conf[g] = (float)(mx / S);
            }
        } else {
            using OT = std::conditional_t<FORM == SMT_ROWS_F64 || FORM == SMT_PROJ_F64, double, float>;
            const double rcp = 1.0 / S;
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
                    static_cast<OT *>(out)[g * Q + sl] = (OT)mine;
            } else {
                OT *dst = static_cast<OT *>(out) + g * n;
#pragma unroll
                for (int e = 0; e < NT; ++e)
                    if (FULL || sl + 16 * e < n)
                        dst[sl + 16 * e] = (OT)(x[e] * rcp);
            }
        }
    };

    double pcur[TPW][4];                        // emission row of the index at hand
    double pld[KIND == EMIT_DISC ? TPW : 1][4]; // discrete: the next index's, on its way
    int trouble = 0;                            // bit r: my row q + 4 r left the range

    auto step = [&](int rs, auto uc, auto mc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value, MODE = decltype(mc)::value;
        const double *X = sX + (u & 1) * 16 * PX; // (groups of four indices: the buffer is the index's parity)
        double *Xn = sX + ((u & 1) ^ 1) * 16 * PX;
        double *Bn = sB + ((u & 1) ^ 1) * 16 * PX;
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
                    // (a column tile beyond NT: its block of A^T is zero, the product is computed all the same)
                    acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[(kk - k0) >> 1][(kk - k0) & 1], Breg[c * KK + kk],
                                                                  kk == 0 ? wide_d4{0.0, 0.0, 0.0, 0.0} : acc[c], 0, 0,
                                                                  0);
        }
        // the exponent this index removes: row maxima of the index before, over the four wavefronts
        int E[4] = {0, 0, 0, 0};
        if constexpr (u == 3) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rho = q + 4 * r;
                E[r] = max(max(sE[rho], sE[16 + rho]), max(sE[32 + rho], sE[48 + rho]));
                trouble |= (rs < ntot[r] && E[r] < WIDE_TROUBLE_EXP) ? (1 << r) : 0;
            }
        }
        int pm[4] = {-(1 << 28), -(1 << 28), -(1 << 28), -(1 << 28)};
#pragma unroll
        for (int c = 0; c < TPW; ++c) {
            if (NT % 4 == 0 || w + 4 * c < NT) {
                const int j = 16 * (w + 4 * c) + s;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double b = acc[c][r];
                    if constexpr (MODE == TM_GEN)
                        if (rs == 0)
                            b = real[c] ? 1.0 : 0.0; // every row starts from the all-ones vector
                    if constexpr (u == 3)
                        b = ldexp(b, -E[r]);
                    const double v = b * pcur[c][r];
                    Bn[xw[r] + j] = b;
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
        // the outputs of the previous index (the b tile it left is not written before the next barrier)
        stage(rs - 1);
        if constexpr (u == 0) {
            if (w == 0) { // the observations of the group two ahead go to LDS, the next ones are fetched
                sObs[((rs + 8 + ldt) & 15) * 16 + lpos] = pend;
                pend = obs_load(rs + 12 + ldt);
            }
        }
        // the emission row of the next index
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

    // groups of four indices; only index 0 is special (the all-ones vector instead of the product)
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

// segments with a flag set in either direction (forward: k_filter_tile's seg_flag, dead segments included)
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_smooth_tile_flags(const uint8_t *fwd,
                                                                                   const uint8_t *bwd, int nseg,
                                                                                   unsigned int *words)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nseg && (fwd[s] | bwd[s]))
        atomicAdd(&words[SMT_FLAGGED], 1u);
}

// deviation of boundary vector x from y by k_filter_tile_check's rule: sixteen lanes per boundary, lane l
__device__ __forceinline__ double smooth_tile_dev(const double *x, const double *y, int n, int l, bool live)
{
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
    return dev;
}

// sixteen lanes per boundary, 16 boundaries per workgroup of 256: grid ((nseg + 15) / 16).  The boundary in front
// of segment s: the entry vector s derived against the exit vector of s - 1, forward; the b vector s computed for
// step t0 - 1 against the one s - 1 assumed there, backward
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_smooth_tile_check(const Segs sg, int n,
                                                                                   const double *a_entry,
                                                                                   const double *a_exit,
                                                                                   const double *b_entry,
                                                                                   const double *b_exit, double tol,
                                                                                   unsigned int *words)
{
    const int s = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 4), l = threadIdx.x & 15;
    const bool live = s < sg.nseg && sg.len[s] != 0 && sg.t0[s] != 0;
    const int64_t at = (int64_t)s * n, before = ((int64_t)s - 1) * n;
    const double df = smooth_tile_dev(a_entry + at, a_exit + before, n, l, live);
    const double db = smooth_tile_dev(b_entry + at, b_exit + before, n, l, live);
    if (live && l == 0) {
        if (!(df <= tol))
            atomicAdd(&words[SMT_FAILS_F], 1u);
        if (!(db <= tol))
            atomicAdd(&words[SMT_FAILS_B], 1u);
        // (non-negative floats order like their bit patterns)
        atomicMax(&words[SMT_DEV_F], __float_as_uint((float)fmin(df, 1e30)));
        atomicMax(&words[SMT_DEV_B], __float_as_uint((float)fmin(db, 1e30)));
    }
}

} // namespace bhmm
