// pair_tile_kernels.hpp -- the row kernel of the generic path of bhmm_posterior_transitions (pair_api.hip) for up to
// 128 states on the matrix cores; DESIGN.md section 21.  From the filtered rows f_t and the posterior rows
// gamma_(t+1) that the generic path already has, per step (P, U_q: 1 x n)
//     P     = f A                          r_j = P_j > 0 ? gamma_(t+1)(j) / P_j : 0
//     U_q   = f M_q,  M_q = A o W_q        (jump form: ONE M, A with its diagonal zeroed)
//     out_q = (sum_j U_q[j] r_j) * (1 / sum_j P_j r_j)
// which is sum_ij f_i A_ij W_ijq r_j / sum_ij f_i A_ij r_j, the quantity k_pair_rows forms, in another order of
// summation.  For 16 consecutive steps F [16 x NP] . [A | M_1 | ... ] is a GEMM on v_mfma_f64_16x16x4 whose
// column blocks all take the same A-operand; r, the two sums over j and the division are an epilogue on the
// accumulators.
//
// Layouts (v_mfma_f64_16x16x4, lane = 16 k + i): A-operand element (row i, k), B-operand element (k, column i);
// result register g of lane l is element (row (l >> 4) + 4 g, column l & 15) -- NOT the f32 row formula.
//   Bop    the matrices in operand order, built by the host: Bop[((m * NT + c) * 4 NT + kk) * 64 + lane] =
//          M_m[4 kk + (lane >> 4)][16 c + (lane & 15)], m = 0 being A; rows and columns beyond n are zero.  The 4 NT
//          fragments of one (m, c) are a SLAB of NT * 256 doubles.
//   work   a workgroup is four wavefronts, a wavefront owns ONE tile of 16 consecutive steps of the concatenated
//          arrays with its F fragments and r in registers (two and four tiles per wavefront were slower at every
//          size: registers halve the wavefronts per SIMD, and it is they that hide the loads).  The slabs go through
//          LDS one after the other, double-buffered (the next one is on its way from L2 while this one multiplies),
//          so the matrices are read once per 64 steps.  One __syncthreads per slab; every wavefront takes part in all
//          of them, with or without rows.
//   masks  a row has n doubles and the next row follows at once: every load is guarded by column < n, by
//          step < total, and the gamma row of step e + 1 by "e is not the last step of its trajectory" (from offsets,
//          by the rule of k_pair_rows), which covers e + 1 == total.  Masked elements are 0.0, never loaded.  The
//          last step of a trajectory writes an exact zero row; steps >= total write nothing.
// Fixed order throughout: the k-sum is the matrix core's, the sum over j is column tiles ascending per lane, then an
// xor butterfly (additions of swapped pairs commute, so all 16 lanes of a row hold the same bits) -- no atomics,
// nothing depends on scheduling, and a row's value depends on its own two input rows and the matrices only.  gam is
// read-only here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bhmm {

typedef double pair_v4d __attribute__((ext_vector_type(4)));

constexpr int PAIR_TILE_WAVES = 4;                        // wavefronts, and tiles of 16 steps, per workgroup
constexpr int pair_tile_slab(int NT) { return NT * 256; } // doubles of one (m, c)

// the sum over the 16 lanes of a DPP row, the same bits in each of them
__device__ __forceinline__ double pair_row16_sum(double v)
{
#pragma unroll
    for (int d = 1; d < 16; d <<= 1)
        v += __shfl_xor(v, d, 64);
    return v;
}

// NT = ceil(n / 16) column tiles; OT: double or float.  nm: matrices in Bop (1 + Q, or 2 for the jump form);
// out: [total][Qp], Qp = nm - 1.
template <int NT, typename OT>
__global__ __launch_bounds__(64 * PAIR_TILE_WAVES) void k_pair_tile(const double *__restrict__ filt,
                                                                    const double *__restrict__ gam,
                                                                    const double *__restrict__ Bop, int nm, int n,
                                                                    int64_t total, int K,
                                                                    const int64_t *__restrict__ offsets,
                                                                    OT *__restrict__ out)
{
    constexpr int KK = 4 * NT, SLAB = pair_tile_slab(NT);
    constexpr int TPB = 64 * PAIR_TILE_WAVES, PER = SLAB / TPB; // (= NT doubles of a slab per thread)
    __shared__ double sB[2][SLAB];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int64_t e0 = ((int64_t)blockIdx.x * PAIR_TILE_WAVES + wave) * 16; // first step of this wavefront's tile
    const int Qp = nm - 1;

    // A-operand fragments of the filtered rows: element (row li, k = 4 kk + lk)
    double F[KK];
    {
        const int64_t e = e0 + li;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int col = 4 * kk + lk;
            F[kk] = (e < total && col < n) ? filt[e * n + col] : 0.0;
        }
    }
    // The last steps of trajectories among the 16 steps of the tile, bit d of endmask for step e0 + d: ONE search for
    // the trajectory of e0 (the last k with offsets[k] <= e0, as k_pair_rows has it per step), then the offsets after
    // it, 64 at a time, until they leave the tile (offsets ascend; offsets[K] == total)
    unsigned endmask = 0;
    if (e0 < total) { // (uniform in the wavefront)
        int lo = 0, hi = K;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (offsets[mid] <= e0)
                lo = mid;
            else
                hi = mid;
        }
        for (int base = lo + 1; base <= K; base += 64) {
            const int k = base + lane;
            const int64_t d = k <= K ? offsets[k] - 1 - e0 : (int64_t)16; // (>= 0: offsets[k] > e0 for k > lo)
            endmask |= d >= 0 && d < 16 ? 1u << d : 0u;
            if (__shfl(d, 63, 64) >= 16)
                break;
        }
#pragma unroll
        for (int x = 1; x < 64; x <<= 1)
            endmask |= __shfl_xor(endmask, x, 64);
    }
    // gamma of the next step in the C / D layout (r[c][g]: row lk + 4 g, column 16 c + li), zero for a last step;
    // bit g of valid / ends: that row exists / is the last step of its trajectory
    pair_v4d r[NT];
    unsigned valid = 0, ends = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int64_t e = e0 + lk + 4 * g;
        const bool ok = e < total;
        const bool end = !ok || (endmask >> (lk + 4 * g) & 1u) || e + 1 >= total;
        valid |= ok ? 1u << g : 0u;
        ends |= end ? 1u << g : 0u;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            const int col = 16 * c + li;
            r[c][g] = (!end && col < n) ? gam[(e + 1) * n + col] : 0.0;
        }
    }

    // slab 0 into LDS
    double st[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u)
        sB[0][tid + TPB * u] = Bop[tid + TPB * u];
    __syncthreads();

    pair_v4d rden; // after m == 0: 1 / sum_j P_j r_j of rows lk + 4 g
    const int S = nm * NT;
    for (int m = 0; m < nm; ++m) {
        pair_v4d part = {0.0, 0.0, 0.0, 0.0}; // this lane's share of the sum over j
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            const int s = m * NT + c;
            const bool more = s + 1 < S; // (uniform)
            if (more) {
#pragma unroll
                for (int u = 0; u < PER; ++u)
                    st[u] = Bop[(int64_t)(s + 1) * SLAB + tid + TPB * u];
            }
            const double *sb = sB[s & 1];
            pair_v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(F[kk], sb[kk * 64 + lane], acc, 0, 0, 0);
            if (m == 0) { // P: r = gamma / P where the model enters the state at all
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const double P = acc[g];
                    const double rr = P > 0.0 ? r[c][g] / P : 0.0;
                    r[c][g] = rr;
                    part[g] += P * rr;
                }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    part[g] += acc[g] * r[c][g];
            }
            if (more) {
                double *sn = sB[(s + 1) & 1]; // (last read before the barrier that ended slab s - 1)
#pragma unroll
                for (int u = 0; u < PER; ++u)
                    sn[tid + TPB * u] = st[u];
            }
            __syncthreads();
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const double sum = pair_row16_sum(part[g]);
            if (m == 0) {
                rden[g] = 1.0 / sum; // (a trajectory of probability zero: NaN rows, as k_pair_rows)
            } else if (li == 0 && (valid >> g & 1u)) {
                const int64_t e = e0 + lk + 4 * g;
                out[e * Qp + (m - 1)] = (ends >> g & 1u) ? (OT)0.0 : (OT)(sum * rden[g]);
            }
        }
    }
}

} // namespace bhmm
