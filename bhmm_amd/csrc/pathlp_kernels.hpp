// pathlp_kernels.hpp -- joint log-probability log p(s, O | model) of given hidden paths (bhmm_path_logprob,
// bhmm_decode_logprob; pathlp_api.hip).
//
//   L[m, k] = log pi(s_0) + e(s_0, o_0) + sum_{t >= 1} [ log A(s_{t-1}, s_t) + e(s_t, o_t) ]
//
// Every term is formed in log space: gaussian e(i, o) = -((o - mu_i) / sigma_i)^2 / 2 - log sigma_i - log(2 pi) / 2
// (the density is never exponentiated), discrete e(i, o) = log B[i, o], explicit e(i, t) = log pobs[t, i].  The
// gaussian outlier rule of the recursions -- an emission row that underflowed to all zeros counts as all ones -- is
// deliberately NOT applied: an outlier gives a very negative finite term.  log 0 = -inf makes that trajectory's
// result -inf, a NaN observation makes it NaN; neither reaches another trajectory (the segmented sums select, they
// never multiply by a flag).
//
// The path is tiled as for bhmm_path_runs (runs_device.hpp: the same TILE, LANE, tile_traj table, load_span and start bitmap): a
// workgroup owns TILE consecutive flat steps, a lane LANE consecutive steps with the matching observations in
// registers (16-byte loads) and the state before its span from one extra load.  Per model -- its log tables staged
// in LDS up to TABLE_MAX_N states, gathered through L2 above -- a lane adds its terms serially and cuts the sum at
// every trajectory start in its span:
//   a piece between two starts inside one lane is a whole trajectory's share of the tile: the lane writes it;
//   the piece before the lane's first start (head) and the one from its last start on (tail; a lane without a start
//   passes its sum on) go through a segmented scan over the lanes in a fixed order -- Hillis-Steele inside the
//   wavefront, the wavefronts in ascending order through LDS; the lane with the start adds its head to what arrives
//   and writes the share of the trajectory that ends there, the last lane writes the tile's open share.
// So a tile writes one partial per (model, trajectory with a step in it): slot tile + trajectory - trajectory of step
// 0, each written exactly once, nothing to clear.  k_pathlp_finish adds the partials of the tiles a trajectory spans
// in ascending tile order.  No floating-point atomics anywhere: the result is bitwise the same from call to call.
//
//   k_pathlp_prepare   once per call: log A, log pi and log B or (mu, 1 / sigma, -log sigma - log(2 pi) / 2) per model
//   k_pathlp_tiles     the pass over path and observations, all models; a state outside [0, n) sets the status word
//                      and is replaced by state 0 before anything is indexed by it
//   k_pathlp_finish    one wavefront per (model, trajectory)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "host_common.hpp"
#include "runs_device.hpp"

namespace bhmm {
namespace pathlp {

using runs::LANE;
using runs::THREADS;
using runs::TILE;
using runs::WAVES;

constexpr unsigned int STATUS_BAD_STATE = 1u;
// Up to this many states a model's log A and log pi (32.5 KiB) and the gaussian constants sit in LDS; above, and
// always above it, every log A entry is a gather through L2
constexpr int TABLE_MAX_N = 64;
// ... and a discrete model's log B with them up to this many entries (24 KiB), through L2 above
constexpr int TABLE_MAX_B = 3072;

// doubles of one model's tables: log A [n * n], log pi [n], then gaussian mu, 1 / sigma, c [n each] or discrete
// log B [n * M]
__host__ __device__ inline size_t model_stride(int kind, int n, int M)
{
    return (size_t)n * n + n + (kind == EMIT_GAUSS ? 3 * (size_t)n : kind == EMIT_DISC ? (size_t)n * M : 0);
}
// bytes of LDS k_pathlp_tiles needs: the staged tables in front, then the start bitmap and the scan's words
inline size_t tiles_lds(size_t table_doubles)
{
    return table_doubles * sizeof(double) + (TILE / 32) * sizeof(unsigned int) + WAVES * sizeof(double) +
           WAVES * sizeof(int);
}

// raw: the caller's stacked models [A S*n*n | pi S*n | par0 | par1]; tab: [S][model_stride]
__global__ __launch_bounds__(256) void k_pathlp_prepare(const double *__restrict__ raw, int S, int n, int M, int kind,
                                                        double *__restrict__ tab)
{
    const size_t nn = (size_t)n * n;
    const size_t ne = kind == EMIT_GAUSS ? 3 * (size_t)n : kind == EMIT_DISC ? (size_t)n * M : 0;
    const size_t stride = nn + n + ne;
    const double *A = raw, *pi = A + (size_t)S * nn, *p0 = pi + (size_t)S * n;
    const double *p1 = p0 + (size_t)S * n; // (gaussian only)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)S * stride;
         i += (size_t)gridDim.x * blockDim.x) {
        const size_t s = i / stride, r = i - s * stride;
        double v;
        if (r < nn) {
            v = log(A[s * nn + r]);
        } else if (r < nn + n) {
            v = log(pi[s * n + (r - nn)]);
        } else if (kind == EMIT_DISC) {
            v = log(p0[s * ne + (r - nn - n)]);
        } else {
            const size_t q = r - nn - n, j = q % n;
            const double sg = p1[s * n + j];
            v = q < (size_t)n ? p0[s * n + j] : q < 2 * (size_t)n ? 1.0 / sg : -log(sg) - 0.5 * log(2.0 * M_PI);
        }
        tab[i] = v;
    }
}

// the LANE observations from step p0 on (zero behind the path's end)
__device__ inline void load_obs(const double *__restrict__ obs, int64_t p0, int64_t total, double (&o)[LANE])
{
    if (p0 + LANE <= total) {
#pragma unroll
        for (int q = 0; q < LANE / 2; ++q) {
            const double2 x = *reinterpret_cast<const double2 *>(obs + p0 + 2 * q);
            o[2 * q] = x.x;
            o[2 * q + 1] = x.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < LANE; ++j)
            o[j] = p0 + j < total ? obs[p0 + j] : 0.0;
    }
}

__device__ inline void load_obs(const int32_t *__restrict__ obs, int64_t p0, int64_t total, int (&o)[LANE])
{
    if (p0 + LANE <= total) {
#pragma unroll
        for (int q = 0; q < LANE / 4; ++q) {
            const int4 x = *reinterpret_cast<const int4 *>(obs + p0 + 4 * q);
            o[4 * q + 0] = x.x;
            o[4 * q + 1] = x.y;
            o[4 * q + 2] = x.z;
            o[4 * q + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < LANE; ++j)
            o[j] = p0 + j < total ? obs[p0 + j] : 0;
    }
}

// PT: uint8_t / int32_t path; KIND: emission kind; TAB: the model's tables are staged in LDS (n <= TABLE_MAX_N; b_lds:
// a discrete model's log B as well), else read through L2.  part: [S][nslots], slot = tile + trajectory - traj0.
template <typename PT, int KIND, bool TAB>
__global__ __launch_bounds__(THREADS) void k_pathlp_tiles(const PT *__restrict__ path, const void *__restrict__ obs_v,
                                                          int64_t total, const int64_t *__restrict__ off, int K,
                                                          const int32_t *__restrict__ tile_traj, int n, int M, int S,
                                                          const double *__restrict__ tab, int b_lds, int traj0,
                                                          int64_t nslots, double *__restrict__ part,
                                                          unsigned int *status)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t stride = model_stride(KIND, n, M);
    const size_t staged = TAB ? (size_t)n * n + n + (KIND == EMIT_GAUSS ? 3 * (size_t)n : b_lds ? (size_t)n * M : 0) : 0;
    double *s_tab = reinterpret_cast<double *>(smem);
    double *s_wv = s_tab + staged;
    unsigned int *bm = reinterpret_cast<unsigned int *>(s_wv + WAVES);
    int *s_wf = reinterpret_cast<int *>(bm + TILE / 32);

    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    const int64_t tend = t0 + TILE < total ? t0 + TILE : total;
    const int64_t p0 = t0 + (int64_t)threadIdx.x * LANE;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool active = p0 < total;

    // the lane's states and observations, in registers for every model (the loads fly while the bitmap is made)
    int v[LANE], prev = 0;
    double og[KIND == EMIT_GAUSS ? LANE : 1];
    int od[KIND == EMIT_DISC ? LANE : 1];
    if (active) {
        runs::load_span(path, p0, total, v, prev);
        if constexpr (KIND == EMIT_GAUSS)
            load_obs(static_cast<const double *>(obs_v), p0, total, og);
        if constexpr (KIND == EMIT_DISC)
            load_obs(static_cast<const int32_t *>(obs_v), p0, total, od);
    } else {
#pragma unroll
        for (int j = 0; j < LANE; ++j)
            v[j] = 0;
    }
    const int klo = tile_traj[blockIdx.x], khi = tile_traj[blockIdx.x + 1];
    runs::tile_starts(off, K, klo, t0, tend, bm);

    // a state outside [0, n): flagged, and state 0 stands in for it before anything is indexed
    bool bad = false;
#pragma unroll
    for (int j = 0; j < LANE; ++j) {
        const bool b = (unsigned int)v[j] >= (unsigned int)n;
        bad = bad || (b && p0 + j < total);
        v[j] = b ? 0 : v[j];
    }
    if ((unsigned int)prev >= (unsigned int)n) // (the lane that owns that step flags it)
        prev = 0;
    if (__ballot(bad) != 0ull && lane == 0)
        atomicOr(status, STATUS_BAD_STATE);

    const int64_t left = total - p0;
    const unsigned int valid = !active ? 0u : left >= LANE ? 0xffffu : ((1u << (int)left) - 1u);
    const unsigned int first = (bm[threadIdx.x >> 1] >> (16 * (threadIdx.x & 1))) & 0xffffu & valid;
    // the trajectory whose share ends at the lane's first start (none when that is the tile's first step), the one
    // that begins there, and for the last lane the one that holds the tile's last step
    int64_t slot_end = -1;
    int kfirst = klo;
    if (first) {
        const int64_t t = p0 + (__ffs(first) - 1);
        if (t > t0)
            slot_end = (int64_t)blockIdx.x + runs::traj_of(off, klo, khi, t - 1) - traj0;
        kfirst = runs::traj_of(off, klo, khi, t);
    }
    int64_t slot_open = -1;
    if (threadIdx.x == THREADS - 1)
        slot_open = (int64_t)blockIdx.x + runs::traj_of(off, klo, khi, tend - 1) - traj0;

    for (int s = 0; s < S; ++s) {
        const double *g = tab + (size_t)s * stride;
        if (TAB) {
            __syncthreads(); // (the model before has been read)
            for (size_t i = threadIdx.x; i < staged; i += THREADS)
                s_tab[i] = g[i];
            __syncthreads();
        }
        const double *lA = TAB ? s_tab : g;
        const double *lpi = lA + (size_t)n * n;
        const double *em = lpi + n;                                  // gaussian: mu | 1 / sigma | c; discrete: log B
        const double *emB = (TAB && b_lds) ? em : g + (size_t)n * n + n; // (discrete)
        double *out = part + (size_t)s * nslots;

        double acc = 0.0, head = 0.0;
        bool seen = false;
        int kcur = kfirst;
        if (active) {
#pragma unroll
            for (int j = 0; j < LANE; ++j) {
                if (!((valid >> j) & 1u))
                    continue;
                const int st = v[j];
                double e;
                if constexpr (KIND == EMIT_GAUSS) {
                    const double z = (og[j] - em[st]) * em[n + st];
                    e = -0.5 * (z * z) + em[2 * n + st];
                } else if constexpr (KIND == EMIT_DISC) {
                    const int sym = od[j];
                    // (a symbol outside the alphabet has probability zero)
                    e = (unsigned int)sym < (unsigned int)M ? emB[(size_t)st * M + sym] : -INFINITY;
                } else {
                    e = log(static_cast<const double *>(obs_v)[(size_t)(p0 + j) * n + st]);
                }
                if ((first >> j) & 1u) {
                    if (!seen) {
                        head = acc;
                        seen = true;
                    } else { // a whole trajectory's share inside this lane
                        out[(int64_t)blockIdx.x + kcur - traj0] = acc;
                        kcur = runs::traj_of(off, kcur, khi, p0 + j);
                    }
                    acc = lpi[st] + e;
                } else {
                    const int from = j == 0 ? prev : v[j > 0 ? j - 1 : 0];
                    acc += lA[(size_t)from * n + st] + e;
                }
            }
        }
        if (!seen) {
            head = acc;
            acc = 0.0;
        }
        // segmented inclusive scan of (seen, seen ? tail : head) over the lanes: (f, x)
        int f = seen ? 1 : 0;
        double x = seen ? acc : head;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int yf = __shfl_up(f, d);
            const double yx = __shfl_up(x, d);
            if (lane >= d) {
                x = f ? x : yx + x;
                f |= yf;
            }
        }
        if (lane == 63) {
            s_wf[w] = f;
            s_wv[w] = x;
        }
        int ef = __shfl_up(f, 1); // the wavefront's scan up to the lane before (lane 0: nothing, 0.0)
        double ex = __shfl_up(x, 1);
        if (lane == 0) {
            ef = 0;
            ex = 0.0;
        }
        __syncthreads();
        double px = 0.0; // the wavefronts before, in ascending order (0.0 + y is y)
#pragma unroll
        for (int i = 0; i < WAVES; ++i)
            if (i < w)
                px = s_wf[i] ? s_wv[i] : px + s_wv[i];
        // what arrives at this lane: the open sum since the last start before it in the tile
        const double carry = ef ? ex : px + ex;
        if (seen && slot_end >= 0)
            out[slot_end] = carry + head;
        if (threadIdx.x == THREADS - 1) // the tile's last, open share
            out[slot_open] = f ? x : px + x;
        __syncthreads(); // (s_wf / s_wv are written again for the next model)
    }
}

// logp[s * K + k]: the partials of the tiles trajectory k spans, added in ascending tile order; one wavefront each
__global__ __launch_bounds__(THREADS) void k_pathlp_finish(const double *__restrict__ part, int64_t nslots,
                                                           const int64_t *__restrict__ off, int K, int S, int traj0,
                                                           double *__restrict__ logp)
{
    const int lane = threadIdx.x & 63;
    const int64_t id = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (id >= (int64_t)S * K)
        return;
    const int s = (int)(id / K), k = (int)(id - (int64_t)s * K);
    const int64_t a = off[k], b = off[k + 1];
    double acc = 0.0; // (an empty trajectory)
    if (b > a) {
        const int64_t i0 = a / TILE, i1 = (b - 1) / TILE;
        const double *p = part + (size_t)s * nslots + (k - traj0);
        for (int64_t c0 = i0; c0 <= i1; c0 += 64) {
            const int cnt = (int)(i1 - c0 + 1 < 64 ? i1 - c0 + 1 : 64);
            const double x = lane < cnt ? p[c0 + lane] : 0.0;
            for (int j = 0; j < cnt; ++j) {
                const double y = __shfl(x, j);
                acc = (c0 == i0 && j == 0) ? y : acc + y;
            }
        }
    }
    if (lane == 0)
        logp[id] = acc;
}

} // namespace pathlp
} // namespace bhmm
