// runs_kernels.hpp -- dwell segments (runs) of a decoded path, compacted on the device (bhmm_path_runs,
// bhmm_decode_runs; runs_api.hip).
//
// The path is flat and trajectory-concatenated, one uint8_t or int32_t per step, its base aligned to 16 bytes.  A
// workgroup of THREADS lanes owns a tile of TILE consecutive flat steps, a lane LANE consecutive steps of it: one
// 16-byte load of a byte path, four of an int32 path, a guarded element-wise tail where the path ends inside the
// lane's span, and the one element before the span for the first comparison.  The trajectory starts inside the tile
// come from the device copy of the offsets into a bitmap in LDS, beginning at the trajectory of the tile's first step
// (tile_traj, made on the host once per observation set: runs_host.hpp).  Both passes form the same 16 flags per lane from
// that; nothing on the per-step path depends on the data for its address.  (The loads, the bitmap and the trajectory
// search are in runs_device.hpp: pathlp_kernels.hpp uses them as well.)
//
//   k_runs_count        flags -> the tile's run count; a state outside [0, n) sets the status word
//   k_runs_scan_tiles   exclusive sum of SCAN_BLOCK tile counts per workgroup, and the workgroup's total
//   k_runs_scan_blocks  one workgroup: exclusive sum of those totals in place, R behind them
//   k_runs_scatter      flags again, ranked inside the tile (a lane's flags by popcount, lanes by a shuffle scan
//                       inside the wave, waves through LDS): start, state, the END of the run before, run_off
//   k_runs_finish       over the R runs: length = end - start, and the statistics tables
//
// The scan is three plain launches: no workgroup ever waits for another one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "runs_device.hpp"
#include "runs_host.hpp"

namespace bhmm {
namespace runs {

constexpr unsigned int STATUS_BAD_STATE = 1u;

// exclusive sum of x over the workgroup (THREADS lanes); *total: the sum.  s_w: WAVES words of LDS.
template <typename T>
__device__ inline T block_excl_scan(T x, T *s_w, T *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(inc, d);
        if (lane >= d)
            inc += y;
    }
    if (lane == 63)
        s_w[w] = inc;
    __syncthreads();
    T woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        const T s = s_w[i];
        woff += i < w ? s : (T)0;
        tot += s;
    }
    __syncthreads(); // (s_w may be written again)
    *total = tot;
    return woff + inc - x;
}

// bit j: a run begins at step p0 + j (first step of a trajectory, or another state than the step before)
__device__ inline unsigned int lane_flags(const int (&v)[LANE], int prev, int64_t p0, int64_t total,
                                          const unsigned int *bm)
{
    const int64_t left = total - p0;
    const unsigned int valid = left >= LANE ? 0xffffu : ((1u << (int)left) - 1u);
    unsigned int f = (bm[threadIdx.x >> 1] >> (16 * (threadIdx.x & 1))) & 0xffffu;
    int last = prev;
#pragma unroll
    for (int j = 0; j < LANE; ++j) {
        f |= v[j] != last ? 1u << j : 0u;
        last = v[j];
    }
    return f & valid;
}

template <typename PT>
__global__ __launch_bounds__(THREADS) void k_runs_count(const PT *__restrict__ path, int64_t total,
                                                        const int64_t *__restrict__ off, int K,
                                                        const int32_t *__restrict__ tile_traj, int n,
                                                        int32_t *__restrict__ tile_cnt, unsigned int *status)
{
    __shared__ unsigned int bm[TILE / 32];
    __shared__ int s_w[WAVES];
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    const int64_t tend = t0 + TILE < total ? t0 + TILE : total;
    const int64_t p0 = t0 + (int64_t)threadIdx.x * LANE;
    int v[LANE], prev = 0;
    if (p0 < total) // (the loads are in flight while the bitmap is made)
        load_span(path, p0, total, v, prev);
    tile_starts(off, K, tile_traj[blockIdx.x], t0, tend, bm);
    int cnt = 0;
    bool bad = false;
    if (p0 < total) {
        cnt = __popc(lane_flags(v, prev, p0, total, bm));
#pragma unroll
        for (int j = 0; j < LANE; ++j) // (the zeros behind the path's end are states)
            bad = bad || (unsigned int)v[j] >= (unsigned int)n;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0)
        atomicOr(status, STATUS_BAD_STATE);
    int tot;
    (void)block_excl_scan<int>(cnt, s_w, &tot);
    if (threadIdx.x == 0)
        tile_cnt[blockIdx.x] = tot;
}

// tile_off[i]: runs of the tiles of this workgroup before tile i; blk[b]: runs of workgroup b's tiles
__global__ __launch_bounds__(THREADS) void k_runs_scan_tiles(const int32_t *__restrict__ tile_cnt, int64_t ntiles,
                                                             int64_t *__restrict__ tile_off, int64_t *__restrict__ blk)
{
    __shared__ int s_w[WAVES];
    const int64_t i0 = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_PER_THREAD;
    int x[SCAN_PER_THREAD], sum = 0;
#pragma unroll
    for (int j = 0; j < SCAN_PER_THREAD; ++j) {
        x[j] = i0 + j < ntiles ? tile_cnt[i0 + j] : 0;
        sum += x[j];
    }
    int tot;
    int run = block_excl_scan<int>(sum, s_w, &tot); // (at most SCAN_BLOCK * TILE = 2^22)
#pragma unroll
    for (int j = 0; j < SCAN_PER_THREAD; ++j) {
        if (i0 + j < ntiles)
            tile_off[i0 + j] = run;
        run += x[j];
    }
    if (threadIdx.x == 0)
        blk[blockIdx.x] = tot;
}

// one workgroup: blk[0 .. nb) becomes its exclusive sum, blk[nb] the number of runs
__global__ __launch_bounds__(THREADS) void k_runs_scan_blocks(int64_t *blk, int64_t nb)
{
    __shared__ long long s_w[WAVES];
    long long carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += THREADS) {
        const int64_t i = b0 + threadIdx.x;
        const long long x = i < nb ? (long long)blk[i] : 0ll;
        long long tot;
        const long long ex = block_excl_scan<long long>(x, s_w, &tot);
        if (i < nb)
            blk[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0)
        blk[nb] = carry;
}

// Run r begins at flat step t of trajectory k: start[r] = t - off[k], state[r]; the run before ends there (at its
// trajectory's end if t is a trajectory's first step): ends[r - 1], in steps from its trajectory's first one.  The
// lane that holds the last step writes ends[R - 1].  run_off[k] = r for every trajectory with a step.
template <typename PT>
__global__ __launch_bounds__(THREADS) void k_runs_scatter(const PT *__restrict__ path, int64_t total,
                                                          const int64_t *__restrict__ off, int K,
                                                          const int32_t *__restrict__ tile_traj,
                                                          const int64_t *__restrict__ tile_off,
                                                          const int64_t *__restrict__ blk, int64_t R,
                                                          int64_t *__restrict__ start, int64_t *__restrict__ ends,
                                                          int32_t *__restrict__ state, int64_t *__restrict__ run_off)
{
    __shared__ unsigned int bm[TILE / 32];
    __shared__ int s_w[WAVES];
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    const int64_t tend = t0 + TILE < total ? t0 + TILE : total;
    const int64_t p0 = t0 + (int64_t)threadIdx.x * LANE;
    int v[LANE], prev = 0;
    if (p0 < total)
        load_span(path, p0, total, v, prev);
    const int klo = tile_traj[blockIdx.x], khi = tile_traj[blockIdx.x + 1]; // the trajectories with a step in the tile
    tile_starts(off, K, klo, t0, tend, bm);
    const unsigned int f = p0 < total ? lane_flags(v, prev, p0, total, bm) : 0u;
    int tot;
    const int ex = block_excl_scan<int>(__popc(f), s_w, &tot);
    if (f) {
        const unsigned int first = (bm[threadIdx.x >> 1] >> (16 * (threadIdx.x & 1))) & 0xffffu;
        int64_t r = tile_off[blockIdx.x] + blk[blockIdx.x / SCAN_BLOCK] + ex;
        int k = traj_of(off, klo, khi, p0);
#pragma unroll
        for (int j = 0; j < LANE; ++j) {
            if (!((f >> j) & 1u) || r >= R) // (r < R unless the path changed under the two passes: nothing out of bounds)
                continue;
            const int64_t t = p0 + j;
            if ((first >> j) & 1u) {
                while (k + 1 < K && off[k + 1] <= t) // (on to the trajectory that begins at t, past empty ones)
                    ++k;
                run_off[k] = r;
                if (r > 0) // (t >= 1; the trajectory of step t - 1 lies before k)
                    ends[r - 1] = t - off[traj_of(off, 0, k - 1, t - 1)];
            } else {
                ends[r - 1] = t - off[k];
            }
            start[r] = t - off[k];
            state[r] = v[j];
            ++r;
        }
    }
    if (p0 < total && total - 1 < p0 + LANE)
        ends[R - 1] = total - off[traj_of(off, 0, K - 1, total - 1)];
}

// dwell[i][5]: runs in state i, their steps, the longest, the runs that touch the first or the last step of their
// trajectory, their steps; jumps[i][j]: run pairs i -> j inside one trajectory.  Up to STATS_LDS_MAX_N states the
// tables are summed in LDS (lds != 0: n * 5 + n * n words) and reach global memory once per workgroup.
__device__ inline void stats_add(unsigned long long *dwell, unsigned long long *jumps, int n, int st, long long len,
                                 bool censored, int next)
{
    atomicAdd(&dwell[st * 5 + 0], 1ull);
    atomicAdd(&dwell[st * 5 + 1], (unsigned long long)len);
    atomicMax(&dwell[st * 5 + 2], (unsigned long long)len);
    if (censored) {
        atomicAdd(&dwell[st * 5 + 3], 1ull);
        atomicAdd(&dwell[st * 5 + 4], (unsigned long long)len);
    }
    if (next >= 0)
        atomicAdd(&jumps[(size_t)st * n + next], 1ull);
}

__global__ __launch_bounds__(THREADS) void k_runs_finish(const int64_t *__restrict__ start, int64_t *length,
                                                         const int32_t *__restrict__ state, int64_t R, int n,
                                                         unsigned long long *dwell, unsigned long long *jumps, int lds)
{
    extern __shared__ unsigned long long s_tab[];
    const int words = n * 5 + n * n;
    if (dwell && lds) {
        for (int i = threadIdx.x; i < words; i += THREADS)
            s_tab[i] = 0ull;
        __syncthreads();
    }
    for (int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * THREADS) {
        const int64_t s = start[r];
        const int64_t len = length[r] - s; // (the scatter pass left the run's end there)
        length[r] = len;
        if (dwell) {
            const bool last = r + 1 == R || start[r + 1] == 0; // the last run of its trajectory
            const int next = last ? -1 : state[r + 1];
            if (lds)
                stats_add(s_tab, s_tab + n * 5, n, state[r], len, s == 0 || last, next);
            else
                stats_add(dwell, jumps, n, state[r], len, s == 0 || last, next);
        }
    }
    if (dwell && lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < words; i += THREADS) {
            const unsigned long long x = s_tab[i];
            if (x == 0ull)
                continue;
            if (i < n * 5) {
                if (i % 5 == 2)
                    atomicMax(&dwell[i], x);
                else
                    atomicAdd(&dwell[i], x);
            } else {
                atomicAdd(&jumps[i - n * 5], x);
            }
        }
    }
}

} // namespace runs
} // namespace bhmm
