// runs_device.hpp -- the device helpers of the flat path tiling (runs_host.hpp) that more than one kernel family
// uses: the kernels of runs_kernels.hpp (bhmm_path_runs) and of pathlp_kernels.hpp (bhmm_path_logprob).
//
// The path is flat and trajectory-concatenated, one uint8_t or int32_t per step, its base aligned to 16 bytes.  A
// workgroup of THREADS lanes owns a tile of TILE consecutive flat steps, a lane LANE consecutive steps of it: one
// 16-byte load of a byte path, four of an int32 path, a guarded element-wise tail where the path ends inside the
// lane's span, and the one element before the span.  The trajectory starts inside the tile come from the device copy
// of the offsets into a bitmap in LDS, beginning at the trajectory of the tile's first step (tile_traj, made on the
// host once per observation set: runs_host.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "runs_host.hpp"

namespace bhmm {
namespace runs {

constexpr int WAVES = THREADS / 64;

// the last k in [lo, hi] with off[k] <= t (off[lo] <= t)
__device__ inline int traj_of(const int64_t *__restrict__ off, int lo, int hi, int64_t t)
{
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= t)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// the LANE steps from p0 on (p0 < total; zero behind the path's end) and the step before them (-1 at p0 == 0)
__device__ inline void load_span(const uint8_t *__restrict__ path, int64_t p0, int64_t total, int (&v)[LANE], int &prev)
{
    if (p0 + LANE <= total) {
        const uint4 q = *reinterpret_cast<const uint4 *>(path + p0);
        const unsigned int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < LANE; ++j)
            v[j] = (int)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
    } else {
#pragma unroll
        for (int j = 0; j < LANE; ++j)
            v[j] = p0 + j < total ? (int)path[p0 + j] : 0;
    }
    prev = p0 > 0 ? (int)path[p0 - 1] : -1;
}

__device__ inline void load_span(const int32_t *__restrict__ path, int64_t p0, int64_t total, int (&v)[LANE], int &prev)
{
    if (p0 + LANE <= total) {
#pragma unroll
        for (int q4 = 0; q4 < LANE / 4; ++q4) {
            const int4 q = *reinterpret_cast<const int4 *>(path + p0 + 4 * q4);
            v[4 * q4 + 0] = q.x;
            v[4 * q4 + 1] = q.y;
            v[4 * q4 + 2] = q.z;
            v[4 * q4 + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < LANE; ++j)
            v[j] = p0 + j < total ? path[p0 + j] : 0;
    }
    prev = p0 > 0 ? path[p0 - 1] : -1;
}

// Trajectory starts of the tile [t0, tend) into the bitmap bm (TILE / 32 words, bit p - t0); klo: the trajectory
// that holds step t0.  Empty trajectories share their offset with the next one: the same bit.
__device__ inline void tile_starts(const int64_t *__restrict__ off, int K, int klo, int64_t t0, int64_t tend,
                                   unsigned int *bm)
{
    for (int i = threadIdx.x; i < TILE / 32; i += THREADS)
        bm[i] = 0u;
    __syncthreads();
    for (int64_t k = (int64_t)klo + threadIdx.x; k < K; k += THREADS) {
        const int64_t o = off[k];
        if (o >= tend)
            break;
        if (o >= t0)
            atomicOr(&bm[(o - t0) >> 5], 1u << ((o - t0) & 31));
    }
    __syncthreads();
}

} // namespace runs
} // namespace bhmm
