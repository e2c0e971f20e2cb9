// runs_host.hpp -- the index arithmetic of bhmm_path_runs / bhmm_decode_runs (runs_api.hip, runs_kernels.hpp;
// DESIGN.md section 19) as plain functions: no HIP, no context, so that a stand-alone host program can exercise them.
#pragma once
#include <stdint.h>

namespace bhmm {
namespace runs {

constexpr int LANE = 16;            // steps per lane: one 16-byte load of a byte path, four of an int32 path
constexpr int THREADS = 256;        // lanes per workgroup
constexpr int TILE = LANE * THREADS; // steps per workgroup (option runs_tile)
constexpr int SCAN_PER_THREAD = 4;  // tile counts per lane of the scan's first pass
constexpr int SCAN_BLOCK = THREADS * SCAN_PER_THREAD; // ... per workgroup
// statistics tables up to this many states are summed in LDS per workgroup first (n * 5 + n * n words of 8 bytes)
constexpr int STATS_LDS_MAX_N = 32;

// tiles of a path of `total` steps
inline int64_t num_tiles(int64_t total) { return (total + TILE - 1) / TILE; }
// workgroups of the scan's first pass over `ntiles` counts
inline int64_t num_scan_blocks(int64_t ntiles) { return (ntiles + SCAN_BLOCK - 1) / SCAN_BLOCK; }

// tile_traj[i], i < ntiles: the trajectory that holds the first step of tile i -- the last k < K with
// offsets[k] <= i * TILE, so never an empty one; tile_traj[ntiles] = K - 1.  The trajectories with a step in tile i
// are tile_traj[i] .. tile_traj[i + 1].  One merge over offsets and tiles, made once per observation set.
inline void tile_trajectories(const int64_t *offsets, int K, int64_t ntiles, int32_t *tile_traj)
{
    int k = 0;
    for (int64_t i = 0; i < ntiles; ++i) {
        const int64_t t0 = i * TILE;
        while (k + 1 < K && offsets[k + 1] <= t0)
            ++k;
        tile_traj[i] = k;
    }
    tile_traj[ntiles] = K - 1;
}

// The scatter pass writes run_off[k] for every trajectory with at least one step.  This completes the table:
// run_off[K] = R, and an empty trajectory starts where the next one does (run_off[k + 1] == run_off[k]).
inline void fill_empty(int64_t *run_off, const int64_t *offsets, int K, int64_t R)
{
    run_off[K] = R;
    for (int k = K - 1; k >= 0; --k)
        if (offsets[k + 1] == offsets[k])
            run_off[k] = run_off[k + 1];
}

// bytes the run buffers need for R runs (start, length: int64; state: int32)
inline uint64_t run_bytes(int64_t R) { return (uint64_t)R * (2 * sizeof(int64_t) + sizeof(int32_t)); }

} // namespace runs
} // namespace bhmm
