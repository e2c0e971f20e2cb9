// runs_api.hip -- bhmm_path_runs, bhmm_decode_runs, bhmm_runs_fetch: the dwell segments (runs) of a decoded path,
// compacted on the device so that only the runs cross the link.  Kernels in runs_kernels.hpp, the index arithmetic in
// runs_host.hpp; DESIGN.md section 19.
//
// One call: (once per observation set: the trajectory of every tile's first step, from the offsets, to the device;)
// count pass over the tiles of the path, three-launch scan of the tile counts, R and the status word to
// the host (a state outside [0, n): BHMM_ERR_INVALID, nothing else runs), the run buffers sized from R, scatter
// pass, k_runs_finish over the runs (lengths and, when asked for, the statistics tables).  The buffers are c->runs.*,
// the only other fields touched are ds.runs_valid / runs_count and last.runs_ms; bhmm_decode_runs decodes through
// the existing entry points first (bhmm_viterbi_batch_u8 into c->runs.path, post_decode_device into c->post.path),
// with everything those do to the context.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_internal.hpp"
#include "launch.hpp"
#include "runs_host.hpp"
#include "runs_kernels.hpp"

namespace bhmm {
namespace {

using namespace runs;

template <typename PT>
int compact_t(bhmm_ctx *c, const PT *path, int64_t *run_off, int64_t *dwell, int64_t *jumps)
{
    auto &b = c->runs;
    const int K = c->K, n = c->n;
    const int64_t total = c->total;
    const int64_t ntiles = num_tiles(total), nb = num_scan_blocks(ntiles);
    const bool stats = dwell || jumps;
    const size_t words = (size_t)n * BHMM_DWELL_COLS + (size_t)n * n;
    c->ds.runs_valid = false;
    c->ds.runs_count = 0;
    c->last.runs_ms = 0.f;
    if (ntiles > 0x7fffffff)
        return invalid_arg("bhmm_path_runs: the path has more tiles than a grid has workgroups");
    int rc;
    if ((rc = b.tile_cnt.ensure(ntiles)) || (rc = b.tile_off.ensure(ntiles)) || (rc = b.blk.ensure(nb + 1)) ||
        (rc = b.status.ensure(1)) || (rc = b.run_off.ensure(K + 1)) || (stats && (rc = b.tables.ensure(words))))
        return rc;
    if (!c->ds.runs_tiles_ready) { // the trajectory of every tile's first step: once per observation set
        std::vector<int32_t> tt((size_t)ntiles + 1);
        tile_trajectories(c->offsets.data(), K, ntiles, tt.data());
        if ((rc = b.tile_traj.ensure(tt.size())))
            return rc;
        BHMM_HIP(hipMemcpyAsync(b.tile_traj.p, tt.data(), tt.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (tt is a temporary)
        c->ds.runs_tiles_ready = true;
    }
    for (hipEvent_t &e : b.ev)
        if (!e)
            BHMM_HIP(hipEventCreate(&e));
    BHMM_HIP(hipMemsetAsync(b.status.p, 0, sizeof(unsigned int), c->stream));
    BHMM_HIP(hipEventRecord(b.ev[0], c->stream));
    BHMM_HIP(launch(k_runs_count<PT>, dim3((unsigned)ntiles), dim3(THREADS), 0, c->stream, path, total, c->d_offsets.p,
                    K, b.tile_traj.p, n, b.tile_cnt.p, b.status.p));
    BHMM_HIP(launch(k_runs_scan_tiles, dim3((unsigned)nb), dim3(THREADS), 0, c->stream, b.tile_cnt.p, ntiles,
                    b.tile_off.p, b.blk.p));
    BHMM_HIP(launch(k_runs_scan_blocks, dim3(1), dim3(THREADS), 0, c->stream, b.blk.p, nb));
    BHMM_HIP(hipEventRecord(b.ev[1], c->stream));
    int64_t R = 0;
    unsigned int status = 0;
    BHMM_HIP(hipMemcpyAsync(&R, b.blk.p + nb, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipMemcpyAsync(&status, b.status.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    if (status & STATUS_BAD_STATE)
        return invalid_arg("bhmm_path_runs: the path holds a state outside [0, " + std::to_string(n) + ")");
    if (R < 1 || R > total)
        return invalid_arg("bhmm_path_runs: inconsistent run count (was the path written during the call?)");
    // the runs: sized from R, never from the number of steps
    if ((rc = b.start.ensure(R)) || (rc = b.length.ensure(R)) || (rc = b.state.ensure(R)))
        return rc;
    if (stats)
        BHMM_HIP(hipMemsetAsync(b.tables.p, 0, words * sizeof(unsigned long long), c->stream));
    BHMM_HIP(hipEventRecord(b.ev[2], c->stream));
    BHMM_HIP(launch(k_runs_scatter<PT>, dim3((unsigned)ntiles), dim3(THREADS), 0, c->stream, path, total,
                    c->d_offsets.p, K, b.tile_traj.p, b.tile_off.p, b.blk.p, R, b.start.p, b.length.p, b.state.p, b.run_off.p));
    const bool lds = n <= STATS_LDS_MAX_N;
    const unsigned fin_grid = (unsigned)std::min<int64_t>((R + THREADS - 1) / THREADS, 4096);
    BHMM_HIP(launch(k_runs_finish, dim3(fin_grid), dim3(THREADS), stats && lds ? words * sizeof(unsigned long long) : 0,
                    c->stream, b.start.p, b.length.p, b.state.p, R, n, stats ? b.tables.p : nullptr,
                    stats ? b.tables.p + (size_t)n * BHMM_DWELL_COLS : nullptr, lds ? 1 : 0));
    BHMM_HIP(hipEventRecord(b.ev[3], c->stream));
    std::vector<unsigned long long> tab(stats ? words : 0);
    if (stats)
        BHMM_HIP(hipMemcpyAsync(tab.data(), b.tables.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                c->stream));
    BHMM_HIP(hipMemcpyAsync(run_off, b.run_off.p, (size_t)K * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    fill_empty(run_off, c->offsets.data(), K, R);
    if (dwell)
        for (size_t i = 0; i < (size_t)n * BHMM_DWELL_COLS; ++i)
            dwell[i] = (int64_t)tab[i];
    if (jumps)
        for (size_t i = 0; i < (size_t)n * n; ++i)
            jumps[i] = (int64_t)tab[(size_t)n * BHMM_DWELL_COLS + i];
    float ms0 = 0.f, ms1 = 0.f;
    (void)hipEventElapsedTime(&ms0, b.ev[0], b.ev[1]);
    (void)hipEventElapsedTime(&ms1, b.ev[2], b.ev[3]);
    c->last.runs_ms = ms0 + ms1;
    c->ds.runs_valid = true;
    c->ds.runs_count = R;
    return BHMM_OK;
}

int compact(bhmm_ctx *c, const void *path, int path_u8, int64_t *run_off, int64_t *dwell, int64_t *jumps)
{
    return path_u8 ? compact_t<uint8_t>(c, static_cast<const uint8_t *>(path), run_off, dwell, jumps)
                   : compact_t<int32_t>(c, static_cast<const int32_t *>(path), run_off, dwell, jumps);
}

} // namespace
} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_path_runs(bhmm_ctx *c, const void *paths, int path_u8, int paths_on_device, int64_t *run_off,
                   int64_t *dwell, int64_t *jumps)
{
    if (int rc = enter_model_call(c, paths && run_off, "bhmm_path_runs: paths / run_off == NULL", false, nullptr,
                                  nullptr))
        return rc;
    if (path_u8 && c->n > 256) // (every byte is a state then; the int32 form holds the others)
        return invalid_arg("bhmm_path_runs: one byte per step holds at most 256 states (use the int32 form)");
    if (paths_on_device) {
        if (reinterpret_cast<uintptr_t>(paths) % 16)
            return invalid_arg("bhmm_path_runs: a device path must be aligned to 16 bytes");
        return compact(c, paths, path_u8, run_off, dwell, jumps);
    }
    const size_t bytes = (size_t)c->total * (path_u8 ? sizeof(uint8_t) : sizeof(int32_t));
    c->ds.runs_valid = false;
    if (int rc = c->runs.path.ensure(bytes))
        return rc;
    BHMM_HIP(hipMemcpyAsync(c->runs.path.p, paths, bytes, hipMemcpyHostToDevice, c->stream));
    return compact(c, c->runs.path.p, path_u8, run_off, dwell, jumps);
}

int bhmm_decode_runs(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                     int method, int64_t *run_off, int64_t *dwell, int64_t *jumps)
{
    if (int rc = enter_model_call(c, A && pi && run_off, "bhmm_decode_runs: A / pi / run_off == NULL", true, par0, par1))
        return rc;
    if (method != 0 && method != 1)
        return invalid_arg("bhmm_decode_runs: method is 0 (Viterbi) or 1 (posterior decoding)");
    if (c->n > 256)
        return invalid_arg("bhmm_decode_runs: more than 256 states: decode with bhmm_viterbi_batch / "
                           "bhmm_posterior_decode and pass the int32 path to bhmm_path_runs");
    c->ds.runs_valid = false;
    const void *path;
    if (method == 0) {
        int rc;
        if ((rc = c->runs.path.ensure((size_t)c->total)) ||
            (rc = bhmm_viterbi_batch_u8(c, A, pi, par0, par1, reinterpret_cast<uint8_t *>(c->runs.path.p), 1)))
            return rc;
        path = c->runs.path.p;
    } else {
        if (int rc = post_decode_device(c, A, pi, par0, par1, true, 1, false))
            return rc;
        path = c->post.path.p;
    }
    return compact(c, path, 1, run_off, dwell, jumps);
}

int bhmm_runs_fetch(bhmm_ctx *c, int64_t *start, int64_t *length, int32_t *state)
{
    if (!c || c->kind < 0)
        return invalid_arg("no observations loaded");
    if (!c->ds.runs_valid)
        return invalid_arg("bhmm_runs_fetch: no runs (call bhmm_path_runs or bhmm_decode_runs on these observations first)");
    BHMM_HIP(hipSetDevice(c->device));
    const size_t R = (size_t)c->ds.runs_count;
    int rc;
    if ((start && (rc = copy_to_host_pinned(c, start, c->runs.start.p, R * sizeof(int64_t)))) ||
        (length && (rc = copy_to_host_pinned(c, length, c->runs.length.p, R * sizeof(int64_t)))) ||
        (state && (rc = copy_to_host_pinned(c, state, c->runs.state.p, R * sizeof(int32_t)))))
        return rc;
    return BHMM_OK;
}

} // extern "C"
