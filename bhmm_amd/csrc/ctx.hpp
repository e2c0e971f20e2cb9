// ctx.hpp -- host-side state of the batched engine (opaque to C callers as bhmm_ctx).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>
#include <string>
#include <vector>

#include "../../include/bhmm_amd.h"

namespace bhmm {

void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what);

#define BHMM_HIP(call)                                  \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess)                           \
            return ::bhmm::hip_fail(e_, #call);         \
    } while (0)

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    // Guard elements in front of p[0] and behind p[n - 1], inside the allocation (both multiples of
    // 16 bytes).  The sweeps of k_estep refill their prefetch registers unconditionally: a chunk's last
    // iteration loads a few CI records before its first (backward) or behind its last (forward) one.
    // Nothing consumes those values, but the addresses must be mapped (SWEEP_GUARD_* below).
    const size_t front = 0, back = 0;
    T *base = nullptr; // what hipMalloc returned: p - front
    DevBuf() = default;
    DevBuf(size_t front_, size_t back_) : front(front_), back(back_) {}
    DevBuf(const DevBuf &) = delete; // (owns its allocation)
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); } // (bhmm_ctx_destroy deletes the context on its own device: nothing is left behind)
    int ensure(size_t count)
    {
        if (count <= n)
            return BHMM_OK;
        release();
        const size_t total = front + count + back;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), total * sizeof(T));
        if (e != hipSuccess) {
            base = nullptr;
            set_error(std::string("hipMalloc of ") + std::to_string(total * sizeof(T)) +
                      " bytes failed: " + hipGetErrorString(e));
            (void)hipGetLastError();
            return BHMM_ERR_NO_MEM;
        }
        p = base + front;
        n = count;
        // debugging aid: BHMM_AMD_POISON=1 fills every fresh allocation with 0xFF bytes (NaN doubles,
        // -1 integers), so that a kernel that reads what nothing wrote shows up at once instead of
        // depending on what the allocator handed out
        static const bool poison = getenv("BHMM_AMD_POISON") != nullptr;
        if (poison) { // (the fill runs on the null stream; the context's streams do not wait for it by themselves)
            (void)hipMemset(base, 0xFF, total * sizeof(T));
            (void)hipDeviceSynchronize();
        }
        return BHMM_OK;
    }
    void release()
    {
        if (base)
            (void)hipFree(base);
        base = p = nullptr;
        n = 0;
    }
};

// Device tables of one segment plan of a forward-only pass (bhmm_score, bhmm_filter; made and uploaded by
// make_seg_tables, seg_host.hpp): trajectory, length and start of every segment, the first segment of every
// trajectory [K + 1] and, at 65..128 states, the segment of every tile row [16 * tiles]
struct SegTables {
    DevBuf<int32_t> seg_traj, seg_len, seg_traj0;
    DevBuf<int64_t> seg_t0;
    DevBuf<int32_t> tile_seg;
};

// What one two-sided sweep over the E-step's chunk plan needs for up to 8 states (sweep_host.hpp; the fused paths of
// bhmm_posterior_decode, bhmm_posterior_marginals and bhmm_posterior_transitions, one of these each): model, probe
// curve, B^T, alpha-row workspace of one range of chunk groups, boundary vectors of both directions, the chunks
// whose exit vector is all zero, failure counter
struct SweepBufs {
    DevBuf<char> model, probe;
    DevBuf<double> Bt, ws, aentry, aexit, bassumed, bout;
    DevBuf<uint8_t> dead;
    DevBuf<unsigned int> fails;
};

} // namespace bhmm

// The fields are grouped by lifetime: `opt` holds what the caller sets (bhmm_ctx_set_option, environment at
// creation) and survives new observations; the problem description and the device / pinned buffers are
// re-made or re-sized by bhmm_ctx_set_observations (allocations are reused); `ds` is the adaptive state of
// one observation set, reset as a whole by bhmm_ctx_set_observations (new_observation_set); `last` holds
// counters and diagnostics of the last calls, read back by bhmm_ctx_get_option.  The remaining top-level
// scalars are state of the call in flight or deliberately outlive the observation set (comment on each).
struct bhmm_ctx {
    int device = 0;
    int num_simd = 1024; // 4 per compute unit (set at creation)
    hipStream_t stream = nullptr;
    bool own_stream = false;

    // ---- caller options (survive bhmm_ctx_set_observations) ----
    struct Options {
        bool spec_enabled = true;        // speculative (verified) chunk boundaries, see k_estep<..., SPEC> (estep_sweep.hpp)
        bool spec_W_fixed = false;       // warm-up given by the caller (option / BHMM_AMD_SPEC_W): never probed
        double spec_tol = 1e-11;         // N <= 8: tolerance of the boundary check (option spec_tol)
        bool carry_enabled = true;       // option "carry" / BHMM_AMD_CARRY=0
        bool obs16_enabled = true;       // option "obs16": 0 keeps the split E-step of the discrete kind on the int32 observations
        bool draw_watch = true;          // option "draw_watch": record and verify draws near the alpha rows' deviation
        double draw_watch_tol = 0.0;     // option "draw_watch_tol" (tests): watch tolerance instead of 64 x deviation
        bool draw_test_redo = false;     // option "draw_test_redo" (tests): treat every event as a decision that did not stand
        int vit_seg_per_simd = 2;
        int vit_seg_warmups = 2;         // a Viterbi segment is at least this many warm-ups long (measured: 1, 2, 4)
        int smp_seg_per_simd = 4;        // (the draw is a short dependent chain: more wavefronts per SIMD hide it)
        bool vit_margin = true;          // accept a first pass whose boundaries are equal to 1e-12 when every decision ON its
                                         // path has a margin (k_vit_margin) instead of running fix-up rounds
        bool vit_mend = true;            // option "viterbi_mend": segments further than 1e-12 run again up to a kept vector
        bool tile_enabled = true;        // option "tile" / BHMM_AMD_TILE=0: takes effect at the next set_observations ...
        int tile_per_cu = 1;             // tiles the segment plan aims at per compute unit (option "tile_per_cu")
        bool wseg_enabled = true;
        bool wseg_split = true;          // 64 states: own, finer plan for the forward pass (wide_plan_segments)
        int wseg_len = 0;                // 0 = automatic
        double f32_tol = 1e-5;           // BHMM_FLAG_SINGLE: tolerance of the fp32 boundary check (option f32_tol)
        int f32_W = 0;                   // ... fp32 warm-up fixed by the caller (option f32_W; 0: measured)
        int score_W = 0;                 // bhmm_score: warm-up fixed by the caller (option score_W; 0: measured per model)
        int score_layout = 1;            // bhmm_score, N <= 8: 1 = one lane per chunk (default), 2 = N/2 lanes per chunk
        int score_seglen = 0;            // bhmm_score, 9..128 states: segment length of its plan (option score_seglen; 0: automatic)
        bool score_lazy = true;          // ... first pass on the lazily scaled kernel (option score_lazy; 0: sum every step)
        int post_W = 0;                  // bhmm_posterior_decode: warm-up fixed by the caller (option post_W; 0: measured)
        int post_ws_mb = 8192;           // ... budget of its alpha-row workspace in MiB (option post_ws_mb; 0: unbounded)
        int marg_W = 0;                  // bhmm_posterior_marginals: warm-up fixed by the caller (option marg_W; 0: measured)
        int marg_ws_mb = 8192;           // ... budget of its alpha-row workspace in MiB (option marg_ws_mb; 0: unbounded)
        int pair_W = 0;                  // bhmm_posterior_transitions: warm-up fixed by the caller (option pair_W; 0: measured)
        int pair_ws_mb = 8192;           // ... budget of its alpha-row workspace in MiB (option pair_ws_mb; 0: unbounded)
        bool pair_fused = true;          // ... option pair_fused: 0 never takes the fused path
        int pair_rows = -1;              // ... row kernel of its generic path: 0 k_pair_rows, 1 k_pair_tile up to 128 states,
                                         // -1 by class (tile_takes, pair_api.hip; option pair_rows)
        int filter_W = 0;                // bhmm_filter: warm-up fixed by the caller (option filter_W; 0: measured)
        int filter_seglen = 0;           // bhmm_filter, 9..64 states: segment length of its plan (option filter_seglen; 0: automatic)
        int filter_parallel = -1;        // ... the time-parallel path: 0 never, 1 always when eligible, -1 automatic
                                         // (eligible and at least FILTER_WIDE_MIN_TOTAL steps; option filter_parallel)
        int filter_tile = -1;            // ... 65..128 states, the matrix-core path (k_filter_tile): 0 never, 1 always when
                                         // eligible, -1 automatic (at least FILTER_TILE_MIN_TOTAL steps; option filter_tile)
        int smooth_wide = -1;            // bhmm_posterior_decode / bhmm_posterior_marginals, 9..64 states: the time-segmented
                                         // path (k_filter_wide + k_smooth_wide_bwd): 0 never, 1 always when eligible, -1
                                         // automatic (smooth_wide_auto, smooth_wide_launch.hpp; option smooth_wide)
        int smooth_tile = -1;            // ... 65..128 states, the matrix-core path (k_filter_tile + k_smooth_tile_bwd): 0 never,
                                         // 1 always when eligible, -1 automatic (smooth_tile_auto, smooth_tile_api.hpp; option
                                         // smooth_tile)
        int smooth_seglen = 0;           // ... both paths: segment length of the plan (option smooth_seglen; 0: automatic)
        int smooth_W = 0;                // ... warm-up fixed by the caller (option smooth_W; 0: measured)
        int smooth_ws_mb = 8192;         // ... budget of the alpha-row workspace in MiB (option smooth_ws_mb; 0: unbounded)
    } opt;

    // ---- loaded problem ----
    int kind = -1;
    int n = 0;    // real number of states
    int N = 0;    // padded (2, 4, 8)
    int M = 0;    // symbols
    bool bt_global = false; // discrete alphabet too large for the LDS tables (global / L2 instead)
    bool obs16 = false;     // discrete, N <= 8: d_obs16 holds the 16-bit copy of these observations under the current plan
    int K = 0;    // trajectories
    int64_t total = 0;
    int L = 0, Lmax = 0, G = 0, Gp = 0;
    int chunk_mult = 1; // automatic plan: 2 / 3 times the default chunk count (very long chunks)
    std::vector<int64_t> offsets;  // [K+1]
    std::vector<int32_t> traj_c0;  // [K+1] first chunk of each trajectory
    int nG = 0;                      // two-level stitch: groups of consecutive chunks (0 when every trajectory is short)
    bool wide = false;               // nstates > 8: wide_kernels.hpp family
    bool gen = false;                // nstates > 64: gen_kernels.hpp family (any N, trajectory-major,
                                     // one workgroup per trajectory; `wide` is false then)

    // ---- adaptive state of one observation set (reset as a whole by bhmm_ctx_set_observations) ----
    struct ObservationSet {
        // chunk plan (N <= 8)
        bool chunk_auto = true;          // the caller left the chunk length to the library
        bool replanned_half = false;     // ... and it has been re-planned with half the chunks (once)
        bool serial_retry_done = false;  // non-finite counts: re-planned with one chunk per trajectory (once)
        // warm-up length: read off the measured forgetting curve at the first E-step on new data
        // (probe_warmup), lengthened after a failed verification; kept when opt.spec_W_fixed
        int spec_W = 288;
        bool spec_calibrated = false;    // probe done for this set of observations
        // boundary vectors carried from one E-step to the next (estep_sweep.hpp: Carry)
        bool carry_valid = false;        // d_carry_* hold vectors of the previous (verified) E-step
        int carry_use = 0;               // this launch: warm-ups start from the carried vectors (their Wc)
        int carry_cap = 0;               // this launch: capture beta when this many steps remain (0: none)
        double carry_kappa = 100.0;      // boundary deviation per unit of model change, running bound
        double carry_rdec = 0.0;         // decades of forgetting per warm-up step, measured: the deviation the
                                         // check found after a FULL warm-up from the uniform vector (0: unknown)
        std::vector<double> prev_model;  // [A | par0 | par1] of the previous E-step
        bool gamma_valid = false;
        bool careful = false;            // E-steps use the kernel with the per-step outlier branch
        bool careful_retry = false;      // the last verdict asked for a repeat with that kernel
        bool wide_careful = false;       // 9..64 states: lazily scaled kernels left their range on these data
        // 9..64 states: time segments of the Viterbi pass [0], of the backward sampler [1] and of the back-trace
        // of the Viterbi pass [2] (finer: the walk is a chain of dependent look-ups, its time is the length of a
        // segment); their tables are in pplan_buf (path_api.hip)
        struct PathPlan {
            int nseg = 0;
            int64_t seglen = 0;
            int64_t maxlen = 0; // longest segment of the plan (boundaries are rounded to multiples of four: up to seglen + 3)
        } pplan[3];
        int smp_W = 0;                   // sampler: warm-up (steps above a segment) of the next call
        // Viterbi (path_api.hip, gen_api.hip): what the calls on these observations learnt
        struct Viterbi {
            bool margin_want = false;    // 9..64 states: a call on these observations needed two or more fix-up rounds
                                         // (the margin acceptance costs about one short round: tried from then on)
            bool seg_given_up = false;   // ... boundaries did not coalesce on these observations: serial kernel
            int rows_fail = 0;           // 129..256 states: first passes in a row that were not accepted (two: given up)
            int W = 0;                   // warm-up the chunked Viterbi last verified with (0: spec_W)
            int bad = 0;                 // ... a shorter one that did not verify
            bool explore = true;         // ... still trying shorter ones (plan.hpp: vit_chunk_attempts)
        } vit;
        int wide_replans = 0;            // 9..64 states: segment plans re-made after failed checks
        bool wseg_given_up = false;      // ... and segmentation abandoned for this data set
        bool tile_latched = true;        // opt.tile_enabled latched: plans, buffers and launches of one data set all use THIS
        int tile_settle = 0;             // warm-up refinements done for these observations (at most 4, first E-step)
        int tile_W_good = 0;             // ... the last warm-up that verified
        int f32_W = 0;                   // fp32 E-step (estep_f32.hip): warm-up read off the forgetting curve at
                                         // 0.01 f32_tol (0: not measured yet), doubled after a failed check
        // bhmm_score, 9..128 states: its own segment plan (tables in score.seg; 65..128 states: and the tile table
        // score.seg.tile_seg), made at the first score call on these observations from the offsets, the state count and
        // the device alone -- never re-made after a check
        int score_nseg = 0;              // segments of the plan (0: not made yet)
        int score_ntraj = 0;             // ... trajectories with at least one step (nseg == ntraj: no boundary)
        int score_seglen_opt = 0;        // ... opt.score_seglen it was made for
        int score_ntiles = 0;            // ... 65..128 states: tiles of 16 segments (k_score_tile)
        // bhmm_filter, 9..64 states: its own segment plan (tables in filt.seg), made at the first eligible filter
        // call on these observations from the offsets, the state count and the device alone -- never after a check
        int filt_nseg = 0;               // segments of the plan (0: not made yet)
        int filt_ntraj = 0;              // ... trajectories with at least one step (nseg == ntraj: no boundary)
        int filt_seglen_opt = 0;         // ... opt.filter_seglen it was made for
        // bhmm_filter, 65..128 states: the segment plan and tile table of k_filter_tile (tables in filt.tseg, with its
        // tile_seg), made the same way; neither the score plan nor the plan above
        int filt_tile_nseg = 0;          // segments of the plan (0: not made yet)
        int filt_tile_ntraj = 0;         // ... trajectories with at least one step (nseg == ntraj: no boundary)
        int filt_tile_ntiles = 0;        // ... tiles of 16 segments
        int filt_tile_seglen_opt = 0;    // ... opt.filter_seglen it was made for
        // posterior calls, 9..64 states: the segment plan of the smoothing pass (tables in smooth.seg, host copies
        // smooth.seg_len / seg_g0), made the same way; none of the plans above
        int smooth_nseg = 0;             // segments of the plan (0: not made yet)
        int smooth_ntraj = 0;            // ... trajectories with at least one step (nseg == ntraj: no boundary)
        int smooth_seglen_opt = 0;       // ... opt.smooth_seglen it was made for
        // posterior calls, 65..128 states: the segment plan of the matrix-core smoothing pass (tables in smooth_tile.seg,
        // the ranges of the budgeted workspace and their tile tables in smooth_tile.ranges / seg.tile_seg / tile_segb),
        // made the same way; none of the plans above
        int smooth_tile_nseg = 0;        // segments of the plan (0: not made yet)
        int smooth_tile_ntraj = 0;       // ... trajectories with at least one step (nseg == ntraj: no boundary)
        int smooth_tile_seglen_opt = 0;  // ... opt.smooth_seglen it was made for
        int smooth_tile_ws_mb_opt = 0;   // ... opt.smooth_ws_mb its ranges were cut for
        // bhmm_path_runs / bhmm_decode_runs (runs_api.hip): the runs of the last call on these observations sit in
        // runs.start / length / state (bhmm_runs_fetch)
        bool runs_tiles_ready = false;   // ... runs.tile_traj holds the trajectory of every tile's first step for these offsets
        bool runs_valid = false;
        int64_t runs_count = 0;          // ... how many (option runs_count)
        // bhmm_path_logprob / bhmm_decode_logprob (pathlp_api.hip)
        bool pathlp_tiles_ready = false; // ... pathlp.tile_traj holds the trajectory of every tile's first step for these offsets
        int32_t pathlp_traj0 = 0;        // ... its first entry: the trajectory of step 0 (the partial of tile i and trajectory
                                         // k is slot i + k - pathlp_traj0)
    } ds;

    // ---- counters and diagnostics of the last calls (bhmm_ctx_get_option) ----
    struct LastCall {
        int spec_fail = 0, spec_ok = 0;
        float spec_last_dev = 0.f;
        int carry_ok = 0, carry_fail = 0, carry_last_W = 0;
        bool obs16_used = false;         // the sweeps of the last E-step read the 16-bit observations (option obs16_used)
        bool draw_fwd_segmented = false; // the last sampler's alpha rows came from the time-segmented forward pass
        bool smp_segmented = false;      // the last sample_paths call ran over time segments
        int smp_seg_mismatch = 0, smp_seg_rounds = 0;
        double draw_alpha_dev = 0.0;     // largest boundary deviation of the forward pass the draws read (0: exact rows)
        unsigned int draw_events = 0;    // last call: draws inside the watch tolerance
        unsigned int draw_checked = 0;   // ... of them decided again on the windowed serial recursion
        unsigned int draw_redone = 0;    // ... calls repeated on the exact alpha rows (0 / 1)
        int vit_seg_mismatch = 0, vit_seg_rounds = 0;
        int vit_far = 0;                 // boundaries of the last first pass that were not equal to 1e-12
        int vit_mended = 0;              // ... how many the last call ran again alone (opt.vit_mend)
        int vit_margin_used = 0;         // ... the last call was accepted by the path margins
        int vit_margin_close = 0;        // ... segments with a close decision on the path in the last call (then: rounds)
        unsigned int viterbi_close = 0;  // ... number of lanes that met a close decision
        bool viterbi_chunked = false;    // last bhmm_viterbi_batch ran chunk-parallel (verified)
        unsigned int wide_trouble = 0;   // flag word of the last lazily scaled E-step (which self-check fired)
        bool tile_used = false;          // the last E-step ran on the tile kernels
        double ms[5] = {0, 0, 0, 0, 0};
        bool f32_used = false;           // the last E-step ran in fp32 end to end (BHMM_FLAG_SINGLE)
        int f32_fallbacks = 0;           // E-steps that asked for fp32 and ran the fp64 path
        float f32_last_dev = 0.f;        // largest relative boundary deviation of the last fp32 check
        int score_fallbacks = 0;         // bhmm_score: models whose boundaries did not verify at the first warm-up
        int score_path = 0;              // ... first pass of the last call: 0 serial, 1 chunk kernels (N <= 8), 2 k_score_wide,
                                         // 3 k_score_tile (65..128 states)
        int score_segments = 0;          // ... segments of the score plan it ran on (0: no such plan)
        int score_W_max = 0;             // ... longest warm-up of its first pass at 9..128 states (0: no boundary, other paths)
        int post_fallbacks = 0;          // bhmm_posterior_decode: calls whose boundaries did not verify at the first warm-up
        int post_path = 0;               // ... first pass of the last call: 3 matrix cores (k_smooth_tile_bwd, 65..128 states),
                                         // 2 time segments (k_smooth_wide_bwd, 9..64 states), 1 fused (k_post_sweep), 0 generic
                                         // (E-step + gamma rows)
        int marg_fallbacks = 0;          // bhmm_posterior_marginals: calls whose boundaries did not verify at the first warm-up
        int marg_path = 0;               // ... first pass of the last call: 3 matrix cores (k_smooth_tile_bwd, 65..128 states),
                                         // 2 time segments (k_smooth_wide_bwd, 9..64 states), 1 fused (k_marg_sweep), 0 generic
                                         // (E-step + gamma rows)
        int pair_fallbacks = 0;          // bhmm_posterior_transitions: calls whose boundaries did not verify at the first warm-up
        int pair_path = 0;               // ... first pass of the last call: 1 fused (k_pair_sweep), 0 generic (filter +
                                         // marginals + pair rows)
        int pair_rows_kernel = 0;        // ... row kernel of the last generic pass: 0 k_pair_rows, 1 k_pair_tile
        int smooth_segments = 0;         // segments of the smoothing plan the last posterior call ran on (0: another path)
        int filter_fallbacks = 0;        // bhmm_filter: calls whose boundaries did not verify at the first warm-up
        int filter_path = 0;             // ... first pass of the last call: 3 matrix cores (k_filter_tile, 65..128 states),
                                         // 2 time segments (k_filter_wide, 9..64 states), 1 fused (k_filter_sweep, up to
                                         // 8 states), 0 serial (k_filter_serial)
        int filter_segments = 0;         // ... segments of the filter plan it ran on (0: no such plan)
        int filter_redone = 0;           // ... filter_path 3: trajectories of the last call done again on k_filter_serial
                                         // because a segment left the range of k_filter_tile (option filter_redone)
        float runs_ms = 0.f;             // bhmm_path_runs / bhmm_decode_runs: device time of count, scan and scatter
        float pathlp_ms = 0.f;           // bhmm_path_logprob / bhmm_decode_logprob: device time of prepare, tiles and finish
        int pathlp_table = 0;            // ... 1: the last call kept the log-transition table in LDS, 0: it read it through L2
    } last;

    // ---- not reset by bhmm_ctx_set_observations: they outlive the observation set ----
    bool rows32_valid = false;       // d_ws32 written by the last forward-only pass (not reset: outlives the observation set)
    int spec_probes_left = 0;        // re-probes allowed after failed checks (not reset: outlives the observation set)
    int carry_Wc = 0;                // carried vectors captured for warm-ups of about this many steps (not reset)
    double carry_delta = -1.0;       // model change against the previous E-step, -1: unknown (not reset)
    int w_nseg[3] = {0, 0, 0};       // wide family segment plans, see d_wseg_* (not reset: read by get_option on any family)
    int64_t wseg_cur_len = 0;        // segment length of plan 1, re-plans only lengthen (not reset: read with w_nseg)
    int tile_reason = 0;             // why the tile path was left (0: it was not): 1 calibration saw a self-check fire,
                                     // 2 calibration did not converge, 3 warm-up >= half a trajectory, 4 self-check in an
                                     // E-step, 5 boundaries did not verify after three attempts, 6 fixed warm-up does not
                                     // verify (reset by tile_gen_alloc only: outlives the observation set at 9..64 states)
    int w_ntiles[3] = {0, 0, 0}, w_ntilesb[3] = {0, 0, 0}; // tiles of the wide plans (written with them)

    // ---- the call in flight / the previous call ----
    bool fwd_defer = false;          // forward-only pass: enqueue the boundary check, do not wait for it
    bool fwd_pending = false;        // ... its verdict is still to be read (forward_ci_verdict)
    bool keep_path = false;          // bhmm_sample_paths from bhmm_mvn_sample_paths: sample_run<N> leaves the int32 path at
                                     // the front of d_scratch2 although no host pointer is given (the wide and generic
                                     // families always do)
    int carry_Wout = 0;              // this launch: capture alpha this many steps before the chunks
    bool carry_store = false;        // this launch: store the captures (else the sweep is only split there)
    std::vector<double> last_pi;     // initial distribution and flags of the last E-step (nonfinite_retry repeats that call)
    int last_flags = 0;
    int tail_slot = 0;               // verdict word set of the next E-step
    bool tail_ready = false;         // d_tail allocated and its verdict words cleared
    bool ev_lean = false;            // last E-step recorded only ev[2..4]
    int wide_retry = 0;              // time-segmented attempts of the E-step call in flight that did not verify
    bool gamma_wanted = false;       // the E-step in flight stores gamma (a re-plan must re-size the rows)
    bool prefetched = false;         // stats + logL_k of the last E-step already sit in h_pinned
    bool logLk_prefetched = true;    // ... logL_k included (not for many trajectories: on demand)
    bool last_stats_internal = true;
    bool last_stats_checked = false; // the caller's buffer of the last E-step has been looked at by bhmm_estep_fetch
    double *last_stats = nullptr;    // device buffer the last E-step wrote its statistics to
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool ev_pending = false;

    // ---- device buffers (kept across observation sets: DevBuf::ensure only grows them) ----
    bhmm::DevBuf<int32_t> d_ctraj, d_clen, d_traj_c0;
    bhmm::DevBuf<int64_t> d_ct0, d_cgoff;
    // Guards of the buffers k_estep prefetches from (DevBuf::front / back), in CI records of the largest
    // kind (8 states): the backward sweeps reach up to 8 records before a chunk's first one (observations,
    // alpha rows, their exponents), the forward sweep up to 2 * ESTEP_PF_F = 8 records behind its last one
    // (observations only).  An explicit-emission record is 8 * 64 doubles like an alpha row.
    static constexpr size_t SWEEP_GUARD_FRONT = 8, SWEEP_GUARD_BACK = 8, SWEEP_REC_DOUBLES = 8 * 64;
    bhmm::DevBuf<char> d_obs_ci{SWEEP_GUARD_FRONT * SWEEP_REC_DOUBLES * sizeof(double),
                                SWEEP_GUARD_BACK * SWEEP_REC_DOUBLES * sizeof(double)}; // CI observations (double / int32 / N doubles)
    // the discrete kind's 16-bit copy for the main loops of the split E-step (k_pack_obs16): 64 elements per step
    // of a record group, guards in elements of this type
    bhmm::DevBuf<uint16_t> d_obs16{SWEEP_GUARD_FRONT * 64, SWEEP_GUARD_BACK * 64};
    bhmm::DevBuf<char> d_obs_rm;     // trajectory-major observations (Viterbi / sampling)
    bhmm::DevBuf<double> d_Bt;       // [M][N] transposed emission matrix
    bhmm::DevBuf<double> d_M;        // chunk transfer matrices
    bhmm::DevBuf<double> d_aentry, d_bexit, d_gamma_ci;
    bhmm::DevBuf<double> d_ws{SWEEP_GUARD_FRONT * SWEEP_REC_DOUBLES, 0}; // CI workspace: alpha / beta rows
    bhmm::DevBuf<float> d_ws32;      // Gibbs step: CI alpha rows rounded to fp32 (forward-only pass)
    bhmm::DevBuf<double> d_logLc, d_logLk, d_gamma0, d_partials, d_dpartials, d_stats;
    bhmm::DevBuf<char> d_scratch;    // paths, uniforms, pointer tables ...
    bhmm::DevBuf<char> d_scratch2;
    bhmm::DevBuf<int64_t> d_offsets; // [K+1] trajectory offsets (time steps)
    bhmm::DevBuf<int32_t> d_obsnan;  // [1] set by the upload if a gaussian observation is NaN
    bhmm::DevBuf<int64_t> d_soff;    // [K] position of each trajectory in the device random stream
                                     // (unset: its offset here; a sharded caller sets global ones)
    bhmm::DevBuf<double> d_Brm;      // [n][M] emission matrix, row-major (path kernels)
    bhmm::DevBuf<double> d_alpha_rm; // [total][n] alpha, trajectory-major (path sampling)
    bhmm::DevBuf<double> d_wmodel;   // model parameters of the 9..64-state family
    bhmm::DevBuf<char> d_probe;      // probe: sample positions + forgetting curve
    bhmm::DevBuf<double> d_aexit, d_bentry;
    bhmm::DevBuf<double> d_carry_a, d_carry_b;
    bhmm::DevBuf<int32_t> d_carry_da, d_carry_db;
    bhmm::DevBuf<unsigned int> d_specres;
    // exponents of the stored alpha rows (k_estep PH_P1 -> PH_P2): [Gp] per chunk, then CI rows of 64; the
    // guard in front keeps SWEEP_GUARD_FRONT rows before the first one mapped however small Gp is
    bhmm::DevBuf<int32_t> d_ea{SWEEP_GUARD_FRONT * 64, 0};
    bhmm::DevBuf<double> d_tail;      // same layout as h_raw, written by k_tail (one D2H copy)
    bhmm::DevBuf<double> d_fold;      // partial statistics folded 128 rows at a time (k_fold_rows)
    bhmm::DevBuf<double> d_tbpart;    // k_tail: per trajectory block [sum logL | sum gamma_0 (N)]
    struct PathPlanBufs {             // tables of ds.pplan[i]
        bhmm::DevBuf<int32_t> traj, len, traj0; // traj0[k]: first segment of trajectory k, [K + 1]
        bhmm::DevBuf<int64_t> t0;
    } pplan_buf[3];
    bhmm::DevBuf<uint8_t> d_vmaps, d_vend; // back-trace over segments: maps [nseg][64], last state of each segment
    bhmm::DevBuf<int32_t> d_sentry, d_sexit;
    // draws decided within reach of the alpha rows' verified deviation (draw_verify.hpp)
    bhmm::DevBuf<char> d_dv;          // [count | disagree | unconverged | pad] (16 B) | DrawEvent[DRAW_EVENT_CAP] | model
    bhmm::DevBuf<double> d_vckpt;     // the first Viterbi pass's vector at every 64th step
    bhmm::DevBuf<uint8_t> d_vflag;    // segments the next fix-up round repeats
    bhmm::DevBuf<int32_t> d_grp_c0, d_grp_c1, d_grp_traj0; // [nG], [nG], [K+1]
    bhmm::DevBuf<double> d_P, d_agrp, d_bgrp;              // group products / boundary vectors
    bhmm::DevBuf<double> d_gpobs, d_gW, d_gAt, d_gxipart, d_gpart, d_gsym;
    bhmm::DevBuf<double> d_bigBf, d_bigBb; // more than 128 states: A / A^T in matrix-operand order (big_kernels.hpp)
    // wide family: segment tables.  Plans: 0 = one segment per trajectory (exact serial recursion),
    // 1 = time segments with verified warm-up boundaries (both passes), 2 = the forward pass's own, finer
    // time segments (64 states: it fits two wavefronts per SIMD, the backward pass one)
    bhmm::DevBuf<int32_t> d_wseg_traj[3], d_wseg_len[3], d_wseg_traj0[3];
    bhmm::DevBuf<int64_t> d_wseg_t0[3];
    bhmm::DevBuf<int64_t> d_wseg_fmid;  // plan 1: start of the forward pass's second segment inside each
    bhmm::DevBuf<double> d_wlogLseg, d_waentry, d_waexit, d_wbexit, d_wbentry;
    // row-batched matrix-core recursions (tile_kernels.hpp): 16 segments per workgroup
    bhmm::DevBuf<int32_t> d_tile_seg[3];  // [16 * ntiles] segment of every tile row (-1: none), forward pass
    bhmm::DevBuf<int32_t> d_tile_segb[3]; // ... backward pass (tiles are formed per direction, plan.hpp)
    bhmm::DevBuf<int32_t> d_wexp;    // [total] exponent the forward pass removed at every step
    bhmm::DevBuf<int32_t> d_wePseg;  // [segments] ... summed over the main part of every segment
    // fp32 E-step (estep_f32.hip): boundary vectors [4][Gp][N], B^T in fp32, verdict words
    bhmm::DevBuf<float> d_f32vec, d_Bt32;
    bhmm::DevBuf<unsigned int> d_f32words;
    // bhmm_score (score_api.hip): its own buffers -- model table, B^T per model, per (model, chunk) log-normaliser
    // and boundary vectors, per (model, trajectory) logL, failure counters, probe curve; nothing else reads them
    struct ScoreBufs {
        bhmm::DevBuf<char> models, probe;
        bhmm::DevBuf<double> Bt, logLc, aentry, aexit, logLk, par;
        bhmm::DevBuf<int32_t> W;
        bhmm::DevBuf<unsigned int> fails;
        // 9..128 states: parameter blocks of the batch's models, tables of the plan ds.score_nseg counts (65..128
        // states: with the tile table, [16 * ds.score_ntiles])
        bhmm::DevBuf<double> wpar;
        bhmm::SegTables seg;
    } score;
    // bhmm_posterior_decode (post_api.hip): its own buffers -- a SweepBufs and the results on the device (path:
    // bytes or int32; conf); nothing else reads them
    struct PostBufs : bhmm::SweepBufs {
        bhmm::DevBuf<char> path;
        bhmm::DevBuf<float> conf;
    } post;
    // bhmm_posterior_marginals (marg_api.hip): its own buffers -- a SweepBufs, the projection matrix V, and the
    // result staged on the device when the caller's buffer is on the host (out); nothing else reads them
    struct MargBufs : bhmm::SweepBufs {
        bhmm::DevBuf<char> out;
        bhmm::DevBuf<double> V;
    } marg;
    // bhmm_posterior_transitions (pair_api.hip): its own buffers -- a SweepBufs, the pair weights W [n][n][PAIR_QMAX]
    // (padded), the result staged on the device when the caller's buffer is on the host (out), and for the generic
    // path the filtered rows (filt) and posterior rows (gam) of every step, [total][n] doubles each, a device copy of
    // the transition matrix (A) and the matrices [A | M_1 | ...] of k_pair_tile in its operand order (Bop,
    // pair_tile_kernels.hpp).  W_host / A_host / Bop_host: what W, A and Bop on the device hold (upload_if_changed,
    // pair_api.hip: an unchanged matrix is not uploaded again; Bop is formed on the host at every call that takes that
    // kernel, so a change of A, W, Q or of the form rebuilds it and nothing else does); nothing else reads them
    struct PairBufs : bhmm::SweepBufs {
        bhmm::DevBuf<char> out;
        bhmm::DevBuf<double> W, filt, gam, A, Bop;
        std::vector<double> W_host, A_host, Bop_host;
    } pair;
    // bhmm_filter (filter_api.hip): its own buffers -- model, B^T, boundary vectors, the chunks whose exit vector
    // is all zero and per trajectory the first of them, failure counter, probe curve, the projection matrix V, the
    // parameters of the serial path, and the two results staged on the device when the caller's buffers are on
    // the host (rows, logc); 9..64 states: the model's parameter block and the tables of the plan ds.filt_nseg
    // counts (seg; dead / first_dead then count segments); 65..128 states: the tables of the plan ds.filt_tile_nseg
    // counts (tseg), dead is then the range flag of every segment, redo the trajectories to do again and
    // fails the words of k_filter_tile_check / k_filter_tile_redo; nothing else reads them
    struct FiltBufs {
        bhmm::DevBuf<char> model, probe, rows, logc;
        bhmm::DevBuf<double> Bt, aentry, aexit, V, par;
        bhmm::DevBuf<uint8_t> dead;
        bhmm::DevBuf<int32_t> first_dead;
        bhmm::DevBuf<unsigned int> fails;
        bhmm::DevBuf<double> wpar;
        bhmm::SegTables seg, tseg;
        bhmm::DevBuf<uint8_t> redo;
    } filt;
    // the time-segmented path of the two posterior calls at 9..64 states (smooth_wide.hip): its own buffers -- model,
    // parameter block, probe curve, the tables of the plan ds.smooth_nseg counts with host copies of every segment's
    // length and first global step (the ranges of the budgeted workspace are cut on the host), the filtered rows of
    // one range of segments (ws), entry / exit vectors of both directions, the segments whose forward sum became
    // zero (dead) and those the backward kernel flagged (trouble), and the words [boundaries out of tolerance |
    // largest deviation | flagged segments] (fails); nothing else reads them
    struct SmoothBufs {
        bhmm::DevBuf<char> model, probe;
        bhmm::DevBuf<double> wpar, ws, aentry, aexit, bexit, bentry;
        bhmm::DevBuf<uint8_t> dead, trouble;
        bhmm::DevBuf<unsigned int> fails;
        bhmm::SegTables seg;
        std::vector<int32_t> seg_len;
        std::vector<int64_t> seg_g0;
    } smooth;
    // the matrix-core path of the two posterior calls at 65..128 states (smooth_tile.hip): its own buffers -- the
    // model's table entry and parameter block (B^T for discrete), the tables of the plan ds.smooth_tile_nseg counts
    // (seg; seg.tile_seg holds the forward tiles of every range, tile_segb the backward ones) with the ranges of the
    // budgeted workspace and every segment's first global step on the host, the filtered rows of one range (ws),
    // entry / exit vectors of both directions, the range flags of both directions (fflag: k_filter_tile's, dead
    // segments included; bflag: k_smooth_tile_bwd's) and the words of a pass (SMT_*); nothing else reads them
    struct SmoothTileBufs {
        bhmm::DevBuf<char> model;
        bhmm::DevBuf<double> wpar, ws, aentry, aexit, bexit, bentry;
        bhmm::DevBuf<uint8_t> fflag, bflag;
        bhmm::DevBuf<unsigned int> words;
        bhmm::SegTables seg;
        bhmm::DevBuf<int32_t> tile_segb;
        std::vector<int32_t> r_s0, r_s1, r_f0, r_nf, r_b0, r_nb; // per range (plan::TileRange)
        std::vector<int64_t> r_steps, r_g0;                       // ... its steps and its first global step
    } smooth_tile;
    // bhmm_path_runs / bhmm_decode_runs (runs_api.hip): its own buffers -- the path where the call has to hold it (a
    // host path staged, the Viterbi path of bhmm_decode_runs), the trajectory of every tile's first step (made once per
    // observation set, ds.runs_tiles_ready), run count and exclusive offset of every tile, the sums
    // of the scan's blocks (the last entry: R), the status word, the first run of every trajectory, the runs
    // (start, length, state: sized from R; valid while ds.runs_valid), the statistics tables [n * 5 | n * n] and
    // the events of runs_ms (count + scan, scatter + finish); nothing else reads them
    struct RunsBufs {
        bhmm::DevBuf<char> path;
        bhmm::DevBuf<int32_t> tile_traj, tile_cnt, state;
        bhmm::DevBuf<int64_t> tile_off, blk, run_off, start, length;
        bhmm::DevBuf<unsigned long long> tables;
        bhmm::DevBuf<unsigned int> status;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        RunsBufs() = default;
        RunsBufs(const RunsBufs &) = delete;
        RunsBufs &operator=(const RunsBufs &) = delete;
        ~RunsBufs()
        {
            for (hipEvent_t e : ev)
                if (e)
                    (void)hipEventDestroy(e);
        }
    } runs;
    // bhmm_path_logprob / bhmm_decode_logprob (pathlp_api.hip): its own buffers -- the path where the call has to hold
    // it (a host path staged, the Viterbi path of bhmm_decode_logprob), the trajectory of every tile's first step (made
    // once per observation set, ds.pathlp_tiles_ready), the stacked models as the caller gave them (raw) and their
    // log tables (tab: per model log A, log pi and log B or mu, 1 / sigma, -log sigma - log(2 pi) / 2), one partial
    // per (model, tile, trajectory with a step in the tile), the result [nmodels][K], the status word and the events
    // of pathlp_ms; nothing else reads them
    struct PathLpBufs {
        bhmm::DevBuf<char> path;
        bhmm::DevBuf<int32_t> tile_traj;
        bhmm::DevBuf<double> raw, tab, part, logp;
        bhmm::DevBuf<unsigned int> status;
        hipEvent_t ev[2] = {nullptr, nullptr};
        PathLpBufs() = default;
        PathLpBufs(const PathLpBufs &) = delete;
        PathLpBufs &operator=(const PathLpBufs &) = delete;
        ~PathLpBufs()
        {
            for (hipEvent_t e : ev)
                if (e)
                    (void)hipEventDestroy(e);
        }
    } pathlp;

    // multivariate gaussian emissions (mvn_api.hip): the D-dimensional observations X
    // [total][D], the emission rows made from them [total][n] (handed to bhmm_ctx_set_observations as explicit
    // observations on the device), m_t [total] and shift_k [K], the tables of the last parameters ([mu | W | c]),
    // partials and result of the moments.  None of it is touched by bhmm_ctx_set_observations, which the re-load
    // inside bhmm_mvn_emissions calls (reloading); a call of it from outside ends the set (active)
    struct MvnBufs {
        bool active = false;     // bhmm_ctx_set_observations_mvn has loaded X
        bool reloading = false;  // the bhmm_ctx_set_observations in flight is bhmm_mvn_emissions' own
        bool rows_valid = false; // rows, m and shift belong to a bhmm_mvn_emissions on these observations
        int D = 0, n = 0, K = 0, chunk = 0;
        int64_t total = 0;
        std::vector<int64_t> offsets; // [K + 1]
        bhmm::DevBuf<int64_t> d_offsets;
        bhmm::DevBuf<double> X, rows, m, shift, tab, part, out;
        // bhmm_mvn_path_moments: a host path staged on the device, the bad-state word
        bhmm::DevBuf<char> path;
        bhmm::DevBuf<unsigned int> path_status;
        // read-only options mvn_rows_ms, mvn_reload_ms, mvn_moments_ms, mvn_path_moments_ms: device time of the rows
        // and shift kernels, host time of the explicit re-load, device time of the two moment kernels, of the path
        // moments and their finish (events ev[0..1], ev[2..3], ev[4..5])
        float rows_ms = 0.f, reload_ms = 0.f, moments_ms = 0.f, path_moments_ms = 0.f;
        hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        MvnBufs() = default;
        MvnBufs(const MvnBufs &) = delete;
        MvnBufs &operator=(const MvnBufs &) = delete;
        ~MvnBufs()
        {
            for (hipEvent_t e : ev)
                if (e)
                    (void)hipEventDestroy(e);
        }
    } mvn;

    // gaussian-mixture emissions (gmm_api.hip), on the observations of the mvn block: rows, m,
    // and shift are that block's; here the table of the components and the (total, n M) buffer that holds the log responsibilities of the
    // last bhmm_gmm_emissions with want_resp and, after bhmm_gmm_moments, the weights the moments were taken with
    struct GmmBufs {
        int M = 0;             // components per state of the last bhmm_gmm_emissions (0: the rows are not a mixture's)
        bool resp_log = false; // resp holds log responsibilities of the loaded rows
        bool resp_any = false; // ... or the weights made from them (bhmm_gmm_fetch_resp)
        bhmm::DevBuf<double> resp;
        // the component draws of a Gibbs sweep: the table [mu | W | c | log w] of the last
        // bhmm_gmm_emissions, kept (the mvn block's table is overwritten by the means of every moments call), its
        // covariance type, and the labels s_t M + c_t of the last draw
        int cov_type = 0;
        bhmm::DevBuf<double> tab;
        bhmm::DevBuf<int32_t> labels;
        bhmm::DevBuf<unsigned int> draw_status;
        float weights_ms = 0.f; // read-only option gmm_weights_ms: device time of the last k_gmm_weights
        float draw_ms = 0.f;    // read-only option gmm_draw_ms: device time of the last k_gmm_draw_components
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        GmmBufs() = default;
        GmmBufs(const GmmBufs &) = delete;
        GmmBufs &operator=(const GmmBufs &) = delete;
        ~GmmBufs()
        {
            for (hipEvent_t e : ev)
                if (e)
                    (void)hipEventDestroy(e);
        }
        void forget() { M = 0, resp_log = resp_any = false; }
    } gmm;

    // ---- pinned host buffers ----
    unsigned int *h_specres = nullptr; // pinned
    double *h_small = nullptr;         // pinned, 64 KB: small results of the path calls (one copy per call)
    double *h_raw = nullptr;           // pinned: [verdict words, 2 sets (4 doubles) | stats | logL_k]
    double *h_pinned = nullptr;        // = h_raw + 4: stats + logL_k landing zone
    size_t h_pinned_n = 0;
};
