// host_internal.hpp -- functions one translation unit of libbhmm_amd.so calls in another.  Every defining
// unit includes this header as well, so the compiler checks each declaration against its definition.
// (Inline host code several units share -- the protocol constants, the probe's staging, the parameter block of a
// WideModel, the upload of a forward-only pass's plan -- is in seg_host.hpp, the scaffold of the paths for up to 8
// states in fused_host.hpp; the arithmetic and the acceptance protocol in plan.hpp.)
#pragma once
#include <math.h>
#include <stdint.h>

#include <functional>
#include <string>

#include "ctx.hpp"
#include "plan.hpp"

namespace bhmm {

struct Chunks;    // estep_kernels.hpp
struct Segs;      // wide_kernels.hpp
struct WideModel; // wide_kernels.hpp
struct DrawWatch; // draw_verify.hpp

// ---- bhmm_amd.hip (up to 8 states, context, E-step) ----
int invalid_arg(const std::string &msg); // error message + BHMM_ERR_INVALID
Chunks chunks_of(const bhmm_ctx *c);
int forward_ci(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1);
int forward_ci_verdict(bhmm_ctx *c, bool *ok);
int unpack_ws_rows(bhmm_ctx *c, double *dst_dev);
// warm-up length read off the measured forgetting curve (k_forget_probe) at `target` (0: none measured)
int probe_warmup_target(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                        double target, int *W);
// The checks every model entry point (bhmm_estep, bhmm_viterbi_batch[_u8], bhmm_sample_paths[_dev]) starts with:
// observations loaded; `given` (its pointer arguments are there, else null_msg); with `emissions`, the
// parameters the emission kind needs.  Then the context's device is made current.
int enter_model_call(bhmm_ctx *c, bool given, const char *null_msg, bool emissions, const double *par0,
                     const double *par1);
int64_t longest_traj(const bhmm_ctx *c); // steps of the longest trajectory
// The status words of the verifying passes: d_specres (at least `words`) and its pinned host copy h_specres
// (four words).  specres_reset clears the first `words` on the stream; specres_read copies them into
// h_specres and waits for the stream (wait = false: the caller synchronises, after copies of its own).
int ensure_specres(bhmm_ctx *c, size_t words = 4);
int specres_reset(bhmm_ctx *c, int words = 4);
int specres_read(bhmm_ctx *c, int words = 4, bool wait = true);

// ---- estep_f32.hip (BHMM_FLAG_SINGLE, up to 8 states) ----
// *done: the E-step ran in fp32 and verified; false: the caller runs the fp64 path (nothing else changed)
int estep_f32(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
              double *stats_dev, int flags, bool *done);

// ---- score_api.hip / filter_api.hip: calibration of the warm-up at 65..128 states (Tile::calibrate, TileFilt) ----
constexpr int SCORE_TILE_W0 = 32;            // the two warm-ups the calibration runs at
constexpr int SCORE_TILE_W1 = 64;
constexpr double SCORE_TILE_DEV_OK = 3e-13;  // boundary deviation that needs no longer warm-up (tile_gen.hip)
constexpr double SCORE_TILE_DEV_GOAL = 1e-13; // the deviation the decay is extrapolated to
constexpr double SCORE_TILE_MARGIN = 1.25;   // safety factor on the extrapolated decay (tile_gen.hip)
constexpr int SCORE_TILE_W_SLOW = 1024;      // no decay between the two warm-ups: this one, the check decides
using plan::SCORE_TILE_W_MAX;                // (plan.hpp, beside the protocol it caps)
// the warm-up from the largest boundary deviations d0, d1 of the passes at SCORE_TILE_W0 and SCORE_TILE_W1 (d1 not
// good enough as it is): the geometric decay between the two extrapolated to SCORE_TILE_DEV_GOAL, times the
// margin, rounded up to 8
inline int score_tile_extrapolate(double d0, double d1)
{
    d0 = d0 > 1e-300 ? d0 : 1e-300;
    d1 = d1 > 1e-300 ? d1 : 1e-300;
    if (!(d1 < 0.5 * d0))
        return SCORE_TILE_W_SLOW;
    const double rate = log(d0 / d1) / (double)(SCORE_TILE_W1 - SCORE_TILE_W0); // per step
    const double w = SCORE_TILE_W1 + SCORE_TILE_MARGIN * log(d1 / SCORE_TILE_DEV_GOAL) / rate;
    const double w8 = (ceil(w) + 7.0) / 8.0;
    return (int)(w8 < SCORE_TILE_W_MAX / 8 ? w8 : SCORE_TILE_W_MAX / 8) * 8;
}

// ---- filter_api.hip (bhmm_filter) ----
// Steps of an observation set from which a call at 9..64 states takes the time-parallel path by itself (option
// filter_parallel = -1; read-only option filter_wide_min_total).  To be the break-even against k_filter_serial of
// the scan in DESIGN.md section 16 (tools/filter_time.py --only scan, profiles/filter/filter_time.json), rounded up
// to a power of two and not below 32768: tests/test_filter_gpu.py::test_parity_serial pins the serial kernel for a
// default call on 23734 steps.  The scan puts the break-even below 4096 steps (64 states: 28.4 ms against 2.4 ms
// there), so this is the floor, not the break-even; lowering it also owns that test.
constexpr int64_t FILTER_WIDE_MIN_TOTAL = 32768;
// The same for 65..128 states (k_filter_tile, option filter_tile = -1; read-only option filter_tile_min_total): the
// break-even against k_filter_serial at 128 states (tools/filter_time.py --only tile, the scan in DESIGN.md section
// 16), rounded up to a power of two and not below 32768: tests/test_filter_gpu.py::test_parity_serial pins the
// serial kernel for a default call at 100 states on 23734 steps.  The scan puts the break-even below 4096 steps
// (128 states: 50.0 ms against 2.5 ms there), so this is the floor, not the break-even.
constexpr int64_t FILTER_TILE_MIN_TOTAL = 32768;

// ---- post_api.hip (bhmm_posterior_decode) ----
// Everything bhmm_posterior_decode does before its results leave the device: the checks (given: the caller's pointer
// arguments are there), the path the call takes and its fallbacks; the decoded path is then in c->post.path (one
// byte per step with path_u8, else int32) and, with want_conf, the confidences in c->post.conf, complete in the
// order of the context's stream.  bhmm_decode_runs compacts that path instead of delivering it.
int post_decode_device(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                       bool given, int path_u8, bool want_conf);

// ---- smooth_wide.hip (bhmm_posterior_decode / bhmm_posterior_marginals at 9..64 states) ----
// Steps of an observation set below which the option smooth_wide = -1 never takes the time-segmented path (read-only
// option smooth_wide_min_total): a power of two, not below 32768 -- the existing tests pin the generic path for a
// default call on 23734 steps.  Above it the automatic rule is per lane-group class and call form, from the
// measurements of DESIGN.md section 17 (smooth_wide_auto, smooth_wide_launch.hpp): no cell is on today.
constexpr int64_t SMOOTH_WIDE_MIN_TOTAL = 32768;

// ---- smooth_tile.hip (bhmm_posterior_decode / bhmm_posterior_marginals at 65..128 states) ----
// Steps of an observation set below which the option smooth_tile = -1 never takes the matrix-core path (read-only
// option smooth_tile_min_total): a power of two, not below 32768 -- the existing tests pin the generic path for a
// default call at 100 states on 23734 steps.  Above it the automatic rule is per call form, from the measurements
// of DESIGN.md section 18 (smooth_tile_auto, smooth_tile_api.hpp).
constexpr int64_t SMOOTH_TILE_MIN_TOTAL = 32768;

// ---- wide_api.hip (9..64 states) ----
int wide_alloc(bhmm_ctx *c);
int wide_model(bhmm_ctx *c, int kind, const double *A, const double *pi, const double *par0, const double *par1,
               WideModel &m);
int wide_plan(bhmm_ctx *c, int which, int64_t seglen, int mult = 1);
Segs segs_of(bhmm_ctx *c, int which);
int wide_forward(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1);
int wide_forward_draw(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1);
int wide_estep(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
               double *stats_dev, int flags);
int wide_backward(bhmm_ctx *c, const double *A);
int wide_transition_counts(double *C, const double *A, const double *pobs, const double *alpha, const double *beta,
                           int n, int64_t T);

// ---- path_api.hip (Viterbi, path sampling) ----
int wide_path_plan(bhmm_ctx *c, int which, int64_t seglen, Segs &sg);
// The paths of a Viterbi call to the caller (out_fmt 0: int32 to a host buffer, 1: one byte per step to a host
// buffer, 2: one byte per step in a device buffer, written there already); completes the call's stream.  A
// pageable host buffer of 8 MiB or more is registered for the copy.
int deliver_paths(bhmm_ctx *c, void *paths_out, int out_fmt, const void *dev_paths);
// `bytes` from the device to a host buffer in one copy, complete on return (deliver_paths, bhmm_filter,
// bhmm_posterior_marginals, bhmm_runs_fetch).  A pageable buffer of 8 MiB or more is registered for the transfer (a
// pageable destination goes through the runtime's staging buffers at a fraction of the link rate); one the caller
// pinned already (hipHostMalloc / hipHostRegister, torch pin_memory) is used as it is
int copy_to_host_pinned(bhmm_ctx *c, void *dst, const void *src, size_t bytes);
// The acceptance protocol of a segment-parallel Viterbi pass on one plan: the first pass is
// accepted when every boundary is bit-identical to its predecessor's vector, or -- vall kept -- when every
// boundary is within SEG_VIT_TOL (after mending the far ones) and every decision on the path clears the margin;
// else fix-up rounds up to max_rounds decide.  The family's hooks launch its kernels (BHMM_* codes):
struct SegViterbi {
    std::function<int(bool fix)> pass;         // the segment pass (fix: a fix-up round) + k_wide_vit_check
    std::function<int()> mend;                 // the far segments again up to a kept vector (empty: no mending)
    std::function<int(double margin)> margins; // k_vit_margin over the path the walks wrote
    std::function<int()> walks;                // back-trace over the segments: maps, stitch, apply
};
constexpr double SEG_VIT_TOL = 1e-12; // boundaries this close count as usable for the margins
struct SegVitResult {
    bool accepted = false;        // the path of the walks is the serial run's (the walks have run)
    bool margin_accepted = false; // ... by the margins of the decisions on it
    int rounds = 0;               // fix-up rounds (max_rounds + 1: they ran out)
};
// seglen: the plan's segment length; maxT: longest_traj; walks_first: the walks follow every pass before its
// verdict is read.  Sets the vit_seg_mismatch, vit_far, vit_mended, vit_margin_used, vit_margin_close and
// vit_seg_rounds counters.
int seg_viterbi(bhmm_ctx *c, const SegViterbi &f, const Segs &sg, int64_t seglen, const double *vall, int64_t maxT,
                int max_rounds, bool walks_first, SegVitResult *res);
int draw_watch_prepare(bhmm_ctx *c, double tol, DrawWatch &w, unsigned int *count_slot);
int draw_verify_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                    unsigned int count, double thr, int64_t Wlong, bool *ok);
// "Watched draws are decided again", for every family: draw_verify_run over a window of 8 x max(spec_W, 64) steps.
// If a decision does not stand, `repeat` -- the caller's draw on exact alpha rows, which records nothing -- runs,
// draw_events and draw_checked stay those of the first draw, draw_redone = 1 and *repeated (its code is returned).
int draw_decide_again(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                      unsigned int count, double thr, const std::function<int()> &repeat, bool *repeated);
// The protocol around the segment-parallel backward draw (wide_sample_run, gen_sample_run) on plan 1 of
// wide_path_plan: alpha rows from forward(false); a watch of 64 x the deviation a segmented forward pass measured
// (none on exact rows); *status_dev cleared; then -- segments_allowed, spec_enabled and more segments than
// trajectories at plan::draw_seglen(total, want_segments) -- the first round and up to plan::DRAW_MAX_ROUNDS fix-up
// rounds, each: reset, poison, pass, k_wide_smp_check, read; else, or if they do not accept, the serial kernel; the
// watched draws of an accepted draw decided again (draw_decide_again), the repeat being a second trip through all
// of this with forward(true).  A hook's BHMM_* code is returned at once.  Two invariants:
//   1. The serial draw never reads speculative rows: if the segmented draw is not accepted and the rows came from a
//      segmented forward pass, forward(true) runs first, draw_fwd_segmented and draw_alpha_dev are cleared and the
//      draws the abandoned rounds recorded are ignored (draw_events stays 0).
//   2. The segmented draw counts as done only if the last round left no mismatching segment AND no round set
//      *status_dev (a draw that found no state may belong to a segment drawn again later); otherwise *status_dev is
//      cleared on the stream before the serial kernel.
// Sets smp_segmented, smp_seg_mismatch (the first round's count), smp_seg_rounds (the round that ended the loop,
// DRAW_MAX_ROUNDS + 1: they ran out), draw_events, draw_checked, draw_redone, draw_fwd_segmented and
// draw_alpha_dev of c->last (both zeroed on exact rows), and ds.smp_W (plan::draw_next_warmup, accepted or not).
struct SegDraw {
    std::function<int(bool exact)> forward;   // alpha rows into d_alpha_rm (exact: the serial recursion); leaves
                                              // last.draw_fwd_segmented / draw_alpha_dev
    std::function<int(const Segs &)> prepare; // what the family's pass needs beyond the driver's buffers (may be empty)
    std::function<int(bool fix, const Segs &, const DrawWatch &)> pass; // the segment kernel (fix: a fix-up round)
    std::function<int()> serial;              // the serial draw kernel
};
int seg_draw(bhmm_ctx *c, const SegDraw &f, const double *A, const double *pi, const double *par0, const double *par1,
             bool segments_allowed, int64_t want_segments, int *status_dev);

// ---- gen_api.hip (more than 64 states) ----
int gen_alloc(bhmm_ctx *c);
int gen_forward(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1);
int gen_backward(bhmm_ctx *c, const double *A);
int gen_estep(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
              double *stats_dev, int flags);
int gen_viterbi_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                    void *paths_out, int out_fmt);
int gen_sample_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                   const double *u, uint64_t seed, int32_t *paths, int64_t *counts, int64_t *n0, double *emis,
                   double *stats_dev);
int gen_transition_counts(double *C, const double *A, const double *pobs, const double *alpha, const double *beta,
                          int N, int64_t T);
int gen_sample_path(int32_t *path, const double *alpha, const double *A, const double *u, int N, int64_t T);

// ---- tile_gen.hip (65..512 states on the row-batched matrix-core kernels) ----
bool tile_gen_capable(const bhmm_ctx *c);
int tile_gen_alloc(bhmm_ctx *c);
int tile_gen_estep(bhmm_ctx *c, const WideModel &m, double *stats_dev, int flags, bool *done);
int tile_gen_forward_draw(bhmm_ctx *c, const WideModel &m, bool *done);

// ---- big_api.hip (more than 128 states, A streamed from L2) ----
int big_launch_fwd(bhmm_ctx *c, const WideModel &m);
int big_launch_bwd(bhmm_ctx *c, const WideModel &m, double *gam, double *stats_dev);

} // namespace bhmm
