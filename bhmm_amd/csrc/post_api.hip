// post_api.hip -- bhmm_posterior_decode: for every step of every loaded trajectory the state of largest
// posterior marginal, argmax_i gamma_t(i), and optionally that marginal.  Kernels in post_kernels.hpp;
// DESIGN.md section 14.
//
// Up to 8 states, gaussian or discrete (the fused path, post_path 1): k_post_sweep over the E-step's chunk
// plan, forward and backward in one launch per range of chunk groups, the alpha rows in a workspace of
// at most post_ws_mb (the host loops over ranges of groups; every lane's arithmetic is its own, so the result
// does not depend on the budget), then k_post_check over the boundary vectors of both directions.  The warm-up
// comes from the forgetting probe of the E-step (k_forget_probe, the larger of its two directions) or the
// option post_W.  Boundaries that do not verify: counted in post_fallbacks, the call runs again with twice
// the warm-up, and if they fail again it takes the generic path (plan::two_attempts, plan.hpp; the pass and the run
// around it are sweep_host.hpp's, shared with bhmm_posterior_marginals and bhmm_posterior_transitions; the model
// upload, the probe and the dispatch on the state count are fused_host.hpp's, shared with bhmm_score and bhmm_filter
// too).
//
// 9 to 64 states, gaussian or discrete (the time-segmented path, post_path 2; smooth_wide.hip):
// k_filter_wide leaves the filtered rows of a range of segments in a workspace of at most smooth_ws_mb,
// k_smooth_wide_bwd walks the same segments back and decodes; both directions are checked, the same protocol.  A
// segment of probability zero or a NaN observation: the generic path answers.  Taken when the option smooth_wide is
// 1, or -1 (the default) where smooth_wide_auto allows it and the set has at least SMOOTH_WIDE_MIN_TOTAL steps.  It
// touches c->smooth.* alone and delivers through c->post.path / conf.
//
// 65 to 128 states, gaussian or discrete (the matrix-core path, post_path 3; smooth_tile.hip):
// k_filter_tile leaves the filtered rows of a range of segments in a workspace of at most smooth_ws_mb,
// k_smooth_tile_bwd walks the same segments back on the matrix cores and decodes; both directions are checked, the
// same protocol.  A segment either kernel flags (probability zero, an outlier, a NaN observation): the generic path
// answers for the whole call.  Taken when the option smooth_tile is 1, or -1 (the default) where smooth_tile_auto
// allows it and the set has at least SMOOTH_TILE_MIN_TOTAL steps.  It touches c->smooth_tile.* alone and delivers
// through c->post.path / conf.
//
// Everything else (9 states and more unless a path above is taken, explicit pobs; post_path 0): bhmm_estep with BHMM_FLAG_STORE_GAMMA
// through its own entry point and protocol, then k_post_gamma_rm / k_post_gamma_ci over the stored rows.
// That IS an E-step for the context's state (statistics, carried boundaries, timers, stored gamma), exactly
// like a caller's own.
//
// The fused path reads or writes nothing of the E-step's state (ds.*, carried vectors, warm-up lengths,
// d_Bt, the timing events, the pinned landing zones): its buffers are c->post.*, the only other fields
// touched are opt.post_* (read) and last.post_*.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "model_check.hpp"
#include "smooth_tile_api.hpp"
#include "smooth_wide_launch.hpp"
#include "sweep_host.hpp"

namespace bhmm {
namespace {

// the results on the device to the caller: the paths as deliver_paths does, the confidences after them
int deliver(bhmm_ctx *c, void *path, int path_u8, float *conf)
{
    auto &b = c->post;
    if (conf)
        BHMM_HIP(hipMemcpyAsync(conf, b.conf.p, (size_t)c->total * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return deliver_paths(c, path, path_u8 ? 1 : 0, b.path.p);
}

template <int N, int KIND, typename PT>
int pass_as(bhmm_ctx *c, const Model<N> *dm, int W, bool want_conf, plan::Verdict *v)
{
    auto &b = c->post;
    return sweep_pass<N, KIND>(c, b, c->opt.post_ws_mb, dm, W, b.Bt.p, k_post_sweep<N, KIND, true, PT>,
                               k_post_sweep<N, KIND, false, PT>, v, reinterpret_cast<PT *>(b.path.p),
                               want_conf ? b.conf.p : nullptr);
}

// the fused path; *verified: the outputs in c->post.path / conf stand
template <int N, int KIND>
int run_fused(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, int path_u8,
              bool want_conf, bool *verified)
{
    return sweep_run<N, KIND>(
        c, c->post, A, pi, par0, par1, c->opt.post_W, &c->last.post_fallbacks,
        [&](const Model<N> *dm, int w, plan::Verdict *v) {
            return path_u8 ? pass_as<N, KIND, uint8_t>(c, dm, w, want_conf, v)
                           : pass_as<N, KIND, int32_t>(c, dm, w, want_conf, v);
        },
        verified);
}

template <int N>
int run_n(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, int path_u8,
          bool want_conf, bool *verified)
{
    return c->kind == EMIT_GAUSS ? run_fused<N, EMIT_GAUSS>(c, A, pi, par0, par1, path_u8, want_conf, verified)
                                 : run_fused<N, EMIT_DISC>(c, A, pi, par0, par1, path_u8, want_conf, verified);
}

// the generic path: an E-step that stores gamma, then argmax / max over the rows in the layout the
// kernel family of this context stores them in
template <typename PT>
int gamma_decode(bhmm_ctx *c, bool want_conf)
{
    auto &b = c->post;
    PT *path = reinterpret_cast<PT *>(b.path.p);
    float *conf = want_conf ? b.conf.p : nullptr;
    if (c->total == 0)
        return BHMM_OK;
    if (c->wide || c->gen) { // trajectory-major rows of n
        BHMM_HIP(launch(k_post_gamma_rm<PT>, dim3((unsigned)((c->total + 255) / 256)), dim3(256), 0, c->stream,
                        c->d_gamma_ci.p, c->n, c->total, path, conf));
        return BHMM_OK;
    }
    const Chunks ch = chunks_of(c); // (the plan the E-step ended on)
    const dim3 grid((c->G + 255) / 256), block(256);
    if (c->N == 2)
        BHMM_HIP(launch(k_post_gamma_ci<2, PT>, grid, block, 0, c->stream, ch, c->G, c->d_gamma_ci.p, c->n, path, conf));
    else if (c->N == 4)
        BHMM_HIP(launch(k_post_gamma_ci<4, PT>, grid, block, 0, c->stream, ch, c->G, c->d_gamma_ci.p, c->n, path, conf));
    else
        BHMM_HIP(launch(k_post_gamma_ci<8, PT>, grid, block, 0, c->stream, ch, c->G, c->d_gamma_ci.p, c->n, path, conf));
    return BHMM_OK;
}

int generic(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, int path_u8,
            bool want_conf)
{
    int rc;
    if ((rc = bhmm_estep(c, A, pi, par0, par1, nullptr, BHMM_FLAG_STORE_GAMMA)) ||
        (rc = bhmm_estep_fetch(c, nullptr, nullptr))) // (waits; a non-finite log-likelihood is its error)
        return rc;
    return path_u8 ? gamma_decode<uint8_t>(c, want_conf) : gamma_decode<int32_t>(c, want_conf);
}

} // namespace

// decode into c->post.path / conf (host_internal.hpp); bhmm_posterior_decode delivers them, bhmm_decode_runs
// compacts the path on the device
int post_decode_device(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                       bool given, int path_u8, bool conf)
{
    int rc = enter_model_call(c, given, "A / pi / path == NULL", true, par0, par1);
    if (rc)
        return rc;
    if (path_u8 && c->n > 256)
        return invalid_arg("bhmm_posterior_decode: one byte per step holds at most 256 states (use the int32 form)");
    if ((rc = check_models(c, "bhmm_posterior_decode", 1, A, pi, par0, par1)))
        return rc;
    auto &b = c->post;
    if ((rc = b.path.ensure(std::max<size_t>((size_t)c->total * (path_u8 ? 1 : sizeof(int32_t)), 8))) ||
        (conf && (rc = b.conf.ensure(std::max<size_t>(c->total, 1)))))
        return rc;
    const bool fused = fused_takes(c);
    const int form = conf ? SMOOTH_FORM_DECODE_CONF : SMOOTH_FORM_DECODE;
    const bool segs = smooth_wide_takes(c, form), tile = smooth_tile_takes(c, form);
    c->last.post_path = fused ? 1 : (segs ? 2 : (tile ? 3 : 0));
    c->last.smooth_segments = 0;
    bool verified = false;
    if (segs || tile) {
        SmoothWideOut o;
        o.form = form;
        o.out = b.path.p;
        o.narrow = path_u8 != 0;
        o.conf = conf ? b.conf.p : nullptr;
        o.V = nullptr;
        o.Q = 0;
        if ((rc = tile ? smooth_tile_run(c, A, pi, par0, par1, o, &c->last.post_fallbacks, &verified)
                       : smooth_wide_run(c, A, pi, par0, par1, o, &c->last.post_fallbacks, &verified)))
            return rc;
    } else if (fused) {
        rc = dispatch_n(c->n, [&](auto N) {
            return run_n<decltype(N)::value>(c, A, pi, par0, par1, path_u8, conf, &verified);
        });
        if (rc)
            return rc;
    }
    if (!verified && (rc = generic(c, A, pi, par0, par1, path_u8, conf)))
        return rc;
    return BHMM_OK;
}

} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_posterior_decode(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                          void *path, int path_u8, float *conf)
{
    if (int rc = post_decode_device(c, A, pi, par0, par1, A && pi && path, path_u8, conf != nullptr))
        return rc;
    return deliver(c, path, path_u8, conf);
}

} // extern "C"
