// marg_api.hip -- bhmm_posterior_marginals: the posterior probability of every hidden state at every step of
// every loaded trajectory, gamma_t(i), or its projection on up to 8 columns, as trajectory-major rows in
// double or float, in a host buffer or left in a device buffer of the caller.  Kernels in marg_kernels.hpp;
// DESIGN.md section 15.
//
// Up to 8 states, gaussian or discrete (the fused path, marg_path 1): k_marg_sweep -- the sweep of k_post_sweep
// (restated as marg_sweep_lane, marg_kernels.hpp) with the emit policy MargRow -- over the E-step's chunk plan,
// the alpha rows in a workspace of at most marg_ws_mb, then k_post_check over the boundary vectors of both directions.
// Warm-up from the forgetting probe or the option marg_W.  Boundaries that do not verify: counted in
// marg_fallbacks, the call runs again with twice the warm-up, and if they fail again it takes the generic path
// (plan::two_attempts, plan.hpp; the pass and the run around it are sweep_host.hpp's, shared with
// bhmm_posterior_decode and bhmm_posterior_transitions; the model upload, the probe and the dispatch on the state
// count are fused_host.hpp's, shared with bhmm_score and bhmm_filter too).
//
// 9 to 64 states, gaussian or discrete (the time-segmented path, marg_path 2; smooth_wide.hip):
// k_filter_wide leaves the filtered rows of a range of segments in a workspace of at most smooth_ws_mb,
// k_smooth_wide_bwd walks the same segments back and writes the rows or their projection (summed by the DPP tree of
// wgroup_sum, not in ascending state order); both directions are checked, the same protocol.  A segment of
// probability zero or a NaN observation: the generic path answers.  Taken when the option smooth_wide is 1, or -1
// (the default) where smooth_wide_auto allows it and the set has at least SMOOTH_WIDE_MIN_TOTAL steps.  It touches
// c->smooth.* alone and writes to c->marg.out or the caller's device buffer.
//
// 65 to 128 states, gaussian or discrete (the matrix-core path, marg_path 3; smooth_tile.hip):
// k_filter_tile forward into a workspace of at most smooth_ws_mb, k_smooth_tile_bwd backward on the matrix cores,
// which writes the rows or their projection (summed by the tree of row16_sum, not in ascending state order); both
// directions are checked, the same protocol.  A segment either kernel flags: the generic path answers for the whole
// call.  Taken when the option smooth_tile is 1, or -1 (the default) where smooth_tile_auto allows it and the set
// has at least SMOOTH_TILE_MIN_TOTAL steps.  It touches c->smooth_tile.* alone and writes to c->marg.out or the
// caller's device buffer.
//
// Everything else (9 states and more unless a path above is taken, explicit pobs; marg_path 0): bhmm_estep with BHMM_FLAG_STORE_GAMMA
// through its own entry point and protocol, then k_marg_rows_rm / k_marg_rows_ci over the stored rows.  That IS
// an E-step for the context's state (statistics, carried boundaries, timers, stored gamma), exactly like a
// caller's own.
//
// The fused path reads or writes nothing of the E-step's state and nothing of c->post.*: its buffers are
// c->marg.*, the only other fields touched are opt.marg_* (read) and last.marg_*.  A host result is staged in
// c->marg.out and crosses the link in ONE copy (copy_to_host_pinned, host_internal.hpp).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "marg_kernels.hpp"
#include "model_check.hpp"
#include "smooth_tile_api.hpp"
#include "smooth_wide_launch.hpp"
#include "sweep_host.hpp"

namespace bhmm {
namespace {

struct Out {          // where the rows go on the device, and what they are
    void *dev;        // [total][Qp] of double / float
    const double *V;  // device copy of the projection, or nullptr
    int Q;            // its columns (0: none)
    int Qp;           // values per row
    bool f32;
};

template <int N, int KIND, typename OT, bool PROJ>
int pass_as(bhmm_ctx *c, const Model<N> *dm, int W, const Out &o, plan::Verdict *v)
{
    auto &b = c->marg;
    return sweep_pass<N, KIND>(c, b, c->opt.marg_ws_mb, dm, W, b.Bt.p, k_marg_sweep<N, KIND, true, OT, PROJ>,
                               k_marg_sweep<N, KIND, false, OT, PROJ>, v, static_cast<OT *>(o.dev), o.V, o.Q);
}

// the fused path; *verified: the rows in o.dev stand
template <int N, int KIND>
int run_fused(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, const Out &o,
              bool *verified)
{
    return sweep_run<N, KIND>(
        c, c->marg, A, pi, par0, par1, c->opt.marg_W, &c->last.marg_fallbacks,
        [&](const Model<N> *dm, int w, plan::Verdict *v) {
            if (o.Q > 0)
                return o.f32 ? pass_as<N, KIND, float, true>(c, dm, w, o, v)
                             : pass_as<N, KIND, double, true>(c, dm, w, o, v);
            return o.f32 ? pass_as<N, KIND, float, false>(c, dm, w, o, v)
                         : pass_as<N, KIND, double, false>(c, dm, w, o, v);
        },
        verified);
}

template <int N>
int run_n(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, const Out &o,
          bool *verified)
{
    return c->kind == EMIT_GAUSS ? run_fused<N, EMIT_GAUSS>(c, A, pi, par0, par1, o, verified)
                                 : run_fused<N, EMIT_DISC>(c, A, pi, par0, par1, o, verified);
}

// the generic path: an E-step that stores gamma, then one kernel that converts / projects the rows in the
// layout the kernel family of this context stores them in
template <typename OT>
int gamma_rows(bhmm_ctx *c, const Out &o)
{
    OT *out = static_cast<OT *>(o.dev);
    if (c->total == 0)
        return BHMM_OK;
    if (c->wide || c->gen) { // trajectory-major rows of n
        const int64_t threads = o.Q > 0 ? c->total : c->total * c->n;
        BHMM_HIP(launch(k_marg_rows_rm<OT>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c->stream,
                        c->d_gamma_ci.p, c->n, c->total, o.V, o.Q, out));
        return BHMM_OK;
    }
    const Chunks ch = chunks_of(c); // (the plan the E-step ended on)
    const dim3 grid((c->G + 255) / 256), block(256);
    if (c->N == 2)
        BHMM_HIP(launch(k_marg_rows_ci<2, OT>, grid, block, 0, c->stream, ch, c->G, c->d_gamma_ci.p, c->n, o.V, o.Q, out));
    else if (c->N == 4)
        BHMM_HIP(launch(k_marg_rows_ci<4, OT>, grid, block, 0, c->stream, ch, c->G, c->d_gamma_ci.p, c->n, o.V, o.Q, out));
    else
        BHMM_HIP(launch(k_marg_rows_ci<8, OT>, grid, block, 0, c->stream, ch, c->G, c->d_gamma_ci.p, c->n, o.V, o.Q, out));
    return BHMM_OK;
}

int generic(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, const Out &o)
{
    int rc;
    if ((rc = bhmm_estep(c, A, pi, par0, par1, nullptr, BHMM_FLAG_STORE_GAMMA)) ||
        (rc = bhmm_estep_fetch(c, nullptr, nullptr))) // (waits; a non-finite log-likelihood is its error)
        return rc;
    return o.f32 ? gamma_rows<float>(c, o) : gamma_rows<double>(c, o);
}

// the staged rows to the caller's host buffer in one copy
int deliver(bhmm_ctx *c, void *host, const void *dev, size_t bytes)
{
    return bytes == 0 ? BHMM_OK : copy_to_host_pinned(c, host, dev, bytes);
}

} // namespace
} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_posterior_marginals(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                             const double *V, int Q, void *out, int flags)
{
    int rc = enter_model_call(c, A && pi && out, "A / pi / out == NULL", true, par0, par1);
    if (rc)
        return rc;
    if (flags & ~(BHMM_MARG_F32 | BHMM_MARG_DEVICE))
        return invalid_arg("bhmm_posterior_marginals: unknown flag");
    if ((V == nullptr) != (Q == 0) || Q < 0 || Q > MARG_QMAX)
        return invalid_arg("bhmm_posterior_marginals: V with 1 <= Q <= 8 columns, or V == NULL and Q == 0");
    const bool on_dev = (flags & BHMM_MARG_DEVICE) != 0;
    if (on_dev && (reinterpret_cast<uintptr_t>(out) & 15))
        return invalid_arg("bhmm_posterior_marginals: a device buffer must be aligned to 16 bytes");
    for (int e = 0; e < c->n * Q; ++e)
        if (!std::isfinite(V[e]))
            return invalid_arg("bhmm_posterior_marginals: V has a non-finite entry");
    if ((rc = check_models(c, "bhmm_posterior_marginals", 1, A, pi, par0, par1)))
        return rc;
    auto &b = c->marg;
    Out o;
    o.f32 = (flags & BHMM_MARG_F32) != 0;
    o.Q = Q;
    o.Qp = Q > 0 ? Q : c->n;
    o.V = nullptr;
    const size_t bytes = (size_t)c->total * o.Qp * (o.f32 ? sizeof(float) : sizeof(double));
    if (!on_dev && (rc = b.out.ensure(std::max<size_t>(bytes, 16)))) // (BHMM_ERR_NO_MEM: nothing is truncated)
        return rc;
    o.dev = on_dev ? out : static_cast<void *>(b.out.p);
    if (Q > 0) {
        if ((rc = b.V.ensure((size_t)std::max(c->n, 8) * MARG_QMAX)))
            return rc;
        BHMM_HIP(hipMemcpyAsync(b.V.p, V, (size_t)c->n * Q * sizeof(double), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (V may be a temporary of the caller's)
        o.V = b.V.p;
    }
    const bool fused = fused_takes(c);
    const int form = Q > 0 ? SMOOTH_FORM_PROJ : SMOOTH_FORM_ROWS;
    const bool segs = smooth_wide_takes(c, form), tile = smooth_tile_takes(c, form);
    c->last.marg_path = fused ? 1 : (segs ? 2 : (tile ? 3 : 0));
    c->last.smooth_segments = 0;
    bool verified = false;
    if (segs || tile) {
        SmoothWideOut so;
        so.form = form;
        so.out = o.dev;
        so.narrow = o.f32;
        so.conf = nullptr;
        so.V = o.V;
        so.Q = Q;
        if ((rc = tile ? smooth_tile_run(c, A, pi, par0, par1, so, &c->last.marg_fallbacks, &verified)
                       : smooth_wide_run(c, A, pi, par0, par1, so, &c->last.marg_fallbacks, &verified)))
            return rc;
    } else if (fused) {
        rc = dispatch_n(c->n, [&](auto N) { return run_n<decltype(N)::value>(c, A, pi, par0, par1, o, &verified); });
        if (rc)
            return rc;
    }
    if (!verified && (rc = generic(c, A, pi, par0, par1, o)))
        return rc;
    if (on_dev) { // the rows are where the caller wants them, ordered on the context's stream
        return BHMM_OK;
    }
    return deliver(c, out, o.dev, bytes);
}

} // extern "C"
