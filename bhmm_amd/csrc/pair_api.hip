// pair_api.hip -- bhmm_posterior_transitions: the pair posterior xi_t(i,j) = P(s_t = i, s_t+1 = j | O) of every
// step of every loaded trajectory under one model, as its off-diagonal sum (the probability of a jump at step t)
// or its projection on up to 8 pair weightings, trajectory-major rows in double or float, in a host buffer or left
// in a device buffer of the caller.  Kernels in pair_kernels.hpp; DESIGN.md section 20.
//
// Up to 8 states, gaussian or discrete (the fused path, pair_path 1): k_pair_sweep -- the sweep of k_marg_sweep
// restated as pair_sweep_lane with the pair row hanging off the backward sweep -- over the E-step's chunk plan, the
// alpha rows in a workspace of at most pair_ws_mb, then k_post_check over the boundary vectors of both directions.
// Warm-up from the forgetting probe or the option pair_W.  Boundaries that do not verify: counted in
// pair_fallbacks, the call runs again with twice the warm-up, and if they fail again it takes the generic path
// (plan::two_attempts, plan.hpp; the run around the pass is sweep_host.hpp's, the dispatch on the state count
// fused_host.hpp's; the kernels and one pass over them are compiled per state count, pair_sweep_n.hip).  The option
// pair_fused = 0 never takes this path.
//
// Everything else (9 states and more, explicit pobs, pair_fused 0, a fused call that did not verify; pair_path 0):
// bhmm_filter and bhmm_posterior_marginals through their public entry points, each leaving fp64 rows in a device
// buffer of c->pair, then the row kernel over the steps: k_pair_rows with a device copy of A (one thread
// per step), or k_pair_tile (pair_tile_kernels.hpp, up to 128 states: 16 steps a matrix-core tile, the matrices in its
// operand order formed here and kept like A and W) -- option pair_rows 0 / 1, -1 by class; read-only
// pair_rows_kernel says which one the last generic pass ran; pair_path is 0 for both.  That IS a filter call and a
// marginals call for the context's state, exactly like a caller's own: where bhmm_posterior_marginals takes its
// generic path (9 states and more unless its time-segmented or matrix-core path is on, explicit pobs) that is an
// E-step; on its paths 1 to 3 it touches no other call's state.
//
// The call's buffers are the group c->pair (ctx.hpp), its options opt.pair_* and its counters last.pair_*, like every
// other call's: set and read by bhmm_ctx_set_option / bhmm_ctx_get_option, kept across bhmm_ctx_set_observations,
// freed by bhmm_ctx_destroy.  bhmm_pair_set_option / bhmm_pair_get_option forward the names that begin with pair_
// to those two; bhmm_pair_release frees the group early and puts the seven values back to their defaults.  The fused
// path reads or writes nothing of the context beyond that, the plan, the observations and the stream.  A host result
// is staged in c->pair.out and crosses the link in ONE copy (copy_to_host_pinned, host_internal.hpp).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "model_check.hpp"
#include "pair_launch.hpp"
#include "sweep_host.hpp"

namespace bhmm {
PAIR_PASS_DECL(extern, 1)
PAIR_PASS_DECL(extern, 2)
PAIR_PASS_DECL(extern, 3)
PAIR_PASS_DECL(extern, 4)
PAIR_PASS_DECL(extern, 5)
PAIR_PASS_DECL(extern, 6)
PAIR_PASS_DECL(extern, 7)
PAIR_PASS_DECL(extern, 8)
namespace {

// the fused path; *verified: the rows in o.dev stand
template <int N, int KIND>
int run_fused(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
              const PairOut &o, bool *verified)
{
    return sweep_run<N, KIND>(
        c, c->pair, A, pi, par0, par1, c->opt.pair_W, &c->last.pair_fallbacks,
        [&](const Model<N> *dm, int w, plan::Verdict *v) {
            return pair_pass<N, KIND>(c, dm, w, o, v); // (pair_sweep_n.hip)
        },
        verified);
}

template <int N>
int run_n(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, const PairOut &o,
          bool *verified)
{
    return c->kind == EMIT_GAUSS ? run_fused<N, EMIT_GAUSS>(c, A, pi, par0, par1, o, verified)
                                 : run_fused<N, EMIT_DISC>(c, A, pi, par0, par1, o, verified);
}

// `count` doubles of `fresh` into dev, kept is what dev holds: uploaded only where they differ from the kept copy or
// the buffer was regrown, so repeated calls with the same matrix upload nothing and wait for nothing
int upload_if_changed(bhmm_ctx *c, DevBuf<double> &dev, std::vector<double> &kept, const double *fresh, size_t count)
{
    const bool regrown = count > dev.n;
    if (int rc = dev.ensure(count))
        return rc;
    if (regrown || kept.size() != count || !std::equal(kept.begin(), kept.end(), fresh)) {
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (an earlier upload may still read the kept copy)
        kept.assign(fresh, fresh + count); // (kept: the copy may still be read when this call returns)
        BHMM_HIP(hipMemcpyAsync(dev.p, kept.data(), count * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    return BHMM_OK;
}

// pair_rows -1: k_pair_tile where it was faster than k_pair_rows in EVERY shape measured for the class (DESIGN.md
// section 21: 16, 32, 64 states and 100, 128 states, jump form, Q = 2 and Q = 8), the rule of smooth_wide / smooth_tile
constexpr bool PAIR_TILE_AUTO_WIDE = true; // 9 .. 64 states
constexpr bool PAIR_TILE_AUTO_TILE = true; // 65 .. 128 states

bool tile_takes(const bhmm_ctx *c)
{
    if (c->n > PAIR_TILE_MAX_N || c->opt.pair_rows == 0)
        return false;
    if (c->opt.pair_rows > 0)
        return true;
    return c->n > 64 ? PAIR_TILE_AUTO_TILE : c->n > 8 ? PAIR_TILE_AUTO_WIDE : false;
}

// the generic path: filtered rows and posterior rows by the calls that hand them out, then one kernel over the steps
int generic(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, const PairOut &o)
{
    auto &b = c->pair;
    const bool tile = tile_takes(c);
    c->last.pair_rows_kernel = tile ? 1 : 0;
    if (c->total == 0)
        return BHMM_OK;
    const size_t rows = (size_t)c->total * c->n;
    int rc;
    if ((rc = b.filt.ensure(std::max<size_t>(rows, 2))) || (rc = b.gam.ensure(std::max<size_t>(rows, 2))) ||
        (rc = upload_if_changed(c, b.A, b.A_host, A, (size_t)c->n * c->n)))
        return rc;
    if ((rc = bhmm_filter(c, A, pi, par0, par1, nullptr, 0, b.filt.p, nullptr, BHMM_FILT_DEVICE)) ||
        (rc = bhmm_posterior_marginals(c, A, pi, par0, par1, nullptr, 0, b.gam.p, BHMM_MARG_DEVICE)))
        return rc;
    if (tile) {
        // the matrices in operand order, formed again from A and the padded W of this call: the same A, W, Q and
        // form as the last time give the same vector, and then nothing is uploaded or waited for
        std::vector<double> ops;
        pair_tile_operands(A, o.Q > 0 ? b.W_host.data() : nullptr, c->n, o.Q, ops);
        if ((rc = upload_if_changed(c, b.Bop, b.Bop_host, ops.data(), ops.size())))
            return rc;
        return pair_tile_rows(c, o); // (pair_tile.hip)
    }
    const dim3 grid((unsigned)((c->total + 63) / 64)), block(64);
    if (o.f32)
        BHMM_HIP(launch(k_pair_rows<float>, grid, block, 0, c->stream, b.filt.p, b.gam.p, b.A.p, c->n, c->total, c->K,
                        c->d_offsets.p, o.W, o.Q, static_cast<float *>(o.dev)));
    else
        BHMM_HIP(launch(k_pair_rows<double>, grid, block, 0, c->stream, b.filt.p, b.gam.p, b.A.p, c->n, c->total, c->K,
                        c->d_offsets.p, o.W, o.Q, static_cast<double *>(o.dev)));
    return BHMM_OK;
}

} // namespace
} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_posterior_transitions(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                               const double *W, int Q, void *out, int flags)
{
    int rc = enter_model_call(c, A && pi && out, "A / pi / out == NULL", true, par0, par1);
    if (rc)
        return rc;
    if (flags & ~(BHMM_PAIR_F32 | BHMM_PAIR_DEVICE))
        return invalid_arg("bhmm_posterior_transitions: unknown flag");
    if ((W == nullptr) != (Q == 0) || Q < 0 || Q > PAIR_QMAX)
        return invalid_arg("bhmm_posterior_transitions: W with 1 <= Q <= 8 columns, or W == NULL and Q == 0");
    const bool on_dev = (flags & BHMM_PAIR_DEVICE) != 0;
    if (on_dev && (reinterpret_cast<uintptr_t>(out) & 15))
        return invalid_arg("bhmm_posterior_transitions: a device buffer must be aligned to 16 bytes");
    const size_t wn = (size_t)c->n * c->n * Q;
    for (size_t e = 0; e < wn; ++e)
        if (!std::isfinite(W[e]))
            return invalid_arg("bhmm_posterior_transitions: W has a non-finite entry");
    if ((rc = check_models(c, "bhmm_posterior_transitions", 1, A, pi, par0, par1)))
        return rc;
    auto &b = c->pair;
    PairOut o;
    o.f32 = (flags & BHMM_PAIR_F32) != 0;
    o.Q = Q;
    o.Qp = Q > 0 ? Q : 1;
    o.W = nullptr;
    const size_t bytes = (size_t)c->total * o.Qp * (o.f32 ? sizeof(float) : sizeof(double));
    if (!on_dev && (rc = b.out.ensure(std::max<size_t>(bytes, 16)))) // (BHMM_ERR_NO_MEM: nothing is truncated)
        return rc;
    o.dev = on_dev ? out : static_cast<void *>(b.out.p);
    if (Q > 0) {
        // the kernels read records of PAIR_QMAX columns: the Q given, then zeros
        const size_t pairs = (size_t)c->n * c->n;
        std::vector<double> padded(pairs * PAIR_QMAX, 0.0);
        for (size_t e = 0; e < pairs; ++e)
            std::copy(W + e * Q, W + (e + 1) * Q, padded.begin() + e * PAIR_QMAX);
        if ((rc = upload_if_changed(c, b.W, b.W_host, padded.data(), padded.size())))
            return rc;
        o.W = b.W.p;
    }
    const bool fused = fused_takes(c) && c->opt.pair_fused;
    c->last.pair_path = fused ? 1 : 0;
    bool verified = false;
    if (fused) {
        rc = dispatch_n(c->n, [&](auto N) { return run_n<decltype(N)::value>(c, A, pi, par0, par1, o, &verified); });
        if (rc)
            return rc;
    }
    if (!verified && (rc = generic(c, A, pi, par0, par1, o)))
        return rc;
    if (on_dev) // the rows are where the caller wants them, ordered on the context's stream
        return BHMM_OK;
    return bytes == 0 ? BHMM_OK : copy_to_host_pinned(c, out, o.dev, bytes);
}

// the names of this call's options and counters, by the context's own functions (bhmm_amd.hip)
int bhmm_pair_set_option(bhmm_ctx *c, const char *name, double value)
{
    if (!c || !name)
        return invalid_arg("bhmm_pair_set_option: ctx / name == NULL");
    if (strncmp(name, "pair_", 5) != 0)
        return invalid_arg(std::string("unknown or read-only option: ") + name);
    return bhmm_ctx_set_option(c, name, value);
}

int bhmm_pair_get_option(bhmm_ctx *c, const char *name, double *value)
{
    if (!c || !name || !value)
        return invalid_arg("bhmm_pair_get_option: ctx / name / value == NULL");
    if (strncmp(name, "pair_", 5) != 0)
        return invalid_arg(std::string("unknown option: ") + name);
    return bhmm_ctx_get_option(c, name, value);
}

// frees c->pair and puts opt.pair_* / last.pair_* back to their defaults: the next call works as on a fresh context
int bhmm_pair_release(bhmm_ctx *c)
{
    if (!c)
        return BHMM_OK;
    BHMM_HIP(hipSetDevice(c->device));
    BHMM_HIP(hipStreamSynchronize(c->stream)); // (a kernel or an upload may still use the buffers and the kept copies)
    using PairBufs = bhmm_ctx::PairBufs;
    c->pair.~PairBufs();
    new (&c->pair) PairBufs();
    const bhmm_ctx::Options opt;
    c->opt.pair_W = opt.pair_W;
    c->opt.pair_ws_mb = opt.pair_ws_mb;
    c->opt.pair_fused = opt.pair_fused;
    c->opt.pair_rows = opt.pair_rows;
    const bhmm_ctx::LastCall last;
    c->last.pair_fallbacks = last.pair_fallbacks;
    c->last.pair_path = last.pair_path;
    c->last.pair_rows_kernel = last.pair_rows_kernel;
    return BHMM_OK;
}

} // extern "C"
