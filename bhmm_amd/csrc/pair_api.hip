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
// (plan::two_attempts, plan.hpp; the model upload, the probe and the dispatch on the state count are
// fused_host.hpp's; the kernels and one pass over them are compiled per state count, pair_sweep_n.hip).  The option
// pair_fused = 0 never takes this path.
//
// Everything else (9 states and more, explicit pobs, pair_fused 0, a fused call that did not verify; pair_path 0):
// bhmm_filter and bhmm_posterior_marginals through their public entry points, each leaving fp64 rows in a device
// buffer of the call's own state, then the row kernel over the steps: k_pair_rows with a device copy of A (one thread
// per step), or k_pair_tile (pair_tile_kernels.hpp, up to 128 states: 16 steps a matrix-core tile, the matrices in its
// operand order formed here and kept like A and W) -- option pair_rows 0 / 1, -1 by class; read-only
// pair_rows_kernel says which one the last generic pass ran; pair_path is 0 for both.  That IS a filter call and a
// marginals call for the context's state, exactly like a caller's own: where bhmm_posterior_marginals takes its
// generic path (9 states and more unless its time-segmented or matrix-core path is on, explicit pobs) that is an
// E-step; on its paths 1 to 3 it touches no other call's state.
//
// The call's buffers, options and counters are a PairState (pair_launch.hpp) that this unit keeps BESIDE the context,
// one per context in a table keyed by its address, made at the first call or the first option SET and released by
// bhmm_pair_release (which the owner of the context calls before bhmm_ctx_destroy) -- not a group in ctx.hpp: the
// context and every other unit are then exactly what they were before this call existed.  The options are therefore
// set and read by bhmm_pair_set_option / bhmm_pair_get_option, not by the tables of bhmm_ctx_set_option.  A state
// that was never released and is found again under the address of a NEW context (another device or stream) is
// discarded before use, its buffers freed on the device they were made on; the table itself is never destroyed, so
// nothing is freed after the HIP runtime has gone at process exit.  The fused
// path reads or writes nothing of the context beyond the plan, the observations and the stream.  A host result is
// staged in the state's out buffer and crosses the link in ONE copy (copy_to_host_pinned, host_internal.hpp).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "fused_host.hpp"
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "model_check.hpp"
#include "pair_launch.hpp"

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

// the state of every context that has made a pair call or set a pair option.  The table is allocated once and
// never destroyed: a static destructor would free device buffers after the HIP runtime
using PairTable = std::unordered_map<const bhmm_ctx *, std::unique_ptr<PairState>>;
std::mutex g_pair_mutex;
PairTable &pair_table()
{
    static PairTable *table = new PairTable();
    return *table;
}

// frees the buffers of a state on the device they were allocated on, then makes c's device current again
void drop_state(std::unique_ptr<PairState> gone, const bhmm_ctx *c)
{
    if (!gone)
        return;
    if (gone->device >= 0)
        (void)hipSetDevice(gone->device);
    (void)hipDeviceSynchronize();
    gone.reset();
    (void)hipSetDevice(c->device);
    (void)hipGetLastError();
}

// the state of c; nullptr if it has none and create is false.  A state left by a context that is gone is dropped
PairState *pair_state(const bhmm_ctx *c, bool create)
{
    std::unique_ptr<PairState> stale;
    PairState *found = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_pair_mutex);
        PairTable &t = pair_table();
        auto it = t.find(c);
        if (it != t.end() && (it->second->device != c->device || it->second->stream != c->stream)) {
            stale = std::move(it->second);
            t.erase(it);
            it = t.end();
        }
        if (it != t.end()) {
            found = it->second.get();
        } else if (create) {
            auto &slot = t[c];
            slot.reset(new PairState());
            slot->device = c->device;
            slot->stream = c->stream;
            found = slot.get();
        }
    }
    drop_state(std::move(stale), c);
    return found;
}

template <int N, int KIND>
struct Fused {
    // *verified: the rows in o.dev stand
    static int run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                   PairState &b, const PairOut &o, bool *verified)
    {
        *verified = false;
        Model<N> m;
        int rc;
        if ((rc = b.aentry.ensure((size_t)c->Gp * N)) || (rc = b.aexit.ensure((size_t)c->Gp * N)) ||
            (rc = b.bassumed.ensure((size_t)c->Gp * N)) || (rc = b.bout.ensure((size_t)c->Gp * N)) ||
            (rc = b.dead.ensure(c->Gp)) || (rc = b.fails.ensure(1)) ||
            (rc = upload_fused_model<N, KIND>(c, b.model, b.Bt, A, pi, par0, par1, m)))
            return rc;
        const Model<N> *dm = reinterpret_cast<const Model<N> *>(b.model.p);
        // the larger of the two directions of the forgetting probe
        int W = b.opt_W;
        if (W <= 0 && (rc = fused_probe<N, KIND>(c, b.probe, m, b.Bt.p, true, &W)))
            return rc;
        return plan::two_attempts(
            W, 1 << 30, &b.fallbacks,
            [&](int w, plan::Verdict *v) {
                return pair_pass<N, KIND>(c, b, dm, w, b.Bt.p, o, v); // (pair_sweep_n.hip)
            },
            verified);
    }
};

template <int N>
int run_n(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, PairState &b,
          const PairOut &o, bool *verified)
{
    return c->kind == EMIT_GAUSS ? Fused<N, EMIT_GAUSS>::run(c, A, pi, par0, par1, b, o, verified)
                                 : Fused<N, EMIT_DISC>::run(c, A, pi, par0, par1, b, o, verified);
}

// pair_rows -1: k_pair_tile where it was faster than k_pair_rows in EVERY shape measured for the class (DESIGN.md
// section 21: 16, 32, 64 states and 100, 128 states, jump form, Q = 2 and Q = 8), the rule of smooth_wide / smooth_tile
constexpr bool PAIR_TILE_AUTO_WIDE = true; // 9 .. 64 states
constexpr bool PAIR_TILE_AUTO_TILE = true; // 65 .. 128 states

bool tile_takes(const bhmm_ctx *c, const PairState &b)
{
    if (c->n > PAIR_TILE_MAX_N || b.opt_rows == 0)
        return false;
    if (b.opt_rows > 0)
        return true;
    return c->n > 64 ? PAIR_TILE_AUTO_TILE : c->n > 8 ? PAIR_TILE_AUTO_WIDE : false;
}

// the generic path: filtered rows and posterior rows by the calls that hand them out, then one kernel over the steps
int generic(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1, PairState &b,
            const PairOut &o)
{
    const bool tile = tile_takes(c, b);
    b.rows_kernel = tile ? 1 : 0;
    if (c->total == 0)
        return BHMM_OK;
    const size_t rows = (size_t)c->total * c->n;
    int rc;
    if ((rc = b.filt.ensure(std::max<size_t>(rows, 2))) || (rc = b.gam.ensure(std::max<size_t>(rows, 2))) ||
        (rc = b.A.ensure((size_t)c->n * c->n)))
        return rc;
    if (b.A_host.size() != (size_t)c->n * c->n || !std::equal(b.A_host.begin(), b.A_host.end(), A)) {
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (an earlier upload may still read the kept copy)
        b.A_host.assign(A, A + (size_t)c->n * c->n); // (kept: the copy may still be read when this call returns)
        BHMM_HIP(hipMemcpyAsync(b.A.p, b.A_host.data(), b.A_host.size() * sizeof(double), hipMemcpyHostToDevice,
                                c->stream));
    }
    if ((rc = bhmm_filter(c, A, pi, par0, par1, nullptr, 0, b.filt.p, nullptr, BHMM_FILT_DEVICE)) ||
        (rc = bhmm_posterior_marginals(c, A, pi, par0, par1, nullptr, 0, b.gam.p, BHMM_MARG_DEVICE)))
        return rc;
    if (tile) {
        // the matrices in operand order, formed again from A and the padded W of this call: the same A, W, Q and
        // form as the last time give the same vector, and then nothing is uploaded or waited for
        std::vector<double> ops;
        pair_tile_operands(A, o.Q > 0 ? b.W_host.data() : nullptr, c->n, o.Q, ops);
        const bool regrown = ops.size() > b.Bop.n;
        if ((rc = b.Bop.ensure(ops.size())))
            return rc;
        if (regrown || ops != b.Bop_host) {
            BHMM_HIP(hipStreamSynchronize(c->stream)); // (an earlier upload may still read the kept copy)
            b.Bop_host.swap(ops); // (kept: the copy may still be read when this call returns)
            BHMM_HIP(hipMemcpyAsync(b.Bop.p, b.Bop_host.data(), b.Bop_host.size() * sizeof(double),
                                    hipMemcpyHostToDevice, c->stream));
        }
        return pair_tile_rows(c, b, o); // (pair_tile.hip)
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
    PairState &b = *pair_state(c, true);
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
        const bool regrown = padded.size() > b.W.n;
        if ((rc = b.W.ensure(padded.size())))
            return rc;
        if (regrown || padded != b.W_host) { // (repeated calls with the same weights upload nothing)
            BHMM_HIP(hipStreamSynchronize(c->stream)); // (an earlier upload may still read the kept copy)
            b.W_host.swap(padded); // (kept: the copy may still be read when this call returns)
            BHMM_HIP(hipMemcpyAsync(b.W.p, b.W_host.data(), b.W_host.size() * sizeof(double), hipMemcpyHostToDevice,
                                    c->stream));
        }
        o.W = b.W.p;
    }
    const bool fused = fused_takes(c) && b.opt_fused;
    b.path = fused ? 1 : 0;
    bool verified = false;
    if (fused) {
        rc = dispatch_n(c->n, [&](auto N) { return run_n<decltype(N)::value>(c, A, pi, par0, par1, b, o, &verified); });
        if (rc)
            return rc;
    }
    if (!verified && (rc = generic(c, A, pi, par0, par1, b, o)))
        return rc;
    if (on_dev) // the rows are where the caller wants them, ordered on the context's stream
        return BHMM_OK;
    return bytes == 0 ? BHMM_OK : copy_to_host_pinned(c, out, o.dev, bytes);
}

int bhmm_pair_set_option(bhmm_ctx *c, const char *name, double value)
{
    if (!c || !name)
        return invalid_arg("bhmm_pair_set_option: ctx / name == NULL");
    const std::string n(name);
    PairState &b = *pair_state(c, true);
    if (n == "pair_W") // fixed warm-up (0: measured)
        b.opt_W = std::max(0, (int)value);
    else if (n == "pair_ws_mb") { // budget of the alpha-row workspace in MiB (0: unbounded)
        if (!(value >= 0.0) || value > (double)(1 << 30))
            return invalid_arg("pair_ws_mb outside [0, 2^30]");
        b.opt_ws_mb = (int)value;
    } else if (n == "pair_fused") // 0: never the fused path (the generic route answers every call)
        b.opt_fused = value != 0.0;
    else if (n == "pair_rows") { // row kernel of the generic path: 0 k_pair_rows, 1 k_pair_tile (n <= 128), -1 by class
        if (value != -1.0 && value != 0.0 && value != 1.0)
            return invalid_arg("pair_rows is -1, 0 or 1");
        b.opt_rows = (int)value;
    } else
        return invalid_arg("unknown or read-only option: " + n);
    return BHMM_OK;
}

int bhmm_pair_get_option(bhmm_ctx *c, const char *name, double *value)
{
    if (!c || !name || !value)
        return invalid_arg("bhmm_pair_get_option: ctx / name / value == NULL");
    const std::string n(name);
    const PairState fresh; // (a context that made no pair call and set no option: the defaults, nothing is kept)
    const PairState *have = pair_state(c, false);
    const PairState &b = have ? *have : fresh;
    if (n == "pair_W")
        *value = b.opt_W;
    else if (n == "pair_ws_mb")
        *value = b.opt_ws_mb;
    else if (n == "pair_fused")
        *value = b.opt_fused ? 1.0 : 0.0;
    else if (n == "pair_fallbacks") // calls whose boundaries did not verify at the first warm-up
        *value = b.fallbacks;
    else if (n == "pair_path") // first pass of the last call: 1 fused kernel, 0 filter + marginals + pair rows
        *value = b.path;
    else if (n == "pair_rows")
        *value = b.opt_rows;
    else if (n == "pair_rows_kernel") // row kernel of the last generic pass: 0 k_pair_rows, 1 k_pair_tile
        *value = b.rows_kernel;
    else
        return invalid_arg("unknown option: " + n);
    return BHMM_OK;
}

int bhmm_pair_release(bhmm_ctx *c)
{
    if (!c)
        return BHMM_OK;
    std::unique_ptr<PairState> gone;
    {
        std::lock_guard<std::mutex> lock(g_pair_mutex);
        PairTable &t = pair_table();
        auto it = t.find(c);
        if (it == t.end())
            return BHMM_OK;
        gone = std::move(it->second);
        t.erase(it);
    }
    drop_state(std::move(gone), c); // (waits for the device, frees the buffers where they were made)
    return BHMM_OK;
}

} // extern "C"
