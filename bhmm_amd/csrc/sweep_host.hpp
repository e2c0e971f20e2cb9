// sweep_host.hpp -- the host code around a two-sided sweep kernel for up to 8 states (k_post_sweep, k_marg_sweep,
// k_pair_sweep: the fused paths of bhmm_posterior_decode, bhmm_posterior_marginals and bhmm_posterior_transitions):
// one verified pass over the ranges of chunk groups (sweep_pass) and the run around it -- sizing, model upload,
// warm-up, the two attempts (sweep_run).  Each unit passes its SweepBufs (ctx.hpp), its option values and its
// counter, and keeps the choice of its kernel's instantiation and the output arguments of that kernel.  The rest of
// the scaffold is fused_host.hpp's.
#pragma once
#include <algorithm>

#include "fused_host.hpp"
#include "post_kernels.hpp"

namespace bhmm {

// The sweep over every range of chunk groups at warm-up W and the check; *v: failed with boundaries out of tolerance.
// The alpha rows of a range sit in a workspace of at most ws_mb MiB (0: unbounded; every lane's arithmetic is its own,
// so the result does not depend on the budget).  lds / global: the kernel with B^T in LDS and with B^T in global
// memory; mid: its arguments between the workspace and the boundary vectors
template <int N, int KIND, typename... P, typename... Mid>
int sweep_pass(bhmm_ctx *c, SweepBufs &b, int ws_mb, const Model<N> *dm, int W, const double *dBt, void (*lds)(P...),
               void (*global)(P...), plan::Verdict *v, Mid... mid)
{
    unsigned int fails = 0;
    const int G = c->G, groups = c->Gp / 64;
    const Chunks ch = chunks_of(c);
    const size_t lds_bt = (size_t)c->M * score_bt_stride(N) * sizeof(double);
    const bool bt_lds = KIND == EMIT_DISC && lds_bt <= LDS_BT_MAX;
    // alpha rows of one group, and how many groups the budget holds (at least one)
    const size_t per_group = (size_t)c->Lmax * N * 64 * sizeof(double);
    const size_t budget = (size_t)ws_mb << 20;
    const int per_range =
        budget == 0 ? groups : (int)std::min<size_t>(groups, std::max<size_t>(1, budget / per_group));
    int rc;
    if ((rc = b.ws.ensure((size_t)per_range * c->Lmax * N * 64)))
        return rc;
    BHMM_HIP(hipMemsetAsync(b.fails.p, 0, sizeof(unsigned int), c->stream));
    for (int g0 = 0; g0 < groups; g0 += per_range)
        BHMM_HIP(launch(bt_lds ? lds : global, dim3(std::min(per_range, groups - g0)), dim3(64), bt_lds ? lds_bt : 0,
                        c->stream, dm, W, ch, G, g0, c->d_offsets.p, c->d_obs_ci.p, c->d_obs_rm.p, dBt, c->M, b.ws.p,
                        mid..., b.aentry.p, b.aexit.p, b.bassumed.p, b.bout.p, b.dead.p));
    if (G > 1)
        BHMM_HIP(launch(k_post_check<N>, dim3((G + 255) / 256), dim3(256), 0, c->stream, ch, G, b.aentry.p, b.aexit.p,
                        b.bassumed.p, b.bout.p, b.dead.p, BOUNDARY_TOL, b.fails.p));
    BHMM_HIP(hipMemcpyAsync(&fails, b.fails.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    *v = plan::verdict_of(fails);
    return BHMM_OK;
}

// One call on the fused path: the boundary vectors sized, the model uploaded, the warm-up fixed_W or (0) the larger of
// the two directions of the forgetting probe, then pass(W, &verdict) by plan::two_attempts, a first failure counted
// in *fallbacks.  pass gets the model on the device and B^T from b.  *verified: the outputs of the pass stand
template <int N, int KIND, class Pass>
int sweep_run(bhmm_ctx *c, SweepBufs &b, const double *A, const double *pi, const double *par0, const double *par1,
              int fixed_W, int *fallbacks, Pass pass, bool *verified)
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
    int W = fixed_W;
    if (W <= 0 && (rc = fused_probe<N, KIND>(c, b.probe, m, b.Bt.p, true, &W)))
        return rc;
    return plan::two_attempts(
        W, 1 << 30, fallbacks, [&](int w, plan::Verdict *v) { return pass(dm, w, v); }, verified);
}

} // namespace bhmm
