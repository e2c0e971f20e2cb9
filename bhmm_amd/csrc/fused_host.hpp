// fused_host.hpp -- host scaffolding of the verified passes for up to 8 states over the E-step's chunk plan (the fused
// paths of bhmm_score, bhmm_filter, bhmm_posterior_decode and bhmm_posterior_marginals): when they are taken
// (fused_takes), the dispatch on the state count (dispatch_n), the upload of a model and its padded B^T
// (upload_fused_model) and the warm-up from the forgetting probe (fused_probe).  Each unit passes buffers of its own
// and keeps its kernels, its pass and its outputs.  The constants of the protocol and the probe's staging are
// seg_host.hpp's, the protocol itself (two_attempts) plan.hpp's.
#pragma once
#include <type_traits>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "seg_host.hpp"

namespace bhmm {

// the fused path answers: the family of up to 8 states, a kind with emission parameters, at least one chunk
inline bool fused_takes(const bhmm_ctx *c)
{
    return !c->wide && !c->gen && c->n <= 8 && (c->kind == EMIT_GAUSS || c->kind == EMIT_DISC) && c->G > 0;
}

// f(std::integral_constant<int, n>()) for 1 <= n <= 8 states
template <class F>
int dispatch_n(int n, F f)
{
    switch (n) {
    case 1:
        return f(std::integral_constant<int, 1>());
    case 2:
        return f(std::integral_constant<int, 2>());
    case 3:
        return f(std::integral_constant<int, 3>());
    case 4:
        return f(std::integral_constant<int, 4>());
    case 5:
        return f(std::integral_constant<int, 5>());
    case 6:
        return f(std::integral_constant<int, 6>());
    case 7:
        return f(std::integral_constant<int, 7>());
    default:
        return f(std::integral_constant<int, 8>());
    }
}

// one model as the kernels read it: m filled (fill_model) and copied to model_buf, for a discrete model B^T padded to
// N columns in Bt_buf; both buffers sized here.  Waits for the copies (B^T is a temporary, m may be)
template <int N, int KIND>
int upload_fused_model(bhmm_ctx *c, DevBuf<char> &model_buf, DevBuf<double> &Bt_buf, const double *A, const double *pi,
                       const double *par0, const double *par1, Model<N> &m)
{
    int rc;
    if ((rc = model_buf.ensure(sizeof(Model<N>))) || (KIND == EMIT_DISC && (rc = Bt_buf.ensure((size_t)c->M * N))))
        return rc;
    fill_model<N>(m, c->n, KIND, c->M, A, pi, par0, par1);
    std::vector<double> bt;
    if (KIND == EMIT_DISC) {
        bt.resize((size_t)c->M * N);
        fill_Bt_padded(c->n, N, c->M, par0, bt.data());
        BHMM_HIP(hipMemcpyAsync(Bt_buf.p, bt.data(), bt.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    BHMM_HIP(hipMemcpyAsync(model_buf.p, &m, sizeof(Model<N>), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    return BHMM_OK;
}

// Warm-up of each of S models from its forgetting curve (k_forget_probe once per model; dBt: their B^T, M x N each):
// the E-step's reading (plan::warmup_of: chains within 0.01 of the check's tolerance from then on, + 15 %) of the
// forward chains, or with `both` of the worse direction, doubled -- the E-step lengthens its warm-up after a failed
// check and keeps it for the observation set, these calls keep nothing (1024 x 1e6 steps, slowly mixing models: the
// plain reading failed the check of bhmm_score for three models of four, twice that passed).  W_UNPROBED where the
// trajectories are too short to probe
template <int N, int KIND>
int fused_probe_models(bhmm_ctx *c, DevBuf<char> &probe_buf, int S, const Model<N> *m, const double *dBt, bool both,
                       int *W)
{
    std::fill(W, W + S, W_UNPROBED);
    const int Wmax = plan::probe_wmax(longest_traj(c));
    if (Wmax == 0)
        return BHMM_OK;
    Probe pr;
    int rc;
    if ((rc = probe_stage(c, probe_buf, Wmax, S, pr)))
        return rc;
    const size_t curve_words = 2 * (size_t)Wmax;
    for (int s = 0; s < S; ++s)
        BHMM_HIP(launch(k_forget_probe<N, KIND>, dim3((2 * PROBE_P + 63) / 64), dim3(64), 0, c->stream, m[s],
                        c->d_obs_rm.p, KIND == EMIT_DISC ? dBt + (size_t)s * c->M * N : nullptr, pr.d_starts, PROBE_P,
                        Wmax, pr.d_curve + s * curve_words));
    std::vector<float> curve;
    if ((rc = probe_read(c, pr, curve)))
        return rc;
    const float target = (float)(0.01 * BOUNDARY_TOL);
    for (int s = 0; s < S; ++s)
        W[s] = 2 * plan::warmup_of(plan::curve_last(curve.data() + s * curve_words, Wmax, target, both), Wmax);
    return BHMM_OK;
}
// ... of one model
template <int N, int KIND>
int fused_probe(bhmm_ctx *c, DevBuf<char> &probe_buf, const Model<N> &m, const double *dBt, bool both, int *W)
{
    return fused_probe_models<N, KIND>(c, probe_buf, 1, &m, dBt, both, W);
}

} // namespace bhmm
