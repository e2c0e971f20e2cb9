// post_host.hpp -- host code the two units on the sweep of post_kernels.hpp share (bhmm_posterior_decode,
// post_api.hip; bhmm_posterior_marginals, marg_api.hip): the warm-up probe.  Each unit passes a buffer of its own.
// The constants of the protocol (BOUNDARY_TOL, W_UNPROBED, LDS_BT_MAX) and the probe's staging are seg_host.hpp's,
// shared with bhmm_score and bhmm_filter.
#pragma once
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "post_kernels.hpp"
#include "seg_host.hpp"

namespace bhmm {

// warm-up from the forgetting curve: the probe's reading as bhmm_score takes it (chains within 1e-13
// from then on, + 15 %, doubled), here the larger of the forward and the backward direction.  0 where
// the trajectories are too short to probe
template <int N, int KIND>
int post_probe(bhmm_ctx *c, DevBuf<char> &buf, const Model<N> &m, const double *dBt, int *W)
{
    *W = 0;
    const int Wmax = plan::probe_wmax(longest_traj(c));
    if (Wmax == 0)
        return BHMM_OK;
    Probe pr;
    int rc;
    if ((rc = probe_stage(c, buf, Wmax, 1, pr)))
        return rc;
    BHMM_HIP(launch(k_forget_probe<N, KIND>, dim3((2 * PROBE_P + 63) / 64), dim3(64), 0, c->stream, m, c->d_obs_rm.p,
                    KIND == EMIT_DISC ? dBt : nullptr, pr.d_starts, PROBE_P, Wmax, pr.d_curve));
    std::vector<float> curve;
    if ((rc = probe_read(c, pr, curve)))
        return rc;
    *W = 2 * plan::warmup_of(plan::curve_last(curve.data(), Wmax, (float)(0.01 * BOUNDARY_TOL), true), Wmax);
    return BHMM_OK;
}

} // namespace bhmm
