// post_host.hpp -- host code the two units on the sweep of post_kernels.hpp share (bhmm_posterior_decode,
// post_api.hip; bhmm_posterior_marginals, marg_api.hip): the constants of the protocol and the warm-up probe.
// Each unit passes buffers of its own.
#pragma once
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "post_kernels.hpp"

namespace bhmm {

constexpr double POST_TOL = 1e-11;         // boundary check: componentwise relative (the E-step's spec_tol default)
constexpr int POST_W_UNPROBED = 288;       // warm-up when the trajectories are too short to probe (the E-step's)
constexpr size_t POST_LDS_BT = 16 * 1024;  // B^T staged in LDS up to this size

// warm-up from the forgetting curve: the probe's reading as bhmm_score takes it (chains within 1e-13
// from then on, + 15 %, doubled), here the larger of the forward and the backward direction.  0 where
// the trajectories are too short to probe
template <int N, int KIND>
int post_probe(bhmm_ctx *c, DevBuf<char> &buf, const Model<N> &m, const double *dBt, int *W)
{
    *W = 0;
    const int64_t maxT = longest_traj(c);
    const int Wmax = (int)std::min<int64_t>(1024, maxT / 2) / 4 * 4;
    if (Wmax < 32)
        return BHMM_OK;
    std::vector<int> longk;
    for (int k = 0; k < c->K; ++k)
        if (c->offsets[k + 1] - c->offsets[k] >= Wmax)
            longk.push_back(k);
    const int P = 256;
    std::vector<int64_t> starts(P);
    for (int i = 0; i < P; ++i) {
        const int k = longk[i % longk.size()];
        const int64_t room = c->offsets[k + 1] - c->offsets[k] - Wmax + 1;
        const int64_t rep = i / (int64_t)longk.size(), reps = (P + longk.size() - 1) / longk.size();
        starts[i] = c->offsets[k] + (room - 1) * rep / std::max<int64_t>(reps - 1, 1);
    }
    const size_t curve_words = 2 * (size_t)Wmax; // forward | backward
    int rc;
    if ((rc = buf.ensure(P * sizeof(int64_t) + curve_words * sizeof(unsigned int))))
        return rc;
    int64_t *d_starts = reinterpret_cast<int64_t *>(buf.p);
    unsigned int *d_curve = reinterpret_cast<unsigned int *>(d_starts + P);
    BHMM_HIP(hipMemcpyAsync(d_starts, starts.data(), P * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemsetAsync(d_curve, 0, curve_words * sizeof(unsigned int), c->stream));
    BHMM_HIP(launch(k_forget_probe<N, KIND>, dim3((2 * P + 63) / 64), dim3(64), 0, c->stream, m, c->d_obs_rm.p,
                    KIND == EMIT_DISC ? dBt : nullptr, d_starts, P, Wmax, d_curve));
    std::vector<float> curve(curve_words);
    BHMM_HIP(hipMemcpyAsync(curve.data(), d_curve, curve.size() * sizeof(float), hipMemcpyDeviceToHost,
                            c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    const float target = (float)(0.01 * POST_TOL);
    int last = -1;
    for (int dir = 0; dir < 2; ++dir)
        for (int w = 0; w < Wmax; ++w)
            if (curve[(size_t)dir * Wmax + w] >= target)
                last = std::max(last, w);
    const int w = (int)std::ceil(1.15 * (last + 2));
    *W = 2 * std::min(std::max(16, (w + 3) / 4 * 4), Wmax);
    return BHMM_OK;
}

} // namespace bhmm
