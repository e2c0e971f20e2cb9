// pair_sweep_n.hip -- k_pair_sweep (pair_kernels.hpp) for ONE state count (-DPAIR_N_VALUE=1 .. 8): its sixteen
// instantiations (gaussian / discrete, B^T in LDS / global, double / float, jump / projected) and one verified pass
// over them.  See pair_api.hip for the driver (model upload, warm-up, retry protocol, generic path).
#include <algorithm>

#include "pair_launch.hpp"

namespace bhmm {
namespace {

template <int N, int KIND, typename OT, bool PROJ>
int pass_as(bhmm_ctx *c, PairState &b, const Model<N> *dm, int W, const double *dBt, const PairOut &o, plan::Verdict *v)
{
    unsigned int fails = 0;
    const int G = c->G, groups = c->Gp / 64;
    const Chunks ch = chunks_of(c);
    const size_t lds_bt = (size_t)c->M * score_bt_stride(N) * sizeof(double);
    const bool bt_lds = KIND == EMIT_DISC && lds_bt <= LDS_BT_MAX;
    // alpha rows of one group, and how many groups the budget holds (at least one)
    const size_t per_group = (size_t)c->Lmax * N * 64 * sizeof(double);
    const size_t budget = (size_t)b.opt_ws_mb << 20;
    const int per_range =
        budget == 0 ? groups : (int)std::min<size_t>(groups, std::max<size_t>(1, budget / per_group));
    int rc;
    if ((rc = b.ws.ensure((size_t)per_range * c->Lmax * N * 64)))
        return rc;
    BHMM_HIP(hipMemsetAsync(b.fails.p, 0, sizeof(unsigned int), c->stream));
    auto *kern = bt_lds ? k_pair_sweep<N, KIND, true, OT, PROJ> : k_pair_sweep<N, KIND, false, OT, PROJ>;
    for (int g0 = 0; g0 < groups; g0 += per_range)
        BHMM_HIP(launch(kern, dim3(std::min(per_range, groups - g0)), dim3(64), bt_lds ? lds_bt : 0, c->stream, dm, W,
                        ch, G, g0, c->d_offsets.p, c->d_obs_ci.p, c->d_obs_rm.p, dBt, c->M, b.ws.p,
                        static_cast<OT *>(o.dev), o.W, o.Q, b.aentry.p, b.aexit.p, b.bassumed.p, b.bout.p, b.dead.p));
    if (G > 1)
        BHMM_HIP(launch(k_post_check<N>, dim3((G + 255) / 256), dim3(256), 0, c->stream, ch, G, b.aentry.p, b.aexit.p,
                        b.bassumed.p, b.bout.p, b.dead.p, BOUNDARY_TOL, b.fails.p));
    BHMM_HIP(hipMemcpyAsync(&fails, b.fails.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    *v = plan::verdict_of(fails);
    return BHMM_OK;
}

} // namespace

template <int N, int KIND>
int pair_pass(bhmm_ctx *c, PairState &b, const Model<N> *dm, int W, const double *dBt, const PairOut &o,
              plan::Verdict *v)
{
    if (o.Q > 0)
        return o.f32 ? pass_as<N, KIND, float, true>(c, b, dm, W, dBt, o, v)
                     : pass_as<N, KIND, double, true>(c, b, dm, W, dBt, o, v);
    return o.f32 ? pass_as<N, KIND, float, false>(c, b, dm, W, dBt, o, v)
                 : pass_as<N, KIND, double, false>(c, b, dm, W, dBt, o, v);
}

PAIR_PASS_DECL(, PAIR_N_VALUE)

} // namespace bhmm
