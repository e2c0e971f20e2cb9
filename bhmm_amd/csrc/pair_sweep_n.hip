// pair_sweep_n.hip -- k_pair_sweep (pair_kernels.hpp) for ONE state count (-DPAIR_N_VALUE=1 .. 8): its sixteen
// instantiations (gaussian / discrete, B^T in LDS / global, double / float, jump / projected) and one verified pass
// over them (sweep_pass, sweep_host.hpp).  See pair_api.hip for the driver (warm-up, retry protocol, generic path).
#include "pair_launch.hpp"
#include "sweep_host.hpp"

namespace bhmm {
namespace {

template <int N, int KIND, typename OT, bool PROJ>
int pass_as(bhmm_ctx *c, const Model<N> *dm, int W, const PairOut &o, plan::Verdict *v)
{
    auto &b = c->pair;
    return sweep_pass<N, KIND>(c, b, c->opt.pair_ws_mb, dm, W, b.Bt.p, k_pair_sweep<N, KIND, true, OT, PROJ>,
                               k_pair_sweep<N, KIND, false, OT, PROJ>, v, static_cast<OT *>(o.dev), o.W, o.Q);
}

} // namespace

template <int N, int KIND>
int pair_pass(bhmm_ctx *c, const Model<N> *dm, int W, const PairOut &o, plan::Verdict *v)
{
    if (o.Q > 0)
        return o.f32 ? pass_as<N, KIND, float, true>(c, dm, W, o, v) : pass_as<N, KIND, double, true>(c, dm, W, o, v);
    return o.f32 ? pass_as<N, KIND, float, false>(c, dm, W, o, v) : pass_as<N, KIND, double, false>(c, dm, W, o, v);
}

PAIR_PASS_DECL(, PAIR_N_VALUE)

} // namespace bhmm
