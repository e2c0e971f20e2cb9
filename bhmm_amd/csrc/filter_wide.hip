// filter_wide.hip -- the kernels of bhmm_filter's time-parallel path for 9..64 states in a translation unit of
// their own: 72 instantiations of k_filter_wide (16 / 32 / 64 lanes per segment x gaussian / discrete with B^T in
// LDS / discrete with B^T read ahead x double / float x rows / projection x with / without logc) and the forward
// forgetting probe of the family.  The plan, the warm-up and the protocol are in filter_api.hip.
#include "filter_wide_kernels.hpp"
#include "filter_wide_launch.hpp"
#include "host_internal.hpp"
#include "launch.hpp"

namespace bhmm {
namespace {

constexpr size_t FILTER_WIDE_LDS_BT = 16 * 1024; // B^T staged in LDS up to this size (bhmm_score's limit)

template <int NP, int KIND, bool BT_LDS, typename OT>
int launch_forms(bhmm_ctx *c, const FilterWideArgs &a, size_t lds)
{
    constexpr int GP = 64 / NP;
    const bool proj = a.Q > 0 && a.rows != nullptr;
    auto *kern = proj ? (a.logc ? k_filter_wide<NP, KIND, BT_LDS, OT, true, true>
                                : k_filter_wide<NP, KIND, BT_LDS, OT, true, false>)
                      : (a.logc ? k_filter_wide<NP, KIND, BT_LDS, OT, false, true>
                                : k_filter_wide<NP, KIND, BT_LDS, OT, false, false>);
    BHMM_HIP(launch(kern, dim3((a.sg.nseg + GP - 1) / GP), dim3(64), lds, c->stream, a.dm, a.W, c->d_offsets.p, a.sg,
                    c->d_obs_rm.p, static_cast<OT *>(a.rows), a.V, a.Q, static_cast<OT *>(a.logc), a.aentry, a.aexit,
                    a.dead));
    return BHMM_OK;
}

template <int NP>
int launch_np(bhmm_ctx *c, const FilterWideArgs &a)
{
    if (c->kind == EMIT_GAUSS)
        return a.f32 ? launch_forms<NP, EMIT_GAUSS, false, float>(c, a, 0)
                     : launch_forms<NP, EMIT_GAUSS, false, double>(c, a, 0);
    const size_t lds_bt = (size_t)c->M * NP * sizeof(double);
    if (lds_bt <= FILTER_WIDE_LDS_BT)
        return a.f32 ? launch_forms<NP, EMIT_DISC, true, float>(c, a, lds_bt)
                     : launch_forms<NP, EMIT_DISC, true, double>(c, a, lds_bt);
    return a.f32 ? launch_forms<NP, EMIT_DISC, false, float>(c, a, 0)
                 : launch_forms<NP, EMIT_DISC, false, double>(c, a, 0);
}

template <int NP>
int probe_np(bhmm_ctx *c, const WideModel &m, const int64_t *d_starts, int P, int Wmax, unsigned int *d_curve)
{
    constexpr int GP = 64 / NP;
    if (c->kind == EMIT_GAUSS)
        BHMM_HIP(launch(k_wide_probe<NP, EMIT_GAUSS>, dim3(P / GP), dim3(64), 0, c->stream, m, c->d_obs_rm.p, d_starts,
                        P, Wmax, d_curve));
    else
        BHMM_HIP(launch(k_wide_probe<NP, EMIT_DISC>, dim3(P / GP), dim3(64), 0, c->stream, m, c->d_obs_rm.p, d_starts,
                        P, Wmax, d_curve));
    return BHMM_OK;
}

} // namespace

int filter_wide_launch(bhmm_ctx *c, int np, const FilterWideArgs &a)
{
    return np == 16 ? launch_np<16>(c, a) : (np == 32 ? launch_np<32>(c, a) : launch_np<64>(c, a));
}

int filter_wide_probe_launch(bhmm_ctx *c, int np, const WideModel &m, const int64_t *d_starts, int P, int Wmax,
                             unsigned int *d_curve)
{
    return np == 16   ? probe_np<16>(c, m, d_starts, P, Wmax, d_curve)
           : np == 32 ? probe_np<32>(c, m, d_starts, P, Wmax, d_curve)
                      : probe_np<64>(c, m, d_starts, P, Wmax, d_curve);
}

} // namespace bhmm
