// pathlp_api.hip -- bhmm_path_logprob, bhmm_decode_logprob: the joint log-probability log p(s, O | model) of given or
// decoded hidden paths, per trajectory and model.  Kernels and the definition in pathlp_kernels.hpp, the tile
// arithmetic that of runs_host.hpp; DESIGN.md section 22.
//
// One call: (once per observation set: the trajectory of every tile's first step, from the offsets, to the device;)
// the stacked models to the device as they are, k_pathlp_prepare (their log tables), k_pathlp_tiles over the tiles of
// the path (one pass over path and observations for all models, one partial per model, tile and trajectory in it),
// k_pathlp_finish (per model and trajectory the partials in ascending tile order), then the status word and the
// result to the host (a state outside [0, n): BHMM_ERR_INVALID, nothing is delivered).  The buffers are c->pathlp.*,
// the only other fields touched are ds.pathlp_tiles_ready / pathlp_traj0 and last.pathlp_ms / pathlp_table;
// bhmm_decode_logprob decodes through the existing entry points first (bhmm_viterbi_batch_u8 into c->pathlp.path,
// post_decode_device into c->post.path), with everything those do to the context.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_internal.hpp"
#include "launch.hpp"
#include "model_check.hpp"
#include "pathlp_kernels.hpp"
#include "runs_host.hpp"

namespace bhmm {
namespace {

using namespace pathlp;

template <typename PT, int KIND>
int score_t(bhmm_ctx *c, const PT *path, int S, const double *A, const double *pi, const double *par0,
            const double *par1, double *logp)
{
    auto &b = c->pathlp;
    const int K = c->K, n = c->n, M = c->M;
    const int64_t total = c->total;
    const int64_t ntiles = runs::num_tiles(total);
    const int64_t nslots = ntiles + K;
    const size_t nn = (size_t)n * n, ne0 = KIND == EMIT_GAUSS ? (size_t)n : KIND == EMIT_DISC ? (size_t)n * M : 0;
    const size_t ne1 = KIND == EMIT_GAUSS ? (size_t)n : 0;
    const size_t stride = model_stride(KIND, n, M);
    c->last.pathlp_ms = 0.f;
    if (ntiles > 0x7fffffff)
        return invalid_arg("bhmm_path_logprob: the path has more tiles than a grid has workgroups");
    int rc;
    if ((rc = b.raw.ensure((size_t)S * (nn + n + ne0 + ne1))) || (rc = b.tab.ensure((size_t)S * stride)) ||
        (rc = b.part.ensure((size_t)S * nslots)) || (rc = b.logp.ensure((size_t)S * K)) || (rc = b.status.ensure(1)))
        return rc;
    if (!c->ds.pathlp_tiles_ready) { // the trajectory of every tile's first step: once per observation set
        std::vector<int32_t> tt((size_t)ntiles + 1);
        runs::tile_trajectories(c->offsets.data(), K, ntiles, tt.data());
        if ((rc = b.tile_traj.ensure(tt.size())))
            return rc;
        BHMM_HIP(hipMemcpyAsync(b.tile_traj.p, tt.data(), tt.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (tt is a temporary)
        c->ds.pathlp_traj0 = tt[0];
        c->ds.pathlp_tiles_ready = true;
    }
    for (hipEvent_t &e : b.ev)
        if (!e)
            BHMM_HIP(hipEventCreate(&e));
    // the models as the caller stacked them: [A | pi | par0 | par1]
    double *raw = b.raw.p;
    BHMM_HIP(hipMemcpyAsync(raw, A, (size_t)S * nn * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(raw + (size_t)S * nn, pi, (size_t)S * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (ne0)
        BHMM_HIP(hipMemcpyAsync(raw + (size_t)S * (nn + n), par0, (size_t)S * ne0 * sizeof(double), hipMemcpyHostToDevice,
                                c->stream));
    if (ne1)
        BHMM_HIP(hipMemcpyAsync(raw + (size_t)S * (nn + n + ne0), par1, (size_t)S * ne1 * sizeof(double),
                                hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemsetAsync(b.status.p, 0, sizeof(unsigned int), c->stream));
    BHMM_HIP(hipEventRecord(b.ev[0], c->stream));
    const unsigned prep_grid = (unsigned)std::min<size_t>(((size_t)S * stride + 255) / 256, 4096);
    BHMM_HIP(launch(k_pathlp_prepare, dim3(prep_grid), dim3(256), 0, c->stream, raw, S, n, M, KIND, b.tab.p));
    // the log tables in LDS when they fit the budget, else every entry through L2
    const bool table = n <= TABLE_MAX_N;
    const bool b_lds = table && KIND == EMIT_DISC && (size_t)n * M <= (size_t)TABLE_MAX_B;
    const size_t staged = !table ? 0 : nn + n + (KIND == EMIT_GAUSS ? 3 * (size_t)n : b_lds ? (size_t)n * M : 0);
    const size_t lds = tiles_lds(staged);
    c->last.pathlp_table = table ? 1 : 0;
    auto kern = table ? k_pathlp_tiles<PT, KIND, true> : k_pathlp_tiles<PT, KIND, false>;
    BHMM_HIP(launch(kern, dim3((unsigned)ntiles), dim3(THREADS), lds, c->stream, path,
                    static_cast<const void *>(c->d_obs_rm.p), total, c->d_offsets.p, K, b.tile_traj.p, n, M, S, b.tab.p,
                    b_lds ? 1 : 0, (int)c->ds.pathlp_traj0, nslots, b.part.p, b.status.p));
    const int64_t waves = (int64_t)S * K;
    BHMM_HIP(launch(k_pathlp_finish, dim3((unsigned)((waves + runs::WAVES - 1) / runs::WAVES)), dim3(THREADS), 0,
                    c->stream, b.part.p, nslots, c->d_offsets.p, K, S, (int)c->ds.pathlp_traj0, b.logp.p));
    BHMM_HIP(hipEventRecord(b.ev[1], c->stream));
    std::vector<double> res((size_t)S * K);
    unsigned int status = 0;
    BHMM_HIP(hipMemcpyAsync(res.data(), b.logp.p, res.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipMemcpyAsync(&status, b.status.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    (void)hipEventElapsedTime(&c->last.pathlp_ms, b.ev[0], b.ev[1]);
    if (status & STATUS_BAD_STATE)
        return invalid_arg("bhmm_path_logprob: the path holds a state outside [0, " + std::to_string(n) + ")");
    memcpy(logp, res.data(), res.size() * sizeof(double));
    return BHMM_OK;
}

int score_paths(bhmm_ctx *c, const void *path, int path_u8, int S, const double *A, const double *pi,
                const double *par0, const double *par1, double *logp)
{
    if ((int64_t)S * c->K > 0x7fffffffll * runs::WAVES)
        return invalid_arg("bhmm_path_logprob: nmodels * trajectories exceeds what one launch finishes");
#define BHMM_PATHLP_KIND(KIND)                                                                                      \
    (path_u8 ? score_t<uint8_t, KIND>(c, static_cast<const uint8_t *>(path), S, A, pi, par0, par1, logp)          \
             : score_t<int32_t, KIND>(c, static_cast<const int32_t *>(path), S, A, pi, par0, par1, logp))
    switch (c->kind) {
    case EMIT_GAUSS:
        return BHMM_PATHLP_KIND(EMIT_GAUSS);
    case EMIT_DISC:
        return BHMM_PATHLP_KIND(EMIT_DISC);
    default:
        return BHMM_PATHLP_KIND(EMIT_EXPL);
    }
#undef BHMM_PATHLP_KIND
}

} // namespace
} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_path_logprob(bhmm_ctx *c, const void *paths, int path_u8, int paths_on_device, int nmodels, const double *A,
                      const double *pi, const double *par0, const double *par1, double *logp)
{
    if (int rc = enter_model_call(c, paths && A && pi && logp, "bhmm_path_logprob: paths / A / pi / logp == NULL", true,
                                  par0, par1))
        return rc;
    if (nmodels < 1)
        return invalid_arg("bhmm_path_logprob: nmodels must be >= 1");
    if (path_u8 && c->n > 256) // (every byte is a state then; the int32 form holds the others)
        return invalid_arg("bhmm_path_logprob: one byte per step holds at most 256 states (use the int32 form)");
    if (int rc = check_models(c, "bhmm_path_logprob", nmodels, A, pi, par0, par1))
        return rc;
    if (paths_on_device) {
        if (reinterpret_cast<uintptr_t>(paths) % 16)
            return invalid_arg("bhmm_path_logprob: a device path must be aligned to 16 bytes");
        return score_paths(c, paths, path_u8, nmodels, A, pi, par0, par1, logp);
    }
    const size_t bytes = (size_t)c->total * (path_u8 ? sizeof(uint8_t) : sizeof(int32_t));
    if (int rc = c->pathlp.path.ensure(bytes))
        return rc;
    BHMM_HIP(hipMemcpyAsync(c->pathlp.path.p, paths, bytes, hipMemcpyHostToDevice, c->stream));
    return score_paths(c, c->pathlp.path.p, path_u8, nmodels, A, pi, par0, par1, logp);
}

int bhmm_decode_logprob(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                        int method, double *logp)
{
    if (int rc = enter_model_call(c, A && pi && logp, "bhmm_decode_logprob: A / pi / logp == NULL", true, par0, par1))
        return rc;
    if (method != 0 && method != 1)
        return invalid_arg("bhmm_decode_logprob: method is 0 (Viterbi) or 1 (posterior decoding)");
    if (c->n > 256)
        return invalid_arg("bhmm_decode_logprob: more than 256 states: decode with bhmm_viterbi_batch / "
                           "bhmm_posterior_decode and pass the int32 path to bhmm_path_logprob");
    if (int rc = check_models(c, "bhmm_decode_logprob", 1, A, pi, par0, par1))
        return rc;
    const void *path;
    if (method == 0) {
        int rc;
        if ((rc = c->pathlp.path.ensure((size_t)c->total)) ||
            (rc = bhmm_viterbi_batch_u8(c, A, pi, par0, par1, reinterpret_cast<uint8_t *>(c->pathlp.path.p), 1)))
            return rc;
        path = c->pathlp.path.p;
    } else {
        if (int rc = post_decode_device(c, A, pi, par0, par1, true, 1, false))
            return rc;
        path = c->post.path.p;
    }
    return score_paths(c, path, 1, 1, A, pi, par0, par1, logp);
}

} // extern "C"
