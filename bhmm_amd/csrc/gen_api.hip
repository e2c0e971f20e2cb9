// gen_api.hip -- host side of the any-N family (gen_kernels.hpp): contexts with more than 64 hidden
// states.  bhmm/hidden/impl_c/_hidden.c:16-378 has no limit on N; neither has the C ABI.  Everything
// is trajectory-major and materialised like the reference does (pobs, alpha, beta / W rows); one
// workgroup per trajectory, no time decomposition.  Compiled with -ffp-contract=off.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "gen_kernels.hpp"
#include "viterbi_host.hpp"

namespace bhmm {

namespace {

size_t gen_smem(int n, int vectors, int extra) { return ((size_t)vectors * n + extra) * sizeof(double); }
// the workgroup's own copy of the transition matrix behind the vectors, where it fits (gen_kernels.hpp, ALDS)
size_t gen_a_bytes(int n) { return (size_t)n * n * sizeof(double); }
bool gen_a_in_lds(int n, size_t vectors_bytes) { return vectors_bytes + gen_a_bytes(n) <= GEN_LDS_LIMIT; }

// emission rows of all steps (the reference materialises them too, maximum_likelihood.py:249-252)
int gen_pobs(bhmm_ctx *c, const WideModel &m, const double **pobs)
{
    if (c->kind == EMIT_EXPL) {
        *pobs = reinterpret_cast<const double *>(c->d_obs_rm.p);
        return BHMM_OK;
    }
    int rc = c->d_gpobs.ensure((size_t)c->total * c->n);
    if (rc)
        return rc;
    const dim3 pg((unsigned)((c->total + 255) / 256)), pb(256);
    auto *k = c->kind == EMIT_GAUSS ? k_pobs_all<EMIT_GAUSS> : k_pobs_all<EMIT_DISC>;
    BHMM_HIP(launch(k, pg, pb, 0, c->stream, m, c->d_obs_rm.p, c->total, c->d_gpobs.p));
    *pobs = c->d_gpobs.p;
    return BHMM_OK;
}

int gen_transposed(bhmm_ctx *c, const WideModel &m)
{
    const int n = c->n;
    int rc = c->d_gAt.ensure((size_t)n * n);
    if (rc)
        return rc;
    BHMM_HIP(launch(k_gen_transpose, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256), 0, c->stream, m.A, n,
                    c->d_gAt.p));
    return BHMM_OK;
}

// rescue: the E-step's forward pass (k_gen_forward<.., RESCUE>)
int gen_launch_forward(bhmm_ctx *c, const WideModel &m, const double *pobs, bool rescue = false)
{
    size_t sm = gen_smem(c->n, 2, 2);
    const bool alds = gen_a_in_lds(c->n, sm);
    sm += alds ? gen_a_bytes(c->n) : 0;
    auto *k = rescue ? (alds ? k_gen_forward<true, true> : k_gen_forward<false, true>)
                     : (alds ? k_gen_forward<true> : k_gen_forward<false>);
    BHMM_HIP(launch(k, dim3(c->K), dim3(GEN_TPB), sm, c->stream, m, c->d_offsets.p, c->K, pobs, c->d_alpha_rm.p,
                    c->d_logLk.p));
    return BHMM_OK;
}

// xi GEMM + reduction geometry
int gen_nsplit(const bhmm_ctx *c)
{
    const int tiles = (c->n + 31) / 32;
    const int64_t want = 4096 / ((int64_t)tiles * tiles) + 1;
    return (int)std::max<int64_t>(1, std::min<int64_t>({want, (c->total + 63) / 64, (int64_t)256}));
}

} // namespace

int gen_alloc(bhmm_ctx *c)
{
    const int n = c->n;
    const size_t rows = (size_t)c->total * n;
    const int K = std::max(c->K, 1);
    const size_t S = 1 + (size_t)n + (size_t)n * n + n + std::max<size_t>(2 * (size_t)n, (size_t)n * c->M);
    int rc;
    if ((rc = c->d_alpha_rm.ensure(rows)) || (rc = c->d_logLk.ensure(K)) ||
        (rc = c->d_gamma0.ensure((size_t)K * n)) || (rc = c->d_stats.ensure(S)))
        return rc;
    if (tile_gen_capable(c) && (rc = tile_gen_alloc(c)))
        return rc;
    return BHMM_OK;
}

int gen_forward(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                const double *par1)
{
    WideModel m;
    int rc = wide_model(c, c->kind, A, pi, par0, par1, m);
    if (rc)
        return rc;
    const double *pobs = nullptr;
    if ((rc = gen_pobs(c, m, &pobs)))
        return rc;
    return gen_launch_forward(c, m, pobs);
}

// beta rows of _hidden.c:69-110 (explicit pobs) into d_alpha_rm
int gen_backward(bhmm_ctx *c, const double *A)
{
    WideModel m;
    std::vector<double> pi(c->n, 1.0 / c->n);
    int rc = wide_model(c, EMIT_EXPL, A, pi.data(), nullptr, nullptr, m);
    if (rc || (rc = gen_transposed(c, m)))
        return rc;
    const double *pobs = reinterpret_cast<const double *>(c->d_obs_rm.p);
    size_t sm = gen_smem(c->n, 3, 1 + GEN_TPB);
    const bool alds = gen_a_in_lds(c->n, sm);
    sm += alds ? gen_a_bytes(c->n) : 0;
    auto *k = alds ? k_gen_backward<EMIT_EXPL, false, true> : k_gen_backward<EMIT_EXPL, false, false>;
    BHMM_HIP(launch(k, dim3(c->K), dim3(GEN_TPB), sm, c->stream, m, c->d_gAt.p, c->d_offsets.p, c->K, pobs, nullptr,
                    nullptr, c->d_alpha_rm.p, nullptr, nullptr, nullptr, nullptr, nullptr));
    return BHMM_OK;
}

int gen_estep(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
              double *stats_dev, int flags)
{
    WideModel m;
    int rc = wide_model(c, c->kind, A, pi, par0, par1, m);
    if (rc)
        return rc;
    {
        // up to 128 states: the row-batched matrix-core kernels (tolerance-compared statistics); the
        // order-faithful kernels below where those do not apply or left their range
        bool done = false;
        if ((rc = tile_gen_estep(c, m, stats_dev, flags, &done)) || done)
            return rc;
    }
    const int n = c->n, K = c->K;
    const bool sg = (flags & BHMM_FLAG_STORE_GAMMA) != 0;
    const int nsplit = gen_nsplit(c);
    if ((rc = gen_transposed(c, m)) || (rc = c->d_gW.ensure((size_t)c->total * n)) ||
        (rc = c->d_gpart.ensure((size_t)std::max(K, 1) * 3 * n)) ||
        (rc = c->d_gxipart.ensure((size_t)nsplit * n * n)) ||
        (c->kind == EMIT_DISC && (rc = c->d_gsym.ensure((size_t)n * c->M))) ||
        (sg && (rc = c->d_gamma_ci.ensure((size_t)c->total * n))))
        return rc;
    BHMM_HIP(hipEventRecord(c->ev[0], c->stream));
    const double *pobs = nullptr;
    if ((rc = gen_pobs(c, m, &pobs)))
        return rc;
    BHMM_HIP(hipEventRecord(c->ev[1], c->stream));
    if ((rc = gen_launch_forward(c, m, pobs, true)))
        return rc;
    BHMM_HIP(hipEventRecord(c->ev[2], c->stream));
    if (c->kind == EMIT_DISC)
        BHMM_HIP(hipMemsetAsync(c->d_gsym.p, 0, (size_t)n * c->M * sizeof(double), c->stream));
    size_t sm = gen_smem(n, 3, 1 + GEN_TPB);
    const bool alds = gen_a_in_lds(n, sm);
    sm += alds ? gen_a_bytes(n) : 0;
    double *gam = sg ? c->d_gamma_ci.p : nullptr;
    auto *kb = c->kind == EMIT_GAUSS
                   ? (alds ? k_gen_backward<EMIT_GAUSS, true, true> : k_gen_backward<EMIT_GAUSS, true, false>)
               : c->kind == EMIT_DISC
                   ? (alds ? k_gen_backward<EMIT_DISC, true, true> : k_gen_backward<EMIT_DISC, true, false>)
                   : (alds ? k_gen_backward<EMIT_EXPL, true, true> : k_gen_backward<EMIT_EXPL, true, false>);
    BHMM_HIP(launch(kb, dim3(K), dim3(GEN_TPB), sm, c->stream, m, c->d_gAt.p, c->d_offsets.p, K, pobs, c->d_obs_rm.p,
                    c->d_alpha_rm.p, nullptr, c->d_gW.p, gam, c->d_gpart.p, c->d_gamma0.p, c->d_gsym.p));
    const int tiles = (n + 31) / 32;
    BHMM_HIP(launch(k_gen_xi_gemm, dim3(tiles * tiles, nsplit), dim3(256), 0, c->stream, c->d_alpha_rm.p, c->d_gW.p,
                    c->total, n, nsplit, c->d_gxipart.p));
    BHMM_HIP(hipEventRecord(c->ev[3], c->stream));
    auto *kf = c->kind == EMIT_GAUSS ? k_gen_finalize<EMIT_GAUSS>
               : c->kind == EMIT_DISC ? k_gen_finalize<EMIT_DISC>
                                      : k_gen_finalize<EMIT_EXPL>;
    BHMM_HIP(launch(kf, dim3(256), dim3(256), 0, c->stream, m, K, nsplit, c->d_gxipart.p, c->d_gpart.p, c->d_gamma0.p,
                    c->d_logLk.p, c->d_gsym.p, stats_dev));
    BHMM_HIP(hipEventRecord(c->ev[4], c->stream));
    c->ev_pending = true;
    return BHMM_OK;
}

namespace {

// ---- Viterbi above 64 states: one function per path (VitCall and the shared hooks: viterbi_host.hpp; v.obs is the
// emission matrix of gen_pobs; the back-trace walks over the segments of plan 0) ----
// 65..128 states: over time segments (k_gen_viterbi_seg), accepted by seg_viterbi (path_api.hip).  A fix-up round
// costs half a first pass here, hence the margin rule from the first call on (round 5: 25.7 -> 11 ms) and the
// mending of the few far boundaries (round 6); warm-up and segment length: plan::vit_gen_*
int gen_seg_viterbi(bhmm_ctx *c, const WideModel &m, const VitCall &v, bool *done)
{
    const int n = c->n, K = c->K;
    const int64_t *off = c->d_offsets.p;
    const double *pobs = static_cast<const double *>(v.obs);
    const size_t smv = (size_t)(128 * GVS_PITCH + 8 * 128) * sizeof(double);
    const int W0 = plan::vit_w_estep(c->ds.spec_W), seg_warmups = c->opt.vit_margin ? 1 : c->opt.vit_seg_warmups;
    const int W_cap = plan::vit_gen_w_cap(W0, plan::vit_gen_fill(c->total, c->num_simd, c->opt.vit_seg_per_simd));
    int W_try = plan::vit_gen_w_start(c->ds.vit.W, W0, W_cap, c->opt.vit_margin, c->opt.vit_mend), rc;
    const size_t smm = vit_margin_lds(n);
    double *vall = vit_vall(c, c->opt.vit_margin);
    if (vall && !(allow_lds(k_vit_margin<int32_t, 2>, smm) == hipSuccess &&
                  allow_lds(k_vit_margin<uint8_t, 2>, smm) == hipSuccess)) {
        (void)hipGetLastError();
        vall = nullptr;
    }
    const int64_t maxT = longest_traj(c);
    for (int attempt = 0; attempt < 2 && !*done; ++attempt) {
        if (attempt > 0)
            W_try *= 2;
        const int64_t seglen = plan::vit_gen_seglen(c->total, c->num_simd, c->opt.vit_seg_per_simd, seg_warmups, W_try);
        Segs sg;
        if ((rc = wide_path_plan(c, 0, seglen, sg)))
            return rc;
        if (sg.nseg <= K)
            break;
        sg.W = W_try;
        if ((rc = vit_boundary_bufs(c, sg, 128)))
            return rc;
        const dim3 sgrid((sg.nseg + 7) / 8), sblk(512);
        SegViterbi f;
        f.pass = [&](bool fix) -> int {
            BHMM_HIP(launch(fix ? k_gen_viterbi_seg<true> : k_gen_viterbi_seg<false>, sgrid, sblk, smv, c->stream, m,
                            off, sg, pobs, v.ptr, v.last, c->d_aentry.p, c->d_aexit.p, c->d_vckpt.p, c->d_vflag.p,
                            fix ? nullptr : vall, 0.0, nullptr));
            BHMM_HIP(launch(k_wide_vit_check<128>, dim3((sg.nseg + 255) / 256), dim3(256), 0, c->stream, sg,
                            c->d_aentry.p, c->d_aexit.p, c->d_vflag.p, c->d_specres.p, (!fix && vall) ? SEG_VIT_TOL : 0.0));
            return BHMM_OK;
        };
        f.mend = [&]() -> int {
            BHMM_HIP(launch(k_gen_viterbi_seg<true>, sgrid, sblk, smv, c->stream, m, off, sg, pobs, v.ptr, v.last,
                            c->d_aentry.p, c->d_aexit.p, c->d_vckpt.p, c->d_vflag.p + sg.nseg, vall, SEG_VIT_TOL,
                            c->d_specres.p + 1));
            return BHMM_OK;
        };
        f.margins = [&](double margin) { return vit_margins<2>(c, v, sg, m.A, smm, vall, margin); };
        f.walks = [&]() { return vit_walks<2>(c, v, sg, c->pplan_buf[0].traj0.p); };
        SegVitResult r;
        if ((rc = seg_viterbi(c, f, sg, seglen, vall, maxT, 12, false, &r)))
            return rc;
        if ((*done = r.accepted))
            vit_accepted(c, r, vall, W_try, W_cap);
    }
    vit_attempts_done(c, *done);
    return BHMM_OK;
}

// 129..256 states (round 5): four segments per workgroup share every pass over A (k_gen_viterbi_rows); first pass
// only -- accepted when every boundary is bit-identical or by the margins of the decisions on its path
// (k_vit_margin), else the serial kernel decides.  Warm-up: plan::vit_rows_w_start (at 256 states one boundary of
// 749 was still 1e-12 off after 504 steps, none after 750 -- and a pass that is not accepted is lost time)
int gen_rows_viterbi(bhmm_ctx *c, const WideModel &m, const VitCall &v, bool *done)
{
    const int n = c->n, K = c->K;
    const int64_t *off = c->d_offsets.p;
    const double *pobs = static_cast<const double *>(v.obs);
    static_assert(GVR_ROWS == plan::VIT_ROWS, "the plan's segments per workgroup are the kernel's");
    const int64_t fill0 = plan::vit_rows_fill(c->total, c->num_simd);
    const int W_try = plan::vit_rows_w_start(c->ds.vit.W, plan::vit_w_estep(c->ds.spec_W), fill0, c->opt.vit_mend);
    const int64_t seglen = plan::vit_rows_seglen(fill0, W_try), maxT = longest_traj(c);
    Segs sg;
    int rc;
    if ((rc = wide_path_plan(c, 0, seglen, sg)))
        return rc;
    c->last.vit_margin_used = c->last.vit_margin_close = c->last.vit_seg_rounds = 0;
    // two threads per target state (candidate ranges; measured 15.8 / 13.3 / 14.1 ms at 129 states with 1 / 2 / 4)
    const size_t smr = (size_t)(2 * GVR_ROWS * n + GVR_ROWS) * sizeof(double) +
                       (size_t)GVR_ROWS * 256 * (sizeof(double) + sizeof(int));
    // (no plan to gain from, or a buffer that cannot be had: the serial kernel)
    if (!(sg.nseg > K && (rc = gen_transposed(c, m)) == BHMM_OK && c->d_gW.ensure((size_t)c->total * n) == BHMM_OK &&
          c->d_aentry.ensure((size_t)sg.nseg * 256) == BHMM_OK && c->d_aexit.ensure((size_t)sg.nseg * 256) == BHMM_OK &&
          c->d_vflag.ensure(2 * (size_t)sg.nseg) == BHMM_OK && ensure_specres(c) == BHMM_OK &&
          c->d_vmaps.ensure((size_t)sg.nseg * 256) == BHMM_OK && c->d_vend.ensure((size_t)sg.nseg) == BHMM_OK)) {
        (void)hipGetLastError();
        return BHMM_OK;
    }
    sg.W = W_try;
    double *vall = c->d_gW.p;
    const dim3 rgrid((sg.nseg + GVR_ROWS - 1) / GVR_ROWS), rblk(512);
    SegViterbi f;
    f.pass = [&](bool) -> int { // (first pass only: no fix-up rounds)
        BHMM_HIP(launch(k_gen_viterbi_rows<GVR_ROWS, 2>, rgrid, rblk, smr, c->stream, m, off, sg, pobs, v.ptr, v.last,
                        c->d_aentry.p, c->d_aexit.p, vall, nullptr, 0.0, nullptr));
        BHMM_HIP(launch(k_wide_vit_check<256>, dim3((sg.nseg + 255) / 256), dim3(256), 0, c->stream, sg,
                        c->d_aentry.p, c->d_aexit.p, c->d_vflag.p, c->d_specres.p, SEG_VIT_TOL));
        return BHMM_OK;
    };
    f.mend = [&]() -> int {
        BHMM_HIP(launch(k_gen_viterbi_rows<GVR_ROWS, 2, true>, rgrid, rblk, smr, c->stream, m, off, sg, pobs, v.ptr,
                        v.last, c->d_aentry.p, c->d_aexit.p, vall, c->d_vflag.p + sg.nseg, SEG_VIT_TOL,
                        c->d_specres.p + 1));
        return BHMM_OK;
    };
    f.margins = [&](double margin) { return vit_margins<4, false>(c, v, sg, c->d_gAt.p, 0, vall, margin); };
    // (the back-trace of the pass is needed either way: enqueued before its verdict is read)
    f.walks = [&]() { return vit_walks<4>(c, v, sg, c->pplan_buf[0].traj0.p); };
    SegVitResult r;
    if ((rc = seg_viterbi(c, f, sg, seglen, vall, maxT, 0, true, &r)))
        return rc;
    if ((*done = c->last.viterbi_chunked = r.accepted)) {
        c->ds.vit.W = W_try;
        c->ds.vit.rows_fail = 0;
    } else if (plan::vit_rows_give_up(++c->ds.vit.rows_fail, W_try, maxT)) {
        // (one pass that was not accepted -- an early EM iterate, say -- only doubles the next call's warm-up)
        c->ds.vit.seg_given_up = true;
    } else {
        c->ds.vit.W = 2 * W_try;
    }
    return BHMM_OK;
}

// one workgroup per trajectory (k_gen_viterbi_fwd, back-pointers of two bytes) and the trace
int gen_serial_viterbi(bhmm_ctx *c, const WideModel &m, const VitCall &v)
{
    const int n = c->n, K = c->K;
    uint16_t *ptr = reinterpret_cast<uint16_t *>(v.ptr);
    size_t sm = gen_smem(n, 2, 2);
    const bool alds = gen_a_in_lds(n, sm);
    sm += alds ? gen_a_bytes(n) : 0;
    BHMM_HIP(launch(alds ? k_gen_viterbi_fwd<true> : k_gen_viterbi_fwd<false>, dim3(K), dim3(GEN_TPB), sm, c->stream, m,
                    c->d_offsets.p, K, static_cast<const double *>(v.obs), ptr, v.last));
    BHMM_HIP(v.out([&](auto *p) {
        return launch(k_gen_viterbi_trace<std::remove_pointer_t<decltype(p)>>, dim3((K + 63) / 64), dim3(64), 0, c->stream,
                      c->d_offsets.p, K, n, ptr, v.last, p);
    }));
    return BHMM_OK;
}

} // namespace

// out_fmt as wide_viterbi_run: 0 int32 host, 1 uint8 host, 2 uint8 device (N <= 256 for the bytes)
int gen_viterbi_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                    const double *par1, void *paths_out, int out_fmt)
{
    const int n = c->n, K = c->K;
    if (out_fmt != 0 && n > 256)
        return invalid_arg("one byte per step holds at most 256 states: use bhmm_viterbi_batch (int32)");
    WideModel m;
    int rc = wide_model(c, c->kind, A, pi, par0, par1, m);
    if (rc)
        return rc;
    c->last.viterbi_chunked = false;
    c->last.vit_mended = 0;
    const double *pobs = nullptr;
    if ((rc = gen_pobs(c, m, &pobs)) ||
        (rc = c->d_scratch.ensure((size_t)c->total * n * sizeof(uint16_t))) ||
        (rc = c->d_scratch2.ensure(((size_t)c->total + K) * sizeof(int32_t))))
        return rc;
    // (one byte per back-pointer in the segment passes, two in the serial kernel)
    const VitCall v = vit_call(c, paths_out, out_fmt, pobs, EMIT_EXPL);
    bool done = false;
    const bool segments = c->opt.spec_enabled && !c->ds.vit.seg_given_up;
    if (n <= 128 && segments)
        rc = gen_seg_viterbi(c, m, v, &done);
    else if (n <= 256 && segments && c->opt.vit_margin)
        rc = gen_rows_viterbi(c, m, v, &done);
    if (rc || (!done && (rc = gen_serial_viterbi(c, m, v))))
        return rc;
    return deliver_paths(c, paths_out, out_fmt, v.path);
}

// alpha_dev: rows to sample from (the context's own forward pass when NULL)
int gen_sample_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                   const double *par1, const double *u, uint64_t seed, int32_t *paths,
                   int64_t *counts, int64_t *n0, double *emis, double *stats_dev)
{
    WideModel m;
    int rc = wide_model(c, c->kind, A, pi, par0, par1, m);
    if (rc)
        return rc;
    const int n = c->n, K = c->K;
    const size_t nstat = (size_t)n * n + n;
    const size_t esz = c->kind == EMIT_GAUSS ? 3 * (size_t)n : (c->kind == EMIT_DISC ? (size_t)n * c->M : 0);
    const size_t nsym = c->kind == EMIT_DISC ? (size_t)n * c->M : 0;
    if ((rc = c->d_scratch2.ensure(((size_t)c->total + 4) * sizeof(int32_t))) ||
        (rc = c->d_scratch.ensure((nstat + nsym + (size_t)std::max(K, 1) * GEN_PS_SLABS * 3 * n + nstat + esz +
                                   (u ? (size_t)c->total : 0) + 8) * sizeof(double))))
        return rc;
    int32_t *path = reinterpret_cast<int32_t *>(c->d_scratch2.p);
    int *status = reinterpret_cast<int *>(path + c->total);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(c->d_scratch.p);
    unsigned long long *symcnt = cnt + nstat;
    double *epart = reinterpret_cast<double *>(symcnt + nsym);
    double *packed = epart + (size_t)std::max(K, 1) * GEN_PS_SLABS * 3 * n;
    double *udev = nullptr;
    if (u) {
        udev = packed + nstat + esz;
        BHMM_HIP(hipMemcpyAsync(udev, u, (size_t)c->total * sizeof(double), hipMemcpyHostToDevice,
                                c->stream));
    }
    BHMM_HIP(hipMemsetAsync(cnt, 0, (nstat + nsym) * sizeof(unsigned long long), c->stream));
    // up to 512 states: the draw over time segments (k_gen_sample_seg), by the protocol of seg_draw (path_api.hip)
    SegDraw f;
    // alpha rows in d_alpha_rm: from the tile forward pass over time segments where it verifies
    // (65..128 states; the draw normalises alpha_t[i] A[i][s_{t+1}] itself, any factor per row cancels),
    // else from the serial recursion
    f.forward = [&](bool exact) -> int {
        bool fwd_seg = false;
        int r;
        if (!exact && (r = tile_gen_forward_draw(c, m, &fwd_seg)))
            return r;
        c->last.draw_fwd_segmented = fwd_seg;
        if (fwd_seg)
            return BHMM_OK;
        c->last.draw_alpha_dev = 0.0;
        return gen_forward(c, A, pi, par0, par1);
    };
    f.prepare = [&](const Segs &) { return gen_transposed(c, m); };
    f.pass = [&](bool fix, const Segs &sg, const DrawWatch &watch) -> int {
        auto *k = n <= 128   ? (fix ? k_gen_sample_seg<2, true> : k_gen_sample_seg<2, false>)
                  : n <= 256 ? (fix ? k_gen_sample_seg<4, true> : k_gen_sample_seg<4, false>)
                             : (fix ? k_gen_sample_seg<8, true> : k_gen_sample_seg<8, false>);
        BHMM_HIP(launch(k, dim3((sg.nseg + 3) / 4), dim3(256), 0, c->stream, m, c->d_gAt.p, c->d_offsets.p, sg,
                        c->d_alpha_rm.p, udev, seed, c->d_soff.p, path, status, c->d_sentry.p, c->d_sexit.p, c->d_vflag.p,
                        watch));
        return BHMM_OK;
    };
    f.serial = [&]() -> int {
        size_t sm = gen_smem(n, 2, 4);
        const bool alds = gen_a_in_lds(n, sm);
        sm += alds ? gen_a_bytes(n) : 0;
        auto *ks = alds ? k_gen_sample<true> : k_gen_sample<false>;
        BHMM_HIP(launch(ks, dim3(K), dim3(GEN_TPB), sm, c->stream, m, c->d_offsets.p, K, c->d_alpha_rm.p, udev, seed,
                        c->d_soff.p, path, status));
        return BHMM_OK;
    };
    if ((rc = seg_draw(c, f, A, pi, par0, par1, n <= 512, (int64_t)c->opt.smp_seg_per_simd * c->num_simd, status)))
        return rc;
    int hstatus = 0;
    BHMM_HIP(hipMemcpyAsync(&hstatus, status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    if (hstatus) {
        set_error("random choice found no state: alpha/A not normalisable (_hidden.c:299-304)");
        return hstatus;
    }
    const void *obs = c->d_obs_rm.p;
    const dim3 pg(256), pb(256);
    auto *kps = c->kind == EMIT_GAUSS ? k_gen_path_stats<EMIT_GAUSS>
                : c->kind == EMIT_DISC ? k_gen_path_stats<EMIT_DISC>
                                       : k_gen_path_stats<EMIT_EXPL>;
    auto *kpack = c->kind == EMIT_GAUSS ? k_gen_pack_path_stats<EMIT_GAUSS>
                  : c->kind == EMIT_DISC ? k_gen_pack_path_stats<EMIT_DISC>
                                         : k_gen_pack_path_stats<EMIT_EXPL>;
    BHMM_HIP(launch(kps, dim3(K, GEN_PS_SLABS), dim3(GEN_TPB), 0, c->stream, m, c->d_offsets.p, K, obs, path, cnt, epart,
                    symcnt));
    BHMM_HIP(launch(kpack, pg, pb, 0, c->stream, m, K, cnt, epart, symcnt, stats_dev ? stats_dev : packed));
    std::vector<double> hp;
    if (!stats_dev && (counts || n0 || emis)) {
        hp.resize(nstat + esz);
        BHMM_HIP(hipMemcpyAsync(hp.data(), packed, hp.size() * sizeof(double), hipMemcpyDeviceToHost,
                                c->stream));
    }
    if (paths)
        BHMM_HIP(hipMemcpyAsync(paths, path, (size_t)c->total * sizeof(int32_t), hipMemcpyDeviceToHost,
                                c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    if (!hp.empty()) {
        if (counts)
            for (size_t e = 0; e < (size_t)n * n; ++e)
                counts[e] = (int64_t)llround(hp[e]);
        if (n0)
            for (int i = 0; i < n; ++i)
                n0[i] = (int64_t)llround(hp[(size_t)n * n + i]);
        if (emis && esz)
            memcpy(emis, hp.data() + nstat, esz * sizeof(double));
    }
    return BHMM_OK;
}

// single-trajectory entry points with host arrays and more than 64 states ---------------------------
int gen_transition_counts(double *C, const double *A, const double *pobs, const double *alpha,
                          const double *beta, int N, int64_t T)
{
    if (N > GEN_MAXN)
        return invalid_arg("more than 4096 hidden states are not supported");
    double *d = nullptr;
    const size_t rows = (size_t)T * N, nn = (size_t)N * N;
    const int tiles = (N + 31) / 32;
    const int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>({4096 / ((int64_t)tiles * tiles) + 1,
                                                                    (T + 63) / 64, (int64_t)256}));
    const size_t need = 4 * rows + 2 * nn + (size_t)nsplit * nn + nn;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), need * sizeof(double));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipMalloc failed");
        return BHMM_ERR_NO_MEM;
    }
    struct Free {
        double *p;
        ~Free() { (void)hipFree(p); }
    } guard{d};
    double *dp = d, *da = dp + rows, *db = da + rows, *dW = db + rows, *dA = dW + rows, *dAt = dA + nn,
           *dpart = dAt + nn, *dC = dpart + (size_t)nsplit * nn;
    BHMM_HIP(hipMemcpy(dp, pobs, rows * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(da, alpha, rows * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(db, beta, rows * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(dA, A, nn * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(launch(k_gen_transpose, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, 0, dA, N, dAt));
    const size_t sm = ((size_t)N + GEN_TPB) * sizeof(double);
    BHMM_HIP(launch(k_gen_w_rows, dim3((unsigned)T), dim3(GEN_TPB), sm, 0, dAt, N, T, dp, da, db, dW));
    BHMM_HIP(launch(k_gen_xi_gemm, dim3(tiles * tiles, nsplit), dim3(256), 0, 0, da, dW, T, N, nsplit, dpart));
    std::vector<double> hpart((size_t)nsplit * nn);
    BHMM_HIP(hipMemcpy(hpart.data(), dpart, hpart.size() * sizeof(double), hipMemcpyDeviceToHost));
    (void)dC;
    for (size_t ij = 0; ij < nn; ++ij) {
        double v = 0.0;
        for (int s = 0; s < nsplit; ++s)
            v += hpart[(size_t)s * nn + ij];
        C[ij] = v * A[ij];
    }
    return BHMM_OK;
}

int gen_sample_path(int32_t *path, const double *alpha, const double *A, const double *u, int N,
                    int64_t T)
{
    if (N > GEN_MAXN)
        return invalid_arg("more than 4096 hidden states are not supported");
    double *d = nullptr;
    const size_t rows = (size_t)T * N, nn = (size_t)N * N;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), (rows + nn + (size_t)T + 8) * sizeof(double) +
                                                                ((size_t)T + 4) * sizeof(int32_t));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipMalloc failed");
        return BHMM_ERR_NO_MEM;
    }
    struct Free {
        double *p;
        ~Free() { (void)hipFree(p); }
    } guard{d};
    double *da = d, *dA = da + rows, *du = dA + nn;
    int64_t *doff = reinterpret_cast<int64_t *>(du + T);
    int32_t *dpath = reinterpret_cast<int32_t *>(doff + 2);
    int *status = reinterpret_cast<int *>(dpath + T);
    const int64_t off[2] = {0, T};
    BHMM_HIP(hipMemcpy(da, alpha, rows * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(dA, A, nn * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(du, u, (size_t)T * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(doff, off, sizeof(off), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemset(status, 0, sizeof(int)));
    WideModel m;
    memset(&m, 0, sizeof(m));
    m.A = dA;
    m.n = N;
    const size_t sm = gen_smem(N, 2, 4);
    BHMM_HIP(launch(k_gen_sample<false>, dim3(1), dim3(GEN_TPB), sm, 0, m, doff, 1, da, du, (uint64_t)0, nullptr, dpath,
                    status));
    int hstatus = 0;
    BHMM_HIP(hipMemcpy(&hstatus, status, sizeof(int), hipMemcpyDeviceToHost));
    if (hstatus) {
        set_error("random choice found no state: alpha/A not normalisable (_hidden.c:299-304)");
        return hstatus;
    }
    BHMM_HIP(hipMemcpy(path, dpath, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost));
    return BHMM_OK;
}

} // namespace bhmm
