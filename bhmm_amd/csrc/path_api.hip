// path_api.hip -- C ABI entry points backed by the order-faithful kernels (Viterbi, path
// sampling) and the small reference-shaped row-major kernels.  This translation unit is
// compiled with -ffp-contract=off (see Makefile): no fused multiply-adds, so products and
// sums round like the reference's scalar C.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "plan.hpp"
#include "path_kernels.hpp"
#include "draw_verify.hpp"
#include "viterbi_host.hpp"

namespace bhmm {

// ---- draws inside the reach of the alpha rows' verified deviation (draw_verify.hpp) ---------------
// d_dv: [count | disagree | unconverged | checked] | DrawEvent[DRAW_EVENT_CAP] | model
static inline size_t dv_model_offset() { return 16 + (size_t)DRAW_EVENT_CAP * sizeof(DrawEvent); }

// watch for one sampling call: tol <= 0 (or the option off) leaves it switched off.  The four counters are
// cleared on the stream.
// count_slot: a counter the caller clears with its own fills (saves a dispatch per Gibbs sweep)
int draw_watch_prepare(bhmm_ctx *c, double tol, DrawWatch &w, unsigned int *count_slot)
{
    w.ev = nullptr;
    w.count = nullptr;
    w.tol = 0.0;
    c->last.draw_events = c->last.draw_checked = c->last.draw_redone = 0;
    if (!c->opt.draw_watch || !(tol > 0.0))
        return BHMM_OK;
    const size_t msz = ((size_t)c->n * c->n + 3 * (size_t)c->n +
                        (c->kind == EMIT_DISC ? (size_t)c->n * c->M : 0)) * sizeof(double);
    int rc = c->d_dv.ensure(dv_model_offset() + msz);
    if (rc)
        return rc;
    if (!count_slot)
        BHMM_HIP(hipMemsetAsync(c->d_dv.p, 0, 16, c->stream));
    w.count = count_slot ? count_slot : reinterpret_cast<unsigned int *>(c->d_dv.p);
    w.ev = reinterpret_cast<DrawEvent *>(c->d_dv.p + 16);
    w.tol = c->opt.draw_watch_tol > 0.0 ? c->opt.draw_watch_tol : tol;
    return BHMM_OK;
}

// `count` draws were recorded: those with gap <= thr are decided again on the windowed serial recursion.
// *ok = every such decision stands (else the caller repeats the call on exact alpha rows).
int draw_verify_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                    unsigned int count, double thr, int64_t Wlong, bool *ok)
{
    *ok = false;
    c->last.draw_events = count;
    if (count > DRAW_EVENT_CAP)
        return BHMM_OK; // (more than the list holds: the exact rows decide)
    const int n = c->n;
    double *md = reinterpret_cast<double *>(c->d_dv.p + dv_model_offset());
    BHMM_HIP(hipMemcpyAsync(md, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(md + (size_t)n * n, pi, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    double *mp0 = md + (size_t)n * n + n;
    if (c->kind == EMIT_GAUSS) {
        BHMM_HIP(hipMemcpyAsync(mp0, par0, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipMemcpyAsync(mp0 + n, par1, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    } else if (c->kind == EMIT_DISC) {
        BHMM_HIP(hipMemcpyAsync(mp0, par0, (size_t)n * c->M * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    unsigned int *res = reinterpret_cast<unsigned int *>(c->d_dv.p);
    BHMM_HIP(hipMemsetAsync(res + 1, 0, 12, c->stream)); // (the three result words; rare path)
    const size_t sm = (4 * (size_t)n + 8) * sizeof(double);
    BHMM_HIP(launch(k_draw_verify, dim3(count), dim3(256), sm, c->stream, reinterpret_cast<const DrawEvent *>(c->d_dv.p + 16),
                    (int)count, md, n, c->M, c->kind, c->d_obs_rm.p, c->d_offsets.p, Wlong, thr, res + 1));
    unsigned int h[4] = {0, 0, 0, 0};
    BHMM_HIP(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    c->last.draw_checked = h[3];
    *ok = h[1] == 0 && h[2] == 0 && !(c->opt.draw_test_redo && h[3] > 0);
    return BHMM_OK;
}

int draw_decide_again(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                      unsigned int count, double thr, const std::function<int()> &repeat, bool *repeated)
{
    *repeated = false;
    bool ok = false;
    int rc = draw_verify_run(c, A, pi, par0, par1, count, thr, 8 * (int64_t)std::max(c->ds.spec_W, 64), &ok);
    if (rc || ok)
        return rc;
    // a decision does not stand: the whole draw again on exact rows; the counters keep what THIS draw recorded
    const unsigned int ev = c->last.draw_events, ck = c->last.draw_checked;
    *repeated = true;
    rc = repeat();
    c->last.draw_events = ev;
    c->last.draw_checked = ck;
    c->last.draw_redone = 1;
    return rc;
}

namespace {

struct Tmp { // scoped raw device allocations for the context-free entry points
    std::vector<void *> ptrs;
    ~Tmp()
    {
        for (void *p : ptrs)
            (void)hipFree(p);
    }
    template <typename T>
    int alloc(T **out, size_t count)
    {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("hipMalloc failed");
            return BHMM_ERR_NO_MEM;
        }
        ptrs.push_back(p);
        *out = static_cast<T *>(p);
        return BHMM_OK;
    }
};

template <int N>
int sample_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
               const double *par1, const double *u, uint64_t seed, int32_t *paths, int64_t *counts,
               int64_t *n0, double *emis, double *stats_dev, bool defer_check = true, bool exact = false)
{
    // alpha -> CI workspace.  The boundary check of a speculative forward pass is only enqueued:
    // its verdict comes back with the results below, and a failed check repeats the call with the
    // waiting form (which then lengthens the warm-up / falls back to the exact pass).
    static const bool no_defer = getenv("BHMM_AMD_NO_DEFER") != nullptr; // (kernel experiments)
    c->fwd_defer = defer_check && !no_defer && !exact;
    // exact: the transfer-matrix pass (every boundary vector computed, none assumed) -- the repeat of a call
    // in which a watched draw did not stand (draw_verify.hpp)
    const bool spec_saved = c->opt.spec_enabled;
    if (exact)
        c->opt.spec_enabled = false;
    int rc = forward_ci(c, A, pi, par0, par1);
    c->opt.spec_enabled = spec_saved;
    c->fwd_defer = false;
    if (rc)
        return rc;
    // A deferred verdict must be consumed on EVERY way out (allocation failure, launch error ...):
    // left pending, its bookkeeping is skipped and a later call reads stale verdict words.
    struct PendingVerdict {
        bhmm_ctx *c;
        ~PendingVerdict()
        {
            if (!c->fwd_pending)
                return;
            c->fwd_pending = false;
            (void)hipStreamSynchronize(c->stream);
            bool ok = false;
            (void)forward_ci_verdict(c, &ok); // (the call is failing anyway: outcome unused)
        }
    } pending_guard{c};
    const int K = c->K, n = c->n;
    const size_t nstat = (size_t)N * N + N;
    // parts per chunk for the map kernels (BHMM_AMD_SMP_PARTS overrides: kernel experiments)
    static const int parts_env = getenv("BHMM_AMD_SMP_PARTS") ? atoi(getenv("BHMM_AMD_SMP_PARTS")) : 0;
    // (k_smp_maps keeps within 128 VGPRs, i.e. four wavefronts per SIMD: 8 parts per chunk fill
    // them on the default plan of 32768 chunks; measured on configs[4]: P = 4 0.56, 8 0.48, 16 0.52 ms
    // for maps + stitch + apply)
    // Few, short chunks (the shard of one of eight ranks: 32 x 1e5 steps -> 16352 chunks of 196 steps) gave ONE
    // part per chunk, i.e. a quarter of a wavefront per SIMD walking 196 dependent steps: k_smp_maps took 325 us
    // of a 550 us path step.  Parts as short as 16 steps until the lanes fill the chip (round 6).
    int Pfill = 1;
    while (Pfill < 16 && c->Lmax / (2 * Pfill) >= 16 && (int64_t)c->G * Pfill < 262144)
        Pfill *= 2;
    const int P = parts_env > 0 ? parts_env : std::max(Pfill, c->Lmax >= 512 ? 8 : (c->Lmax >= 256 ? 4 : 1));
    const int nblk = (c->Gp / BLOCK) * P;
    const size_t esz = c->kind == EMIT_GAUSS ? 3 * (size_t)N : (c->kind == EMIT_DISC ? (size_t)c->M * N : 0);
    // scratch2: [path] | status | part maps | next-part states | lowest non-final step per part |
    // nibbles of the final steps (8 per word)
    // (c->keep_path: the caller reads the path on the device afterwards -- bhmm_mvn_sample_paths -- no copy for it)
    const bool want_path = paths || c->keep_path;
    const size_t npath = want_path ? (size_t)c->total : 0;
    const int Lp = c->Lmax / P + 2;          // steps per part (upper bound)
    const int W8 = (Lp + 7) / 8 + 1;
    // ... | full step maps above the coalescence point (one word per step)
    if ((rc = c->d_scratch2.ensure((npath + 4 + (3 + (size_t)W8 + (size_t)Lp) * (size_t)c->Gp * P) *
                                   sizeof(int32_t))))
        return rc;
    int32_t *path = want_path ? reinterpret_cast<int32_t *>(c->d_scratch2.p) : nullptr;
    int *status = nullptr; // (lives behind the counts, see below)
    uint32_t *fmap = reinterpret_cast<uint32_t *>(reinterpret_cast<int32_t *>(c->d_scratch2.p) + npath + 4);
    int32_t *nstate = reinterpret_cast<int32_t *>(fmap + (size_t)c->Gp * P);
    int32_t *dmark = nstate + (size_t)c->Gp * P;
    uint32_t *nib = reinterpret_cast<uint32_t *>(dmark + (size_t)c->Gp * P);
    uint32_t *gw = nib + (size_t)W8 * c->Gp * P;
    const int64_t Gp64 = c->Gp;
    // scratch: counts | reduced emission | status | emission partials | u   (the first three are
    // zeroed by ONE fill: every fill is a dispatch of its own, ~5 us on the stream)
    // emission partials: one table per workgroup, or (big discrete alphabets) a few global ones
    const bool bigM = c->kind == EMIT_DISC && c->bt_global;
    const size_t ntab = bigM ? (size_t)DISC_GLOBAL_TABLES : (size_t)nblk;
    const size_t dbl = nstat + esz + 1 + ntab * esz + (u ? (size_t)c->total : 0) + 8;
    if ((rc = c->d_scratch.ensure(dbl * sizeof(double))))
        return rc;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(c->d_scratch.p);
    double *ered = reinterpret_cast<double *>(c->d_scratch.p) + nstat;
    status = reinterpret_cast<int *>(ered + esz);
    double *epart = ered + esz + 1;
    BHMM_HIP(hipMemsetAsync(cnt, 0, (nstat + esz + 1) * sizeof(double), c->stream));
    if (bigM)
        BHMM_HIP(hipMemsetAsync(epart, 0, ntab * esz * sizeof(double), c->stream));
    double *udev = nullptr;
    if (u) {
        udev = epart + ntab * esz;
        BHMM_HIP(hipMemcpyAsync(udev, u, (size_t)c->total * sizeof(double), hipMemcpyHostToDevice,
                                c->stream));
    }
    Model<N> m;
    fill_model<N>(m, n, c->kind, c->M, A, pi, par0, par1);
    m.bt_global = bigM ? 1 : 0;
    // rows of a speculative pass: draws within 64 x the tolerance of its boundary check are recorded (the
    // measured deviation, usually far smaller, is applied when they are looked at)
    DrawWatch watch;
    if ((rc = draw_watch_prepare(c, c->rows32_valid && !exact ? 64.0 * c->opt.spec_tol : 0.0, watch,
                                 reinterpret_cast<unsigned int *>(status) + 1))) // (second word of the cleared status slot)
        return rc;
    {
        // exact chunk-parallel sampling: maps per part, stitch, apply + statistics
        const Chunks chs = chunks_of(c);
        const int64_t *offd = c->d_offsets.p;
        const void *obs_ci = c->d_obs_ci.p;
        const int64_t *soffd = c->d_soff.p ? c->d_soff.p : c->d_offsets.p;
        const double *wsd = c->d_ws.p, *Btd = c->d_Bt.p;
        // fp32 copies of the alpha rows, if the forward pass that just ran wrote them
        const float *r32 = c->rows32_valid ? c->d_ws32.p : nullptr;
        auto *km = c->kind == EMIT_GAUSS ? (r32 ? k_smp_maps<N, EMIT_GAUSS, true> : k_smp_maps<N, EMIT_GAUSS, false>)
                   : c->kind == EMIT_DISC ? (r32 ? k_smp_maps<N, EMIT_DISC, true> : k_smp_maps<N, EMIT_DISC, false>)
                                          : (r32 ? k_smp_maps<N, EMIT_EXPL, true> : k_smp_maps<N, EMIT_EXPL, false>);
        BHMM_HIP(launch(km, dim3(nblk), dim3(BLOCK), 0, c->stream, m, chs, offd, soffd, wsd, r32, obs_ci, Btd, udev, seed,
                        P, fmap, status, dmark, nib, W8, Gp64, gw, Lp, watch));
        if ((int64_t)c->G * P >= (int64_t)32 * K) // long chains: one wavefront per trajectory
            BHMM_HIP(launch(k_smp_stitch, dim3(K), dim3(64), 0, c->stream, c->d_traj_c0.p, K, P, fmap, nstate, nullptr));
        else
            BHMM_HIP(launch(k_smp_stitch_serial, dim3((K + SMP_STITCH_TPB - 1) / SMP_STITCH_TPB), dim3(64), 0, c->stream,
                            c->d_traj_c0.p, K, P, fmap, nstate, nullptr));
        const int32_t *ns = nstate, *dmk = dmark;
        const uint32_t *nb = nib, *gwc = gw;
        auto *ka = c->kind == EMIT_GAUSS  ? k_smp_apply<N, EMIT_GAUSS>
                   : c->kind == EMIT_DISC ? k_smp_apply<N, EMIT_DISC>
                                          : k_smp_apply<N, EMIT_EXPL>;
        const size_t smd = c->kind == EMIT_DISC && !bigM ? (size_t)c->M * N * sizeof(double) : 0;
        BHMM_HIP(launch(ka, dim3(nblk), dim3(BLOCK), smd, c->stream, m, chs, offd, obs_ci, P, ns, path, cnt, epart, dmk, nb,
                        W8, Gp64, gwc, Lp, status));
        if (esz)
            BHMM_HIP(launch(k_add_partials, dim3((unsigned)esz), dim3(64), 0, c->stream, epart, (int)ntab, (int)esz, ered));
    }
    // counts | reduced emission statistics | [status, watched draws] are contiguous on the device: ONE copy, into
    // pinned memory where it fits (a pageable destination makes every small copy a round trip of its own)
    const size_t nres = nstat + esz + 1;
    std::vector<double> hres_v;
    double *hres = nullptr;
    if (nres <= 8192) {
        if (!c->h_small)
            BHMM_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_small), 8192 * sizeof(double), hipHostMallocDefault));
        hres = c->h_small;
    } else {
        hres_v.resize(nres);
        hres = hres_v.data();
    }
    int hstatus = 0;
    if (stats_dev) {
        // statistics stay on the device, packed for the caller's all-reduce
        BHMM_HIP(launch(k_pack_path_stats, dim3(1), dim3(256), 0, c->stream, cnt, ered, n, N, c->M, c->kind, 1, stats_dev));
        BHMM_HIP(hipMemcpyAsync(hres + nres - 1, status, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    } else {
        BHMM_HIP(hipMemcpyAsync(hres, cnt, nres * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    const unsigned long long *hc = reinterpret_cast<const unsigned long long *>(hres);
    const double *he = hres + nstat;
    const int *hst = reinterpret_cast<const int *>(hres + nres - 1); // [status | watched draws]
    if (paths)
        BHMM_HIP(hipMemcpyAsync(paths, path, (size_t)c->total * sizeof(int32_t),
                                hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    if (c->fwd_pending) {
        c->fwd_pending = false;
        bool ok = false;
        if ((rc = forward_ci_verdict(c, &ok)))
            return rc;
        if (!ok) // boundaries did not verify: everything above ran on wrong alpha rows
            return sample_run<N>(c, A, pi, par0, par1, u, seed, paths, counts, n0, emis, stats_dev,
                                 false);
    }
    hstatus = hst[0];
    const unsigned int nwatched = watch.count ? (unsigned int)hst[1] : 0u;
    c->last.draw_alpha_dev = watch.count ? (double)c->last.spec_last_dev : 0.0;
    if (nwatched) {
        // draws inside 64 x the deviation the boundary check measured: decided again on the serial recursion
        // over a long window; if one does not stand, the whole call again on the transfer-matrix rows
        bool repeated = false;
        const double thr = c->opt.draw_watch_tol > 0.0 ? c->opt.draw_watch_tol
                                                   : 64.0 * std::max((double)c->last.spec_last_dev, 1e-16);
        rc = draw_decide_again(
            c, A, pi, par0, par1, nwatched, thr,
            [&] { return sample_run<N>(c, A, pi, par0, par1, u, seed, paths, counts, n0, emis, stats_dev, false, true); },
            &repeated);
        if (rc || repeated)
            return rc;
    }
    if (hstatus) {
        set_error("random choice found no state: alpha/A not normalisable (_hidden.c:299-304)");
        return hstatus;
    }
    if (stats_dev)
        return BHMM_OK;
    if (counts)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                counts[i * n + j] = (int64_t)hc[i * N + j];
    if (n0)
        for (int i = 0; i < n; ++i)
            n0[i] = (int64_t)hc[N * N + i];
    if (emis) {
        if (c->kind == EMIT_GAUSS)
            for (int w = 0; w < 3; ++w)
                for (int i = 0; i < n; ++i)
                    emis[w * n + i] = he[w * N + i];
        else if (c->kind == EMIT_DISC)
            for (int i = 0; i < n; ++i)
                for (int o = 0; o < c->M; ++o)
                    emis[(size_t)i * c->M + o] = he[(size_t)o * N + i];
    }
    return BHMM_OK;
}

} // namespace

// time segments of at most seglen steps for the segment-parallel Viterbi pass (which = 0) / backward
// sampler (which = 1); rebuilt only when the length changes
int wide_path_plan(bhmm_ctx *c, int which, int64_t seglen, Segs &sg)
{
    auto &pp = c->ds.pplan[which];
    auto &pb = c->pplan_buf[which];
    if (pp.nseg == 0 || pp.seglen != seglen) {
        plan::SegPlan sp;
        plan::plan_segments(c->offsets, c->K, seglen, 1, sp);
        const int ns = (int)sp.traj.size();
        int rc;
        if ((rc = pb.traj.ensure(std::max(ns, 1))) || (rc = pb.len.ensure(std::max(ns, 1))) ||
            (rc = pb.t0.ensure(std::max(ns, 1))) || (rc = pb.traj0.ensure(c->K + 1)))
            return rc;
        BHMM_HIP(hipMemcpyAsync(pb.traj0.p, sp.traj0.data(), (c->K + 1) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipMemcpyAsync(pb.traj.p, sp.traj.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipMemcpyAsync(pb.len.p, sp.len.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipMemcpyAsync(pb.t0.p, sp.t0.data(), ns * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream)); // (the vectors go out of scope)
        pp.nseg = ns;
        pp.seglen = seglen;
        pp.maxlen = 0;
        for (int32_t l : sp.len)
            pp.maxlen = std::max<int64_t>(pp.maxlen, l);
    }
    sg.traj = pb.traj.p;
    sg.len = pb.len.p;
    sg.t0 = pb.t0.p;
    sg.nseg = pp.nseg;
    return BHMM_OK;
}

int deliver_paths(bhmm_ctx *c, void *paths_out, int out_fmt, const void *dev_paths)
{
    if (out_fmt == 2) { // the paths are where the caller wants them; the call still completes them
        BHMM_HIP(hipStreamSynchronize(c->stream));
        return BHMM_OK;
    }
    return copy_to_host_pinned(c, paths_out, dev_paths,
                               (size_t)c->total * (out_fmt == 0 ? sizeof(int32_t) : sizeof(uint8_t)));
}

int copy_to_host_pinned(bhmm_ctx *c, void *dst, const void *src, size_t bytes)
{
    hipPointerAttribute_t attr;
    const bool caller_pinned = hipPointerGetAttributes(&attr, dst) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    const bool pinned = !caller_pinned && bytes >= ((size_t)8 << 20) &&
                        hipHostRegister(dst, bytes, hipHostRegisterDefault) == hipSuccess;
    if (!pinned)
        (void)hipGetLastError();
    hipError_t ce = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
    if (ce == hipSuccess)
        ce = hipStreamSynchronize(c->stream);
    if (pinned)
        (void)hipHostUnregister(dst);
    BHMM_HIP(ce);
    return BHMM_OK;
}

// Accepted only if EVERY segment arrives at its first step with the bit pattern its predecessor left there --
// then the back-pointers are the serial run's, by induction from the exact first segment of each trajectory --
// or by the path margins (k_vit_margin) when every boundary is within SEG_VIT_TOL.
int seg_viterbi(bhmm_ctx *c, const SegViterbi &f, const Segs &sg, int64_t seglen, const double *vall, int64_t maxT,
                int max_rounds, bool walks_first, SegVitResult *res)
{
    *res = SegVitResult();
    int rc;
    if ((rc = ensure_specres(c)))
        return rc;
    unsigned int *h = c->h_specres;
    bool allow_mend = c->opt.vit_mend && f.mend, mended = false, walked = false, bitwise = false;
    c->last.vit_mended = 0;
    // pass 0 with warm-ups, then fix-up rounds while any boundary is not bit-identical
    int round = 0;
    for (; round <= max_rounds; ++round) {
        if ((rc = specres_reset(c)))
            return rc;
        lds_poison(c->stream);
        if ((rc = f.pass(round > 0)))
            return rc;
        walked = walks_first;
        if ((walks_first && (rc = f.walks())) || (rc = specres_read(c)))
            return rc;
        if (round == 0) {
            c->last.vit_seg_mismatch = (int)h[3];
            c->last.vit_far = (int)h[0];
        }
        if (h[3] == 0) {
            bitwise = true;
            break;
        }
        if (round > 0)
            continue;
        int spliced = 0;
        if (vall && h[0] != 0 && (int64_t)h[0] * 2 <= sg.nseg && allow_mend) {
            mended = true;
            // Some boundaries are further than SEG_VIT_TOL from their predecessors' vectors (the warm-up was too short
            // THERE; the max-product vectors of a metastable model need several times the filter's forgetting length
            // at a few boundaries -- configs[3]: 276 of 2048 after 256 steps, none after 904): those segments alone
            // are run again from the predecessor's vector until they are within SEG_VIT_TOL of a kept vector of the
            // first pass instead of lengthening every warm-up.  If one reaches its end the rounds decide.
            if ((rc = specres_reset(c)))
                return rc;
            lds_poison(c->stream);
            if ((rc = f.mend()))
                return rc;
            walked = false;
            unsigned int notmet = 0;
            BHMM_HIP(hipMemcpyAsync(&notmet, c->d_specres.p + 1, sizeof(unsigned int), hipMemcpyDeviceToHost,
                                    c->stream));
            BHMM_HIP(hipStreamSynchronize(c->stream));
            c->last.vit_mended = (int)h[0];
            if (notmet == 0) {
                spliced = (int)h[0];
                h[0] = 0;
            }
        }
        if (vall && h[0] == 0) {
            // every boundary (and splice) within SEG_VIT_TOL: the path of this pass, and the margins of the
            // decisions on it
            const int maxseg = (int)((maxT + seglen - 1) / seglen) + 1 + spliced;
            const double margin = std::max(1e-10, 16.0 * (2e-15 * (double)maxT + SEG_VIT_TOL * maxseg));
            if (!walked && (rc = f.walks()))
                return rc;
            walked = true;
            if ((rc = specres_reset(c)) || (rc = f.margins(margin)) || (rc = specres_read(c)))
                return rc;
            c->last.vit_margin_close = (int)h[2];
            if (h[2] == 0) {
                c->last.vit_margin_used = 1;
                res->margin_accepted = true;
                break;
            }
            // (a close decision on the path: the rounds decide)
        }
        if (mended && max_rounds > 0) {
            // The rounds compare BITWISE with the kept vectors of the first pass; a mended segment now holds exact
            // vectors up to its splice and first-pass vectors behind it, so a repeated run would stop at the first
            // kept vector and take the rest for exact.  A pass that was mended and then not accepted is therefore
            // run again from scratch, without mending (one first pass lost).
            allow_mend = false;
            mended = false;
            round = -1;
        }
    }
    res->rounds = c->last.vit_seg_rounds = max_rounds > 0 ? round : 0;
    res->accepted = bitwise || res->margin_accepted;
    if (res->accepted && !walked && (rc = f.walks()))
        return rc;
    return BHMM_OK;
}

// The draws are coupled through the per-step uniforms: a segment that did not continue its successor's state is
// drawn again from that state until it meets its own earlier path, so an accepted draw is the serial kernel's.
int seg_draw(bhmm_ctx *c, const SegDraw &f, const double *A, const double *pi, const double *par0, const double *par1,
             bool segments_allowed, int64_t want_segments, int *status_dev)
{
    // one trip: rows, watch, draw.  *nwatched: draws an accepted segmented draw recorded, to be decided again
    auto trip = [&](bool exact, DrawWatch &watch, unsigned int *nwatched) -> int {
        *nwatched = 0;
        int rc;
        if ((rc = f.forward(exact)))
            return rc;
        if (exact) {
            c->last.draw_fwd_segmented = false;
            c->last.draw_alpha_dev = 0.0;
        }
        // rows of a segmented pass: draws within 64 x the deviation its boundary check measured are recorded
        if ((rc = draw_watch_prepare(c, c->last.draw_fwd_segmented ? 64.0 * std::max(c->last.draw_alpha_dev, 1e-16) : 0.0,
                                     watch, nullptr)))
            return rc;
        BHMM_HIP(hipMemsetAsync(status_dev, 0, sizeof(int), c->stream));
        c->last.smp_segmented = false;
        bool seg_done = false;
        Segs sg;
        if (segments_allowed && c->opt.spec_enabled) {
            if ((rc = wide_path_plan(c, 1, plan::draw_seglen(c->total, want_segments), sg)))
                return rc;
            seg_done = sg.nseg > c->K; // (else one segment per trajectory: the serial kernel)
        }
        if (seg_done) {
            if (c->ds.smp_W <= 0)
                c->ds.smp_W = plan::DRAW_W_START;
            sg.W = c->ds.smp_W;
            if ((f.prepare && (rc = f.prepare(sg))) || (rc = c->d_sentry.ensure((size_t)sg.nseg)) ||
                (rc = c->d_sexit.ensure((size_t)sg.nseg)) || (rc = c->d_vflag.ensure((size_t)sg.nseg)) ||
                (rc = ensure_specres(c)))
                return rc;
            const unsigned int *h = c->h_specres;
            int round = 0;
            for (; round <= plan::DRAW_MAX_ROUNDS; ++round) {
                if ((rc = specres_reset(c)))
                    return rc;
                lds_poison(c->stream);
                if ((rc = f.pass(round > 0, sg, watch)))
                    return rc;
                BHMM_HIP(launch(k_wide_smp_check, dim3((sg.nseg + 255) / 256), dim3(256), 0, c->stream, sg, c->d_sentry.p,
                                c->d_sexit.p, c->d_vflag.p, c->d_specres.p));
                if ((rc = specres_read(c, 4, false)))
                    return rc;
                BHMM_HIP(hipMemcpyAsync(&c->h_specres[0], status_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
                BHMM_HIP(hipStreamSynchronize(c->stream));
                if (round == 0)
                    c->last.smp_seg_mismatch = (int)h[3];
                if (h[3] == 0)
                    break;
            }
            c->last.smp_seg_rounds = round;
            // (a draw that found no state may belong to a segment that was drawn again afterwards:
            // the serial kernel decides such a call)
            seg_done = h[3] == 0 && h[0] == 0;
            if (!seg_done)
                BHMM_HIP(hipMemsetAsync(status_dev, 0, sizeof(int), c->stream));
            c->ds.smp_W = plan::draw_next_warmup(c->ds.smp_W, c->last.smp_seg_mismatch, sg.nseg);
            c->last.smp_segmented = seg_done;
        }
        if (!seg_done) {
            if (c->last.draw_fwd_segmented) { // (the serial draw has no watch: it reads rows of the serial recursion)
                if ((rc = f.forward(true)))
                    return rc;
                c->last.draw_fwd_segmented = false;
                c->last.draw_alpha_dev = 0.0;
            }
            return f.serial();
        }
        if (watch.count) {
            BHMM_HIP(hipMemcpyAsync(nwatched, watch.count, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
            BHMM_HIP(hipStreamSynchronize(c->stream));
        }
        return BHMM_OK;
    };
    DrawWatch watch;
    unsigned int nwatched = 0;
    const int rc = trip(false, watch, &nwatched);
    if (rc || !nwatched)
        return rc;
    // watched draws are decided again on the serial recursion over a long window; if one does not stand, the
    // second trip: the whole draw on the rows of the serial recursion (no watch, nothing to decide again)
    bool repeated = false;
    return draw_decide_again(c, A, pi, par0, par1, nwatched, watch.tol, [&] { return trip(true, watch, &nwatched); },
                             &repeated);
}

namespace {

// ---- Viterbi, up to 64 states: one function per path (what they share: VitCall, viterbi_host.hpp) ----
// Emission probabilities in a separate, fully parallel pass when the (total, n) matrix fits (it is what the
// reference materialises anyway, maximum_likelihood.py:345-347) -- unless the kernels of the run evaluate them
template <int KIND>
hipError_t launch_pobs(bhmm_ctx *c, const WideModel &m, const void *obs)
{
    // one thread per element where n is a power of two (coalesced stores), else per step
    const dim3 pl((unsigned)(((size_t)c->total * c->n + 256 * POBS_LANES_R - 1) / (256 * POBS_LANES_R)));
    auto lanes = [&](auto nl) {
        return launch(k_pobs_lanes<KIND, decltype(nl)::value>, pl, dim3(256), 0, c->stream, m, obs, c->total, c->d_alpha_rm.p);
    };
    switch (c->n) {
    case 2: return lanes(std::integral_constant<int, 2>());
    case 4: return lanes(std::integral_constant<int, 4>());
    case 8: return lanes(std::integral_constant<int, 8>());
    case 16: return lanes(std::integral_constant<int, 16>());
    case 32: return lanes(std::integral_constant<int, 32>());
    case 64: return lanes(std::integral_constant<int, 64>());
    }
    return launch(k_pobs_all<KIND>, dim3((unsigned)((c->total + 255) / 256)), dim3(256), 0, c->stream, m, obs, c->total,
                  c->d_alpha_rm.p);
}
int viterbi_emissions(bhmm_ctx *c, const WideModel &m, VitCall &v)
{
    // n <= 8 with a chunk plan: the chunk-parallel kernel evaluates the emission itself (gathers from B / evaluates the
    // gaussian density): no (total, n) emission matrix is written and re-read
    const bool disc_direct = !c->wide && c->kind != EMIT_EXPL && c->opt.spec_enabled && c->G > c->K;
    // 9..64 states over time segments, discrete: the kernel gathers from B itself (no (total, n) matrix).  Measured
    // for the Gaussian kind too: the division by sigma and the exponential in every step, warm-ups included, cost more
    // than the matrix pass saves (64 states: 9.0 -> 9.7 ms, 16: 0.67 -> 0.81).  (round 6: the Gaussian density in the
    // step too, with the reciprocal-based quotient and the one-block exponential of k_pobs_lanes -- at 64 states:
    // 6.5 GB less written and read again per call)
    const bool wide_direct = c->wide && (c->kind == EMIT_DISC || c->kind == EMIT_GAUSS) && c->opt.spec_enabled &&
                             !c->ds.vit.seg_given_up;
    if (c->kind == EMIT_EXPL || disc_direct || wide_direct)
        return BHMM_OK;
    size_t freeb = 0, totb = 0;
    const size_t need = (size_t)c->total * c->n * sizeof(double);
    if (hipMemGetInfo(&freeb, &totb) == hipSuccess && need + ((size_t)1 << 30) < freeb + c->d_alpha_rm.n * sizeof(double) &&
        c->d_alpha_rm.ensure((size_t)c->total * c->n) == BHMM_OK) {
        BHMM_HIP(c->kind == EMIT_GAUSS ? launch_pobs<EMIT_GAUSS>(c, m, v.obs) : launch_pobs<EMIT_DISC>(c, m, v.obs));
        v.obs = c->d_alpha_rm.p;
        v.kind = EMIT_EXPL;
    } else {
        (void)hipGetLastError();
    }
    return BHMM_OK;
}

// ---- 8 states and fewer with a chunk plan: the chunk-parallel run (k_viterbi_chunks); its back-pointers are
// accepted only if every chunk boundary verifies and no decision was close ----
// Back-trace of such a run (k_vit_walk, maps -> stitch -> paths), parallel over chunks; VNP lanes per chunk (models
// of up to four states: four lanes, 16 chunks per wavefront)
template <int VNP>
hipError_t chunk_walks(bhmm_ctx *c, const VitCall &v)
{
    const int K = c->K, n = c->n;
    const Chunks chs = chunks_of(c);
    const dim3 wg((c->G + 64 / VNP - 1) / (64 / VNP));
    uint32_t *vmaps = reinterpret_cast<uint32_t *>(v.path + c->total); // chunk maps,
    int32_t *vend = reinterpret_cast<int32_t *>(vmaps + c->Gp);        // state at each chunk's end,
    int32_t *vcoal = vend + c->Gp; // step below which the map pass wrote the path itself (k_vit_walk)
    return v.out([&](auto *out) {
        using PT = std::remove_pointer_t<decltype(out)>;
        hipError_t e = launch(k_vit_walk<VNP, false, PT>, wg, dim3(64), 0, c->stream, chs, c->G, n, v.ptr, nullptr, vmaps, out,
                              vcoal);
        if (e == hipSuccess)
            e = (int64_t)c->G >= (int64_t)32 * K
                    ? launch(k_smp_stitch, dim3(K), dim3(64), 0, c->stream, c->d_traj_c0.p, K, 1, vmaps, vend, v.last)
                    : launch(k_smp_stitch_serial, dim3((K + SMP_STITCH_TPB - 1) / SMP_STITCH_TPB), dim3(64), 0, c->stream,
                             c->d_traj_c0.p, K, 1, vmaps, vend, v.last);
        if (e == hipSuccess)
            e = launch(k_vit_walk<VNP, true, PT>, wg, dim3(64), 0, c->stream, chs, c->G, n, v.ptr, vend, nullptr, out, vcoal);
        return e;
    });
}
// A warm-up too short for some boundary (the survivors of that stretch had not met yet) shows as a boundary out of
// tolerance: the run is repeated with a longer one (~1 ms a pass) before the serial kernel (tens of ms) has to decide.
// The warm-up is THIS recursion's (round 4): the max-product chains coalesce faster than the E-step's filter forgets
// (configs[1]: bit-identical boundaries from W ~ 128 on, the probe says 280); the lengths: plan::vit_chunk_attempts
template <int VNP>
int chunk_viterbi(bhmm_ctx *c, const WideModel &m, const VitCall &v, bool *done)
{
    const int K = c->K, n = c->n;
    int maxchunks = 1, rc;
    for (int k = 0; k < K; ++k)
        maxchunks = std::max(maxchunks, c->traj_c0[k + 1] - c->traj_c0[k]);
    const double tol = 1e-11, margin = std::max(1e-7, 16.0 * tol * maxchunks);
    if ((rc = c->d_aentry.ensure((size_t)c->Gp * 8)) || (rc = c->d_aexit.ensure((size_t)c->Gp * 8)) ||
        (rc = ensure_specres(c)))
        return rc;
    const Chunks chs = chunks_of(c);
    // discrete: B in LDS when it is small enough to leave four wavefronts per SIMD their room
    const size_t smB = (v.kind == EMIT_DISC && (size_t)n * c->M * sizeof(double) <= 16 * 1024) ? (size_t)n * c->M * sizeof(double) : 0;
    const unsigned int *h = c->h_specres;
    bool walks_in_flight = false;
    // one attempt at warm-up W: first without the close-decision count (bit-identical boundaries make it
    // irrelevant), then with it
    auto attempt = [&](int W, bool first, plan::ChunkVerdict *verdict) -> int {
        for (int pass = 0; pass < 2; ++pass) {
            if (int rca = specres_reset(c))
                return rca;
            hipError_t e = dispatch_kind(v.kind, [&](auto kc) {
                constexpr int KIND = decltype(kc)::value;
                auto *k = pass > 0 ? k_viterbi_chunks<VNP, KIND, true> : k_viterbi_chunks<VNP, KIND, false>;
                return launch(k, dim3((c->G + 64 / VNP - 1) / (64 / VNP)), dim3(64), smB, c->stream, m, chs, c->G,
                              c->d_offsets.p, v.obs, W, margin, v.ptr, v.last, c->d_aentry.p, c->d_aexit.p, c->d_specres.p,
                              smB ? 1 : 0);
            });
            if (e == hipSuccess)
                e = launch(k_viterbi_check<VNP>, dim3((c->G + 255) / 256), dim3(256), 0, c->stream, chs, c->G,
                           c->d_aentry.p, c->d_aexit.p, tol, c->d_specres.p);
            BHMM_HIP(e);
            if (int rca = specres_read(c, 4, false))
                return rca;
            // the normal case is "all boundaries bit-identical": the back-trace is enqueued behind the first pass
            // before its verdict is known (one host round trip less); the walks only read back-pointers, which are
            // valid state indices whatever the verdict, and are repeated after any further pass
            const bool speculative = first && pass == 0;
            if (speculative)
                BHMM_HIP(chunk_walks<VNP>(c, v));
            BHMM_HIP(hipStreamSynchronize(c->stream));
            walks_in_flight = speculative && h[3] == 0;
            if (h[3] == 0 || h[0] != 0)
                break; // the serial run outright / out of tolerance: the count cannot help
        }
        // all boundaries bit-identical: it is the serial run; else within tolerance and no close decision
        verdict->accepted = h[3] == 0 || (h[0] == 0 && h[2] == 0);
        verdict->within = h[0] == 0;
        return BHMM_OK;
    };
    plan::ChunkVerdict verdict;
    if ((rc = plan::vit_chunk_attempts(c->ds.vit.W, c->ds.vit.bad, c->ds.vit.explore, c->ds.spec_W, c->opt.spec_W_fixed,
                                       attempt, &verdict)))
        return rc;
    *done = c->last.viterbi_chunked = verdict.accepted;
    memcpy(&c->last.spec_last_dev, &h[1], sizeof(float));
    c->last.viterbi_close = h[2];
    if (*done && !walks_in_flight)
        BHMM_HIP(chunk_walks<VNP>(c, v));
    return BHMM_OK;
}

// ---- 9..64 states: one lane group per time segment (k_wide_viterbi_seg), accepted by seg_viterbi ----
// Warm-up: its own, not the E-step's.  Every length is exact (bitwise check + fix-up rounds), so it only trades
// warm-up steps against rounds (1.1 ms each at configs[3], whatever the number of flagged segments), and the E-step's
// length says little about that: its check asks for 1e-11 on every boundary -- 904 steps after a dozen EM iterations
// on configs[3] --, while the max-product vectors are within rounding noise of their predecessors' after 128 (one
// round either way: 17.6 ms against 23.6).  The lengths: plan::vit_wide_w_start, vit_next_warmup
int wide_seg_viterbi(bhmm_ctx *c, const WideModel &m, const VitCall &v, bool *done)
{
    const int K = c->K, n = c->n, NP = c->N, GP = 64 / NP;
    const int W_estep = plan::vit_w_estep(c->ds.spec_W);
    int W_try = plan::vit_wide_w_start(c->ds.vit.W, W_estep), rc;
    double *vall = vit_vall(c, c->opt.vit_margin && c->ds.vit.margin_want);
    const int64_t maxT = longest_traj(c);
    for (int attempt = 0; attempt < 2 && !*done; ++attempt) {
        if (attempt > 0)
            W_try *= 2;
        const int64_t seglen =
            plan::vit_wide_seglen(c->total, NP, c->num_simd, c->opt.vit_seg_per_simd, c->opt.vit_seg_warmups, W_try);
        Segs sg;
        if ((rc = wide_path_plan(c, 0, seglen, sg)))
            return rc;
        if (sg.nseg <= K)
            break; // nothing to gain: one segment per trajectory is the serial kernel
        sg.W = W_try;
        if ((rc = vit_boundary_bufs(c, sg, NP)))
            return rc;
        const dim3 sgrid((sg.nseg + GP * WVS_WPB - 1) / (GP * WVS_WPB)), sblk(64 * WVS_WPB);
        auto seg_kernel = [&](bool fix, uint8_t *flag, double *kept, double tol, unsigned int *notmet) {
            return dispatch_np<16>(NP, [&](auto npc) {
                return dispatch_kind(v.kind, [&](auto kc) {
                    constexpr int V = decltype(npc)::value, KIND = decltype(kc)::value;
                    return launch(fix ? k_wide_viterbi_seg<V, KIND, true> : k_wide_viterbi_seg<V, KIND, false>, sgrid, sblk, 0,
                                  c->stream, m, c->d_offsets.p, sg, v.obs, v.ptr, v.last, c->d_aentry.p, c->d_aexit.p, c->d_vckpt.p,
                                  flag, kept, tol, notmet);
                });
            });
        };
        SegViterbi f;
        f.pass = [&](bool fix) -> int {
            BHMM_HIP(seg_kernel(fix, c->d_vflag.p, fix ? nullptr : vall, 0.0, nullptr));
            BHMM_HIP(dispatch_np<16>(NP, [&](auto npc) {
                return launch(k_wide_vit_check<decltype(npc)::value>, dim3((sg.nseg + 255) / 256), dim3(256), 0, c->stream, sg,
                              c->d_aentry.p, c->d_aexit.p, c->d_vflag.p, c->d_specres.p, (!fix && vall) ? SEG_VIT_TOL : 0.0);
            }));
            return BHMM_OK;
        };
        f.mend = [&]() -> int {
            BHMM_HIP(seg_kernel(true, c->d_vflag.p + sg.nseg, vall, SEG_VIT_TOL, c->d_specres.p + 1));
            return BHMM_OK;
        };
        f.margins = [&](double margin) { return vit_margins<1>(c, v, sg, m.A, vit_margin_lds(n), vall, margin); };
        // back-trace on a plan of its own, eight times finer than the pass's: a walk is a chain of dependent
        // look-ups, its time the length of a segment (configs[3]: 2 x 0.49 ms on the 2048 segments of the pass)
        f.walks = [&]() -> int {
            Segs sgw;
            if (int rcw = wide_path_plan(c, 2, std::max<int64_t>(256, c->ds.pplan[0].seglen / 8), sgw))
                return rcw;
            sgw.W = 0;
            return vit_walks<1>(c, v, sgw, c->pplan_buf[2].traj0.p);
        };
        SegVitResult r;
        if ((rc = seg_viterbi(c, f, sg, seglen, vall, maxT, 12, false, &r)))
            return rc;
        // (a round runs as long as its longest flagged segment needs to fall onto a vector of the first pass again:
        // 1.1 ms at configs[3] on white-noise observations, 6.7 ms -- half a first pass -- on observations drawn from
        // the model, where 1800 of 2048 boundaries carry rounding noise.  The margins cost about 1.3 ms there: wanted
        // from the next call on when rounds were many, or the flagged segments more than a quarter)
        if (r.rounds >= 2 || (r.rounds >= 1 && !r.margin_accepted && (int64_t)c->last.vit_seg_mismatch * 4 > sg.nseg))
            c->ds.vit.margin_want = true;
        // (How many boundaries the first pass left to the fix-up does not say whether the warm-up was too short -- most
        // are rounding noise, a round costs the same for one as for a thousand: doubling on that count was slower.)
        if ((*done = r.accepted))
            vit_accepted(c, r, vall, W_try, W_estep);
    }
    vit_attempts_done(c, *done);
    return BHMM_OK;
}

// ---- one lane group per trajectory (k_wide_viterbi_fwd) and the trace: what no time-parallel run decided ----
int serial_viterbi(bhmm_ctx *c, const WideModel &m, const VitCall &v)
{
    const int K = c->K, NP = c->wide ? c->N : 8, GP = 64 / NP;
    // U trajectories per lane group.  Measured on configs[1] (256 trajectories): the kernel is bound by the instruction
    // stream of each wavefront, not by latency, and SIMDs are plentiful (32 of 1024 busy), so U = 1 is fastest (U = 4
    // was 3.5x slower); the parameter stays for batches with more trajectories than SIMD slots.
    constexpr int U = 1;
    BHMM_HIP(dispatch_np(NP, [&](auto npc) {
        return dispatch_kind(v.kind, [&](auto kc) {
            return launch(k_wide_viterbi_fwd<decltype(npc)::value, decltype(kc)::value, U>, dim3((K + GP * U - 1) / (GP * U)),
                          dim3(64), 0, c->stream, m, c->d_offsets.p, K, v.obs, v.ptr, v.last);
        });
    }));
    BHMM_HIP(v.out([&](auto *p) {
        return launch(k_wide_viterbi_trace<std::remove_pointer_t<decltype(p)>>, dim3(K), dim3(64), 0, c->stream,
                      c->d_offsets.p, K, c->n, v.ptr, v.last, p);
    }));
    return BHMM_OK;
}

int wide_viterbi_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                     const double *par1, void *paths_out, int out_fmt)
{
    WideModel m;
    int rc = wide_model(c, c->kind, A, pi, par0, par1, m);
    if (rc)
        return rc;
    c->last.viterbi_chunked = false;
    c->last.vit_mended = 0;
    const size_t gpad = c->wide ? 0 : (size_t)c->Gp; // (the chunk maps of chunk_walks behind the paths)
    if ((rc = c->d_scratch.ensure((size_t)c->total * c->n)) ||
        (rc = c->d_scratch2.ensure(((size_t)c->total + c->K + 3 * gpad) * sizeof(int32_t))))
        return rc;
    VitCall v = vit_call(c, paths_out, out_fmt, c->d_obs_rm.p, c->kind);
    if ((rc = viterbi_emissions(c, m, v)))
        return rc;
    bool done = false;
    if (!c->wide && c->opt.spec_enabled && c->G > c->K)
        rc = c->n <= 4 ? chunk_viterbi<4>(c, m, v, &done) : chunk_viterbi<8>(c, m, v, &done);
    else if (c->wide && c->opt.spec_enabled && !c->ds.vit.seg_given_up)
        rc = wide_seg_viterbi(c, m, v, &done);
    if (rc || (!done && (rc = serial_viterbi(c, m, v))))
        return rc;
    return deliver_paths(c, paths_out, out_fmt, v.path);
}

int wide_sample_run(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                    const double *par1, const double *u, uint64_t seed, int32_t *paths,
                    int64_t *counts, int64_t *n0, double *emis, double *stats_dev)
{
    WideModel m; // (the forward passes upload the same block again: m stays valid)
    int rc = wide_model(c, c->kind, A, pi, par0, par1, m);
    if (rc)
        return rc;
    const int K = c->K, n = c->n, NP = c->N, GP = 64 / NP;
    const size_t nstat = (size_t)n * n + n;
    const size_t esz = c->kind == EMIT_GAUSS ? 3 * (size_t)n
                                             : (c->kind == EMIT_DISC ? (size_t)n * c->M : 0);
    if ((rc = c->d_scratch2.ensure(((size_t)c->total + 4) * sizeof(int32_t))))
        return rc;
    int32_t *path = reinterpret_cast<int32_t *>(c->d_scratch2.p);
    int *status = reinterpret_cast<int *>(path + c->total);
    const size_t dbl = nstat + (size_t)K * esz + esz + (u ? (size_t)c->total : 0) + 8;
    if ((rc = c->d_scratch.ensure(dbl * sizeof(double))))
        return rc;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(c->d_scratch.p);
    double *epart = reinterpret_cast<double *>(c->d_scratch.p) + nstat;
    double *ered = epart + (size_t)K * esz;
    double *udev = nullptr;
    if (u) {
        udev = ered + esz;
        BHMM_HIP(hipMemcpyAsync(udev, u, (size_t)c->total * sizeof(double), hipMemcpyHostToDevice,
                                c->stream));
    }
    BHMM_HIP(hipMemsetAsync(cnt, 0, nstat * sizeof(unsigned long long), c->stream));
    if (esz)
        BHMM_HIP(hipMemsetAsync(ered, 0, esz * sizeof(double), c->stream));
    const int64_t *off = c->d_offsets.p;
    // parallel over time segments where that fills more of the device than the trajectories do
    // (k_wide_sample_seg), by the protocol of seg_draw; alpha (row-major, any scale per row) in d_alpha_rm
    SegDraw f;
    f.forward = [&](bool exact) {
        return exact ? wide_forward(c, A, pi, par0, par1) : wide_forward_draw(c, A, pi, par0, par1);
    };
    f.pass = [&](bool fix, const Segs &sg, const DrawWatch &watch) -> int {
        const dim3 sgrid((sg.nseg + GP * WVS_WPB - 1) / (GP * WVS_WPB)), sblk(64 * WVS_WPB);
        auto *k = NP == 16   ? (fix ? k_wide_sample_seg<16, true> : k_wide_sample_seg<16, false>)
                  : NP == 32 ? (fix ? k_wide_sample_seg<32, true> : k_wide_sample_seg<32, false>)
                             : (fix ? k_wide_sample_seg<64, true> : k_wide_sample_seg<64, false>);
        BHMM_HIP(launch(k, sgrid, sblk, 0, c->stream, m, off, sg, c->d_alpha_rm.p, udev, seed, path, status, c->d_soff.p,
                        c->d_sentry.p, c->d_sexit.p, c->d_vflag.p, watch));
        return BHMM_OK;
    };
    f.serial = [&]() -> int {
        auto *ks = NP == 16 ? k_wide_sample_path<16> : NP == 32 ? k_wide_sample_path<32> : k_wide_sample_path<64>;
        BHMM_HIP(launch(ks, dim3((K + GP - 1) / GP), dim3(64), 0, c->stream, m, off, K, c->d_alpha_rm.p, udev, seed, path,
                        status, c->d_soff.p));
        return BHMM_OK;
    };
    if ((rc = seg_draw(c, f, A, pi, par0, par1, true, (int64_t)c->opt.smp_seg_per_simd * c->num_simd * GP, status)))
        return rc;
    if (counts || n0 || emis || stats_dev) {
        // the per-trajectory emission table in LDS, or -- alphabets too large for it -- in epart itself
        const bool gtab = c->kind == EMIT_DISC &&
                          esz * sizeof(double) + nstat * sizeof(unsigned int) > (size_t)150 * 1024;
        const size_t sm = (gtab ? 0 : esz * sizeof(double)) + nstat * sizeof(unsigned int);
        if (gtab)
            BHMM_HIP(hipMemsetAsync(epart, 0, (size_t)K * esz * sizeof(double), c->stream));
        const void *obs = c->d_obs_rm.p;
        auto *kst = c->kind == EMIT_GAUSS  ? k_wide_path_stats<EMIT_GAUSS>
                    : c->kind == EMIT_DISC ? k_wide_path_stats<EMIT_DISC>
                                           : k_wide_path_stats<EMIT_EXPL>;
        BHMM_HIP(launch(kst, dim3(K), dim3(256), sm, c->stream, m, off, obs, path, cnt, epart, gtab ? 1 : 0));
        if (esz)
            BHMM_HIP(launch(k_add_partials, dim3((unsigned)esz), dim3(64), 0, c->stream, epart, K, (int)esz, ered));
    }
    std::vector<unsigned long long> hc(nstat);
    std::vector<double> he(esz);
    int hstatus = 0;
    if (stats_dev) {
        BHMM_HIP(launch(k_pack_path_stats, dim3(16), dim3(256), 0, c->stream, cnt, ered, n, n, c->M, c->kind, 0, stats_dev));
    } else {
        BHMM_HIP(hipMemcpyAsync(hc.data(), cnt, nstat * sizeof(unsigned long long),
                                hipMemcpyDeviceToHost, c->stream));
        if (esz)
            BHMM_HIP(hipMemcpyAsync(he.data(), ered, esz * sizeof(double), hipMemcpyDeviceToHost,
                                    c->stream));
    }
    BHMM_HIP(hipMemcpyAsync(&hstatus, status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (paths)
        BHMM_HIP(hipMemcpyAsync(paths, path, (size_t)c->total * sizeof(int32_t),
                                hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    if (hstatus) {
        set_error("random choice found no state: alpha/A not normalisable (_hidden.c:299-304)");
        return hstatus;
    }
    if (stats_dev)
        return BHMM_OK;
    if (counts)
        for (size_t e = 0; e < (size_t)n * n; ++e)
            counts[e] = (int64_t)hc[e];
    if (n0)
        for (int i = 0; i < n; ++i)
            n0[i] = (int64_t)hc[(size_t)n * n + i];
    if (emis && esz)
        memcpy(emis, he.data(), esz * sizeof(double)); // gaussian [3][n]; discrete [n][M]
    return BHMM_OK;
}

struct TmpCtx {
    bhmm_ctx *c = nullptr;
    ~TmpCtx() { bhmm_ctx_destroy(c); }
};

int cur_device()
{
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) {
        (void)hipGetLastError();
        d = 0;
    }
    return d;
}

} // namespace

} // namespace bhmm

using namespace bhmm;

extern "C" {

int bhmm_viterbi_batch(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                       const double *par1, int32_t *paths)
{
    if (int rc = enter_model_call(c, A && pi && paths, "NULL argument", true, par0, par1))
        return rc;
    if (c->gen)
        return gen_viterbi_run(c, A, pi, par0, par1, paths, 0);
    // all state counts up to 64 use the LDS-exchange kernels (k_wide_viterbi_*)
    return wide_viterbi_run(c, A, pi, par0, par1, paths, 0);
}

int bhmm_viterbi_batch_u8(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                          const double *par1, uint8_t *paths, int paths_on_device)
{
    if (int rc = enter_model_call(c, A && pi && paths, "NULL argument", true, par0, par1))
        return rc;
    if (c->gen)
        return gen_viterbi_run(c, A, pi, par0, par1, paths, paths_on_device ? 2 : 1);
    return wide_viterbi_run(c, A, pi, par0, par1, paths, paths_on_device ? 2 : 1);
}

int bhmm_sample_paths(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                      const double *par1, const double *u, uint64_t seed, int32_t *paths,
                      int64_t *counts, int64_t *n0, double *emis)
{
    if (int rc = enter_model_call(c, A && pi, "NULL argument", false, par0, par1))
        return rc;
    if (c->gen)
        return gen_sample_run(c, A, pi, par0, par1, u, seed, paths, counts, n0, emis, nullptr);
    if (c->wide)
        return wide_sample_run(c, A, pi, par0, par1, u, seed, paths, counts, n0, emis, nullptr);
    switch (c->N) {
    case 2:
        return sample_run<2>(c, A, pi, par0, par1, u, seed, paths, counts, n0, emis, nullptr);
    case 4:
        return sample_run<4>(c, A, pi, par0, par1, u, seed, paths, counts, n0, emis, nullptr);
    default:
        return sample_run<8>(c, A, pi, par0, par1, u, seed, paths, counts, n0, emis, nullptr);
    }
}

int bhmm_ctx_set_stream_offsets(bhmm_ctx *c, const int64_t *soff)
{
    if (!c || c->kind < 0)
        return invalid_arg("no observations loaded");
    BHMM_HIP(hipSetDevice(c->device));
    if (!soff) {
        c->d_soff.release();
        return BHMM_OK;
    }
    int rc = c->d_soff.ensure((size_t)std::max(c->K, 1));
    if (rc)
        return rc;
    BHMM_HIP(hipMemcpy(c->d_soff.p, soff, (size_t)c->K * sizeof(int64_t), hipMemcpyHostToDevice));
    return BHMM_OK;
}

int bhmm_ctx_path_stats_size(const bhmm_ctx *c)
{
    if (!c || c->kind < 0)
        return 0;
    const int n = c->n;
    return n * n + n + (c->kind == EMIT_GAUSS ? 3 * n : (c->kind == EMIT_DISC ? n * c->M : 0));
}

int bhmm_sample_paths_dev(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                          const double *par1, const double *u, uint64_t seed, int32_t *paths,
                          double *stats_dev)
{
    if (int rc = enter_model_call(c, A && pi && stats_dev, "NULL argument", false, par0, par1))
        return rc;
    if (c->gen)
        return gen_sample_run(c, A, pi, par0, par1, u, seed, paths, nullptr, nullptr, nullptr,
                              stats_dev);
    if (c->wide)
        return wide_sample_run(c, A, pi, par0, par1, u, seed, paths, nullptr, nullptr, nullptr,
                               stats_dev);
    switch (c->N) {
    case 2:
        return sample_run<2>(c, A, pi, par0, par1, u, seed, paths, nullptr, nullptr, nullptr, stats_dev);
    case 4:
        return sample_run<4>(c, A, pi, par0, par1, u, seed, paths, nullptr, nullptr, nullptr, stats_dev);
    default:
        return sample_run<8>(c, A, pi, par0, par1, u, seed, paths, nullptr, nullptr, nullptr, stats_dev);
    }
}

int bhmm_viterbi(int32_t *path, const double *A, const double *pobs, const double *pi, int N,
                 int64_t T)
{
    if (!path || !A || !pobs || !pi || N < 1 || T < 1)
        return invalid_arg("NULL argument or empty problem");
    TmpCtx t;
    int rc = bhmm_ctx_create(&t.c, cur_device(), nullptr);
    if (rc)
        return rc;
    const int64_t off[2] = {0, T};
    rc = bhmm_ctx_set_observations(t.c, BHMM_EMIT_EXPLICIT, pobs, off, 1, N, 0, 0, 0);
    if (rc)
        return rc;
    return bhmm_viterbi_batch(t.c, A, pi, nullptr, nullptr, path);
}

int bhmm_sample_path(int32_t *path, const double *alpha, const double *A, const double *u, int N,
                     int64_t T)
{
    if (!path || !alpha || !A || !u || N < 1 || T < 1)
        return invalid_arg("NULL argument or empty problem");
    if (N > 64)
        return gen_sample_path(path, alpha, A, u, N, T);
    Tmp tmp;
    double *d_alpha, *d_u;
    int64_t *d_off;
    int32_t *d_path;
    int *d_status;
    int rc;
    if ((rc = tmp.alloc(&d_alpha, (size_t)T * N)) || (rc = tmp.alloc(&d_u, (size_t)T)) ||
        (rc = tmp.alloc(&d_off, 2)) || (rc = tmp.alloc(&d_path, (size_t)T)) ||
        (rc = tmp.alloc(&d_status, 1)))
        return rc;
    const int64_t off[2] = {0, T};
    BHMM_HIP(hipMemcpy(d_alpha, alpha, (size_t)T * N * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(d_u, u, (size_t)T * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(d_off, off, sizeof(off), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemset(d_status, 0, sizeof(int)));
    if (N > 8) {
        double *d_A;
        if ((rc = tmp.alloc(&d_A, (size_t)N * N)))
            return rc;
        BHMM_HIP(hipMemcpy(d_A, A, (size_t)N * N * sizeof(double), hipMemcpyHostToDevice));
        WideModel m;
        memset(&m, 0, sizeof(m));
        m.A = d_A;
        m.n = N;
        auto *k = N <= 16 ? k_wide_sample_path<16> : N <= 32 ? k_wide_sample_path<32> : k_wide_sample_path<64>;
        BHMM_HIP(launch(k, dim3(1), dim3(64), 0, 0, m, d_off, 1, d_alpha, d_u, (uint64_t)0, d_path, d_status, nullptr));
        int stw = 0;
        BHMM_HIP(hipMemcpy(path, d_path, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost));
        BHMM_HIP(hipMemcpy(&stw, d_status, sizeof(int), hipMemcpyDeviceToHost));
        if (stw) {
            set_error("random choice found no state: p not normalised (_hidden.c:299-304)");
            return stw;
        }
        return BHMM_OK;
    }
    const int NP = pad_states(N);
    std::vector<double> pi(N, 0.0);
#define BHMM_SAMPLE_CASE(NN)                                                                    \
    {                                                                                           \
        Model<NN> m;                                                                            \
        fill_model<NN>(m, N, EMIT_EXPL, 0, A, pi.data(), nullptr, nullptr);                 \
        BHMM_HIP(launch(k_sample_path<NN>, dim3(1), dim3(64), 0, 0, m, d_off, 1, d_alpha, d_u,    \
                        (uint64_t)0, d_path, d_status));                                        \
    }
    if (NP == 2)
        BHMM_SAMPLE_CASE(2)
    else if (NP == 4)
        BHMM_SAMPLE_CASE(4)
    else
        BHMM_SAMPLE_CASE(8)
    int st = 0;
    BHMM_HIP(hipMemcpy(path, d_path, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost));
    BHMM_HIP(hipMemcpy(&st, d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) {
        set_error("random choice found no state: p not normalised (_hidden.c:299-304)");
        return st;
    }
    return BHMM_OK;
}

int bhmm_libc_uniforms(double *u, int64_t T, int seed)
{
    if (!u || T < 0)
        return invalid_arg("NULL argument");
    if (seed >= 0)
        srand((unsigned)seed); // _hidden.c:321-327
    for (int64_t t = T - 1; t >= 0; --t)
        u[t] = (double)rand() / ((double)RAND_MAX + 1.0); // _hidden.c:285-287
    return BHMM_OK;
}

int bhmm_state_probabilities(double *gamma, const double *alpha, const double *beta, int N,
                             int64_t T)
{
    if (!gamma || !alpha || !beta || N < 1 || T < 1)
        return invalid_arg("NULL argument or empty problem");
    Tmp tmp;
    double *da, *db, *dg;
    int rc;
    const size_t cnt = (size_t)T * N;
    if ((rc = tmp.alloc(&da, cnt)) || (rc = tmp.alloc(&db, cnt)) || (rc = tmp.alloc(&dg, cnt)))
        return rc;
    BHMM_HIP(hipMemcpy(da, alpha, cnt * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(db, beta, cnt * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(launch(k_gamma_rows, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, 0, da, db, dg, N, T));
    BHMM_HIP(hipMemcpy(gamma, dg, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return BHMM_OK;
}

int bhmm_transition_counts(double *C, const double *A, const double *pobs, const double *alpha,
                           const double *beta, int N, int64_t T)
{
    if (!C || !A || !pobs || !alpha || !beta || N < 1 || T < 1)
        return invalid_arg("NULL argument or empty problem");
    if (N > 64)
        return gen_transition_counts(C, A, pobs, alpha, beta, N, T);
    if (N > 8)
        return wide_transition_counts(C, A, pobs, alpha, beta, N, T);
    Tmp tmp;
    double *dA, *dp, *da, *db, *dpart, *dC;
    int rc;
    const size_t cnt = (size_t)T * N;
    const int nblk = (int)std::min<int64_t>(1024, (T + 255) / 256);
    const int NP = pad_states(N);
    if ((rc = tmp.alloc(&dA, (size_t)N * N)) || (rc = tmp.alloc(&dp, cnt)) ||
        (rc = tmp.alloc(&da, cnt)) || (rc = tmp.alloc(&db, cnt)) ||
        (rc = tmp.alloc(&dpart, (size_t)nblk * NP * NP)) || (rc = tmp.alloc(&dC, (size_t)N * N)))
        return rc;
    BHMM_HIP(hipMemcpy(dA, A, (size_t)N * N * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(dp, pobs, cnt * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(da, alpha, cnt * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(db, beta, cnt * sizeof(double), hipMemcpyHostToDevice));
#define BHMM_XI_CASE(NN)                                                                        \
    {                                                                                           \
        BHMM_HIP(launch(k_xi_rows<NN>, dim3(nblk), dim3(256), 0, 0, dA, dp, da, db, N, T, dpart));  \
        BHMM_HIP(launch(k_sum_partials<NN>, dim3(1), dim3(64), 0, 0, dpart, nblk, N, dC));       \
    }
    if (NP == 2)
        BHMM_XI_CASE(2)
    else if (NP == 4)
        BHMM_XI_CASE(4)
    else
        BHMM_XI_CASE(8)
    BHMM_HIP(hipMemcpy(C, dC, (size_t)N * N * sizeof(double), hipMemcpyDeviceToHost));
    return BHMM_OK;
}

int bhmm_pobs_gaussian(double *pobs, const double *obs, const double *mu, const double *sigma,
                       int N, int64_t T, int ignore_outliers)
{
    if (!pobs || !obs || !mu || !sigma || N < 1 || T < 1)
        return invalid_arg("NULL argument or empty problem");
    Tmp tmp;
    double *dobs, *dmu, *dsig, *dp;
    int rc;
    if ((rc = tmp.alloc(&dobs, (size_t)T)) || (rc = tmp.alloc(&dmu, (size_t)N)) ||
        (rc = tmp.alloc(&dsig, (size_t)N)) || (rc = tmp.alloc(&dp, (size_t)T * N)))
        return rc;
    BHMM_HIP(hipMemcpy(dobs, obs, (size_t)T * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(dmu, mu, (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(dsig, sigma, (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(launch(k_pobs_gaussian, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, 0, dobs, dmu, dsig, dp, N, T,
                    ignore_outliers));
    BHMM_HIP(hipMemcpy(pobs, dp, (size_t)T * N * sizeof(double), hipMemcpyDeviceToHost));
    return BHMM_OK;
}

int bhmm_update_pout(double *pout, const int32_t *obs, const double *weights, int64_t T, int N,
                     int M)
{
    if (!pout || !obs || !weights || N < 1 || M < 1 || T < 1)
        return invalid_arg("NULL argument or empty problem");
    if ((size_t)N * M * sizeof(double) > 64 * 1024)
        return invalid_arg("N*M too large for the LDS histogram");
    Tmp tmp;
    int32_t *dobs;
    double *dw, *dpart, *dout;
    int rc;
    const int nblk = (int)std::min<int64_t>(512, (T + 255) / 256);
    if ((rc = tmp.alloc(&dobs, (size_t)T)) || (rc = tmp.alloc(&dw, (size_t)T * N)) ||
        (rc = tmp.alloc(&dpart, (size_t)nblk * N * M)) || (rc = tmp.alloc(&dout, (size_t)N * M)))
        return rc;
    BHMM_HIP(hipMemcpy(dobs, obs, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(dw, weights, (size_t)T * N * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(dout, pout, (size_t)N * M * sizeof(double), hipMemcpyHostToDevice));
    BHMM_HIP(launch(k_update_pout, dim3(nblk), dim3(256), (size_t)N * M * sizeof(double), 0, dobs, dw, T, N, M, dpart));
    BHMM_HIP(launch(k_add_partials, dim3(N * M), dim3(64), 0, 0, dpart, nblk, N * M, dout));
    BHMM_HIP(hipMemcpy(pout, dout, (size_t)N * M * sizeof(double), hipMemcpyDeviceToHost));
    return BHMM_OK;
}

} // extern "C"
