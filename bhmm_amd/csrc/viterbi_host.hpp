// viterbi_host.hpp -- what the segment-parallel Viterbi passes share on the host (9..64 states: path_api.hip,
// wide_seg_viterbi; 65..128 and 129..256: gen_api.hip, gen_seg_viterbi and gen_rows_viterbi): the buffers of a call,
// the margins and walks hooks of seg_viterbi (host_internal.hpp), the boundary buffers, the kept vectors and the
// bookkeeping after seg_viterbi.  Kernels, LDS sizes, grids, f.pass and f.mend are each pass's own; the integer
// rules are plan.hpp's (vit_*).
#pragma once
#include <type_traits>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "path_kernels.hpp"
#include "plan.hpp"
#include "seg_host.hpp"

namespace bhmm {

// What every path of one Viterbi call shares.  out_fmt: 0 = int32 paths to a host buffer (the reference's type,
// hidden.pyx:161-162), 1 = one byte per step to a host buffer, 2 = one byte per step into a device buffer of the
// context's device (written by the back-trace kernels directly, no copy at all)
struct VitCall {
    uint8_t *ptr = nullptr;    // back-pointers of every (step, state)
    int32_t *last = nullptr;   // [K] state at each trajectory's last step
    int32_t *path = nullptr;   // the paths, out_fmt 0 ...
    uint8_t *path8 = nullptr;  // ... 1 and 2
    int out_fmt = 0;
    const void *obs = nullptr; // the observations, or the emission matrix once it is materialised
    int kind = EMIT_EXPL;      // ... what obs holds (the effective kind of the kernels that read it)
    // f(path) or f(path8): the pointee is the path type of the kernel to launch
    template <class F>
    auto out(F f) const { return out_fmt == 0 ? f(path) : f(path8); }
};
// ... over the context's scratch buffers, which the caller has sized: back-pointers in d_scratch, [last | paths] in
// d_scratch2 (one byte per step: over the int32 paths, or where the caller wants them)
inline VitCall vit_call(bhmm_ctx *c, void *paths_out, int out_fmt, const void *obs, int kind)
{
    int32_t *last = reinterpret_cast<int32_t *>(c->d_scratch2.p), *path = last + c->K;
    uint8_t *path8 = out_fmt == 2 ? static_cast<uint8_t *>(paths_out) : reinterpret_cast<uint8_t *>(path);
    return VitCall{reinterpret_cast<uint8_t *>(c->d_scratch.p), last, path, path8, out_fmt, obs, kind};
}

// f.margins: k_vit_margin<PT, V[, false]> over the segments of plan 0 on the path the walks wrote (A: the matrix
// this instantiation reads, lds: its dynamic LDS)
inline size_t vit_margin_lds(int n) { return (size_t)n * (n | 1) * sizeof(double); } // (odd pitch, k_vit_margin)
template <int V, bool ALDS = true>
int vit_margins(bhmm_ctx *c, const VitCall &v, const Segs &sg, const double *A, size_t lds, const double *vall, double margin)
{
    const dim3 mgrid(sg.nseg, (unsigned)((c->ds.pplan[0].maxlen + VM_STEPS - 1) / VM_STEPS)); // (the longest REAL segment)
    BHMM_HIP(v.out([&](auto *p) {
        return launch(k_vit_margin<std::remove_pointer_t<decltype(p)>, V, ALDS>, mgrid, dim3(256), lds, c->stream, A, c->n,
                      c->d_offsets.p, sg, vall, p, margin, c->d_specres.p);
    }));
    return BHMM_OK;
}

// f.walks: back-trace over the segments sg -- maps, stitch (traj0: first segment of every trajectory in sg's plan),
// apply.  NC: column tiles of the back-pointer maps (64 states each)
template <int NC>
int vit_walks(bhmm_ctx *c, const VitCall &v, const Segs &sg, const int32_t *traj0)
{
    const int n = c->n, K = c->K;
    const int64_t *off = c->d_offsets.p;
    int rc;
    if ((rc = c->d_vmaps.ensure((size_t)sg.nseg * 64 * NC)) || (rc = c->d_vend.ensure((size_t)sg.nseg)))
        return rc;
    BHMM_HIP(launch(k_wide_vit_walk<false, uint8_t, NC>, dim3(sg.nseg), dim3(64), 0, c->stream, off, sg, n, v.ptr,
                    c->d_vmaps.p, nullptr, nullptr));
    BHMM_HIP(launch(k_wide_vit_stitch, dim3((K + 63) / 64), dim3(64), 0, c->stream, traj0, K, c->d_vmaps.p, 64 * NC, v.last,
                    c->d_vend.p));
    BHMM_HIP(v.out([&](auto *p) {
        return launch(k_wide_vit_walk<true, std::remove_pointer_t<decltype(p)>, NC>, dim3(sg.nseg), dim3(64), 0, c->stream,
                      off, sg, n, v.ptr, nullptr, c->d_vend.p, p);
    }));
    return BHMM_OK;
}

// boundary vectors of `width` doubles per segment, the checkpoints of the fix-up rounds and the flags
// ([nseg] flagged | [nseg] flagged and further than SEG_VIT_TOL)
inline int vit_boundary_bufs(bhmm_ctx *c, const Segs &sg, int width)
{
    int rc;
    if ((rc = c->d_aentry.ensure((size_t)sg.nseg * width)) || (rc = c->d_aexit.ensure((size_t)sg.nseg * width)) ||
        (rc = c->d_vckpt.ensure(((size_t)(c->total >> 6) + 1) * width)) || (rc = c->d_vflag.ensure(2 * (size_t)sg.nseg)))
        return rc;
    return BHMM_OK;
}

// The path-margin acceptance keeps every vector of the first pass ([total][n], in the buffer of the 65..128-state
// E-step's W rows): that buffer where the rule is wanted and memory allows, else nullptr (the rounds alone decide)
inline double *vit_vall(bhmm_ctx *c, bool wanted)
{
    c->last.vit_margin_used = 0;
    c->last.vit_margin_close = 0;
    if (wanted && c->d_gW.ensure((size_t)c->total * c->n) == BHMM_OK)
        return c->d_gW.p;
    (void)hipGetLastError();
    return nullptr;
}

// After seg_viterbi accepted a pass at W_try: where the next call on these observations starts -- longer, up to
// W_cap, if far boundaries kept the margin rule from being asked (or could not be mended) or after three rounds
inline void vit_accepted(bhmm_ctx *c, const SegVitResult &r, const double *vall, int W_try, int W_cap)
{
    const bool longer = !r.margin_accepted && ((vall && c->last.vit_far > 0) || r.rounds >= 3);
    c->ds.vit.W = plan::vit_next_warmup(W_try, longer, W_cap);
}
// After the attempts of a pass with fix-up rounds: not accepted -- these observations go to the serial kernel from now on
inline void vit_attempts_done(bhmm_ctx *c, bool done)
{
    if (!done && c->ds.pplan[0].nseg > c->K)
        c->ds.vit.seg_given_up = true;
    c->last.viterbi_chunked = done;
}

} // namespace bhmm
