// plan.hpp -- host-side planning of the time decomposition: chunk tables of the N <= 8 family
// (bhmm_amd.hip), segment tables of the 9..64-state family (wide_api.hip), the plan of a forward-only pass
// (bhmm_score, bhmm_filter: plan_pass, uploaded by seg_host.hpp), the ranges of a budgeted workspace of the posterior
// calls (smooth_ranges, smooth_tile_ranges), and the forgetting probe every family
// warms up by: where it samples (probe_starts) and how its curve is read (curve_last, warmup_of,
// warmup_wide_of), the acceptance protocol of a verified pass (two_attempts, doubled), and the integer rules of the
// segment-parallel backward draw (draw_seglen, draw_next_warmup) and of the Viterbi passes (vit_*).  Pure C++ (no HIP), so
// the same code runs under -fsanitize=address,undefined in the CPU sanitizer build
// (oracle/Makefile `asan`); the .hip files only allocate and upload what these functions return.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace bhmm {
namespace plan {

struct ChunkPlan {
    int L = 0, Lmax = 1, G = 0, Gp = 0, chunk_mult = 1;
    std::vector<int32_t> ctraj, clen, traj_c0; // [Gp], [Gp], [K+1]
    std::vector<int64_t> ct0, cgoff;           // [Gp], [Gp]
    // two-level stitch: groups of R consecutive chunks (empty when every trajectory is short)
    int nG = 0;
    std::vector<int32_t> g0, g1, gt; // [nG], [nG], [K+1]
};

// Every trajectory is cut into ceil(T/L) chunks whose lengths differ by at most one.
//   offsets[K+1]  trajectory offsets in time steps;  N  padded state count (2, 4, 8)
//   chunk         chunk length, or <= 0 for the automatic plan
//   allow_mult    automatic plan may take two / three times the default chunk count
//   block         chunks per workgroup (the tables are padded to a multiple of it)
//   half          automatic plan with half the default chunk count (see default_chunk_count)
// Returns false if the plan would exceed 2^30 chunks.
inline int64_t default_chunk_count(int N) { return 32768 * 4 / std::max(1, N / 2); } // N/2 lanes per chunk
inline bool plan_chunks(const std::vector<int64_t> &offsets, int K, int N, int64_t total, int chunk,
                        bool allow_mult, int block, ChunkPlan &p, bool half = false)
{
    p = ChunkPlan();
    int L = chunk;
    if (L <= 0) {
        // k_estep uses N/2 lanes per chunk: 32768 chunks (N = 8) put two 64-lane wavefronts on every
        // SIMD of the 256 CUs.  Fewer, longer chunks amortise the warm-up of the speculative
        // boundaries (W / L extra steps); more chunks only help occupancy (measured optimum on
        // configs[1]: profiles/r01).
        // `half`: 16384 chunks -- ONE wavefront per SIMD in the backward sweep, which issues at 0.85-0.9
        // of the rate of two.  The better plan when the default one's chunks come out shorter than
        // about 1.6 warm-ups (a batch of a few million steps): each chunk's two warm-ups then cost
        // more than the lost occupancy (tools/chunk_scan.py; the host re-plans once the warm-up of
        // the model has been measured, bhmm_amd.hip: replan_for_warmup)
        const int64_t target = default_chunk_count(N) / (half ? 2 : 1);
        int64_t l = (total + target - 1) / target;
        // Very long chunks: two or three times as many.  The sweeps without xi accumulators (P1,
        // the forward-only pass) then have four to six long wavefronts per SIMD instead of two
        // (configs[2], 1024 x 1e6: P1 7.2 -> 5.9 ms, E-step 20.2 -> 18.7 ms), while the warm-up
        // stays below a few per cent of the chunk even if it calibrates to four times the default.
        if (l >= 3 * 9216 && allow_mult) {
            l = (l + 2) / 3;
            p.chunk_mult = 3;
        } else if (l >= 2 * 9216 && allow_mult) {
            l = (l + 1) / 2;
            p.chunk_mult = 2;
        }
        L = (int)std::min<int64_t>(std::max<int64_t>(l, 32), (int64_t)1 << 20);
    }
    p.L = L;
    p.traj_c0.assign(K + 1, 0);
    for (int k = 0; k < K; ++k) {
        const int64_t T = offsets[k + 1] - offsets[k];
        p.traj_c0[k] = (int32_t)p.ctraj.size();
        if (T <= 0)
            continue;
        const int64_t nck = (T + L - 1) / L;
        const int64_t base = T / nck, rem = T % nck;
        if ((int64_t)p.ctraj.size() + nck > (int64_t)1 << 30)
            return false;
        for (int64_t q = 0; q < nck; ++q) {
            const int64_t len = base + (q < rem ? 1 : 0);
            const int64_t t0 = q * base + std::min(q, rem);
            p.ctraj.push_back(k);
            p.clen.push_back((int32_t)len);
            p.ct0.push_back(t0);
            p.cgoff.push_back(offsets[k] + t0);
            p.Lmax = std::max<int>(p.Lmax, (int)len);
        }
    }
    p.traj_c0[K] = (int32_t)p.ctraj.size();
    p.G = (int)p.ctraj.size();
    p.Gp = std::max(block, (p.G + block - 1) / block * block);
    p.ctraj.resize(p.Gp, 0);
    p.clen.resize(p.Gp, 0);
    p.ct0.resize(p.Gp, 1);
    p.cgoff.resize(p.Gp, 0);
    // two-level stitch: groups of R consecutive chunks; serial depth 2R + n/R instead of n
    int nmax = 0;
    for (int k = 0; k < K; ++k)
        nmax = std::max(nmax, p.traj_c0[k + 1] - p.traj_c0[k]);
    if (nmax > 48) {
        const int R = std::max(4, std::min(256, (int)lround(sqrt(0.5 * nmax))));
        p.gt.assign(K + 1, 0);
        for (int k = 0; k < K; ++k) {
            p.gt[k] = (int32_t)p.g0.size();
            for (int cc = p.traj_c0[k]; cc < p.traj_c0[k + 1]; cc += R) {
                p.g0.push_back(cc);
                p.g1.push_back(std::min(cc + R, p.traj_c0[k + 1]));
            }
        }
        p.gt[K] = (int32_t)p.g0.size();
        p.nG = (int)p.g0.size();
    }
    return true;
}

struct SegPlan {
    std::vector<int32_t> traj, len, traj0; // [ns], [ns], [K+1]
    std::vector<int64_t> t0;               // [ns]
};

// Segments of at most seglen steps (seglen <= 0: one per trajectory), `mult` times as many;
// boundaries at multiples of four (the lazily scaled kernels rescale on t % 4 == 3).
inline void plan_segments(const std::vector<int64_t> &offsets, int K, int64_t seglen, int mult,
                          SegPlan &s)
{
    s = SegPlan();
    s.traj0.assign(K + 1, 0);
    for (int k = 0; k < K; ++k) {
        s.traj0[k] = (int32_t)s.traj.size();
        const int64_t T = offsets[k + 1] - offsets[k];
        if (T <= 0)
            continue;
        const int64_t ns = (seglen > 0 ? (T + seglen - 1) / seglen : 1) * mult;
        int64_t prev = 0;
        for (int64_t q = 1; q <= ns; ++q) {
            const int64_t b = q == ns ? T : ((q * T) / ns) & ~(int64_t)3;
            if (b <= prev)
                continue;
            s.traj.push_back(k);
            s.len.push_back((int32_t)(b - prev));
            s.t0.push_back(prev);
            prev = b;
        }
    }
    s.traj0[K] = (int32_t)s.traj.size();
}

// Segment length of the scoring plan for 9..64 states (score_api.hip: plan_pass with it; bhmm_filter's too).  A
// function of the observation set's size, the lane-group width np (16, 32, 64) and the device only: a score
// must not depend on what earlier calls found out.  asked > 0: the caller's length (option score_seglen).
// Automatic: two wavefronts per SIMD for ONE model (the kernel's registers allow two at np = 64; more models
// bring their own wavefronts), but at least 2048 steps, against which a warm-up of a few hundred is small.
inline int64_t score_seglen(int64_t total, int np, int num_simd, int64_t asked)
{
    if (asked > 0)
        return (asked + 3) & ~(int64_t)3;
    const int64_t want = 2 * (int64_t)num_simd * (64 / np);
    return (std::max<int64_t>((total + want - 1) / want, 2048) + 3) & ~(int64_t)3;
}

// Segment length of the scoring plan for 65..128 states (score_api.hip: plan_pass with it and tiles; bhmm_filter's
// too).  A function of the observation set's size and the device only, like score_seglen.  asked > 0: the
// caller's length (option score_seglen).  Automatic: enough tiles of 16 segments for one workgroup per compute
// unit for ONE model (num_simd / 4 tiles; more models bring their own workgroups), but at least 256 steps: a
// quickly mixing model forgets its start within some tens of steps, and a segment of four times that keeps the
// warm-up, which is paid per segment, a minor share of the steps.
constexpr int64_t SCORE_TILE_MIN_SEGLEN = 256;
inline int64_t score_tile_seglen(int64_t total, int num_simd, int64_t asked)
{
    if (asked > 0)
        return (asked + 3) & ~(int64_t)3;
    const int64_t want = 16 * std::max<int64_t>(num_simd / 4, 1);
    return (std::max<int64_t>((total + want - 1) / want, SCORE_TILE_MIN_SEGLEN) + 3) & ~(int64_t)3;
}

// Tiles of the row-batched kernels (tile_kernels.hpp): 16 segments per workgroup, which runs as long
// as its longest row and takes its fast paths where all 16 rows are in the same phase -- so segments
// without a warm-up in the direction of the pass (backward = false: those that start a trajectory;
// backward = true: those that end one) get tiles of their own, and inside each class the segments are
// sorted by length (stable, longest first).  Empty slots: -1.
inline void plan_tiles(const SegPlan &s, const std::vector<int64_t> &offsets, bool backward,
                       std::vector<int32_t> &tile_seg)
{
    tile_seg.clear();
    for (int cls = 0; cls < 2; ++cls) {
        std::vector<int32_t> order;
        for (size_t i = 0; i < s.len.size(); ++i) {
            if (s.len[i] <= 0)
                continue;
            const int64_t T = offsets[s.traj[i] + 1] - offsets[s.traj[i]];
            const bool edge = backward ? s.t0[i] + s.len[i] >= T : s.t0[i] == 0;
            if ((edge ? 0 : 1) == cls)
                order.push_back((int32_t)i);
        }
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return s.len[a] > s.len[b]; });
        const size_t base = tile_seg.size();
        tile_seg.resize(base + (order.size() + 15) / 16 * 16, -1);
        std::copy(order.begin(), order.end(), tile_seg.begin() + base);
    }
}

// The plan of a forward-only pass over segments of at most seglen steps (bhmm_score and bhmm_filter at 9..128
// states; seg_host.hpp uploads it): plan_segments with mult 1, with `tiles` the tile table of the forward
// direction, and the number of trajectories with at least one step (as many segments: no boundary).
struct PassPlan {
    SegPlan seg;
    std::vector<int32_t> tile_seg; // [16 * tiles], empty without `tiles`
    int ntraj = 0;
};
inline void plan_pass(const std::vector<int64_t> &offsets, int K, int64_t seglen, bool tiles, PassPlan &p)
{
    plan_segments(offsets, K, seglen, 1, p.seg);
    p.tile_seg.clear();
    if (tiles)
        plan_tiles(p.seg, offsets, false, p.tile_seg);
    p.ntraj = 0;
    for (int k = 0; k < K; ++k)
        p.ntraj += offsets[k + 1] > offsets[k];
}

// ---- ranges of segments for a budgeted workspace (the posterior calls at 9..64 states, smooth_wide.hip) ----
// The filtered rows of a segment live in a workspace of `row_bytes` per step between the forward and the backward
// launch.  smooth_ranges cuts the plan's segments (lengths `len`, in plan order) into ranges [s0, s1) of consecutive
// whole segments whose steps fit `budget` bytes (0: unbounded, one range).  A range starts at a multiple of `group`
// (the segments of one wavefront, 64 / np) and holds whole groups -- so the workgroups of a range are those of the
// whole launch -- and at least one, however small the budget; only the last range may end on a partial group.
struct SegRange {
    int s0 = 0, s1 = 0;
    int64_t steps = 0;
};
inline void smooth_ranges(const std::vector<int32_t> &len, int group, int64_t row_bytes, int64_t budget,
                          std::vector<SegRange> &out)
{
    out.clear();
    const int nseg = (int)len.size();
    int s = 0;
    while (s < nseg) {
        SegRange r;
        r.s0 = s;
        while (s < nseg) {
            const int e = std::min(nseg, s + group);
            int64_t add = 0;
            for (int q = s; q < e; ++q)
                add += len[q];
            if (budget > 0 && s > r.s0 && (r.steps + add) * row_bytes > budget)
                break;
            r.steps += add;
            s = e;
        }
        r.s1 = s;
        out.push_back(r);
    }
}

// ---- the same at 65..128 states (smooth_tile.hip): ranges with tile tables of their own ----
// A tile's sixteen segments are picked by length, not by position, and the forward and the backward tile tables
// differ (plan_tiles puts different segments in the edge class), so the cut comes first: smooth_ranges with group 1
// over the plan's segments in plan order (consecutive global steps), whole segments that fit `budget` bytes, at least
// one per range.  Then every range gets a forward and a backward tile table over its segments alone (plan_tiles on
// the range's sub-plan).  The tables are concatenated in tile_f / tile_b and name segments of the WHOLE plan; a
// range's tiles are [f0, f0 + nf) and [b0, b0 + nb).  Budget 0 or one that fits: one range, the whole plan.
struct TileRange {
    int s0 = 0, s1 = 0;
    int64_t steps = 0;
    int f0 = 0, nf = 0, b0 = 0, nb = 0;
};
inline void smooth_tile_ranges(const SegPlan &s, const std::vector<int64_t> &offsets, int64_t row_bytes, int64_t budget,
                               std::vector<TileRange> &out, std::vector<int32_t> &tile_f, std::vector<int32_t> &tile_b)
{
    out.clear();
    tile_f.clear();
    tile_b.clear();
    std::vector<SegRange> cut;
    smooth_ranges(s.len, 1, row_bytes, budget, cut);
    for (const SegRange &r : cut) {
        SegPlan sub;
        sub.traj.assign(s.traj.begin() + r.s0, s.traj.begin() + r.s1);
        sub.len.assign(s.len.begin() + r.s0, s.len.begin() + r.s1);
        sub.t0.assign(s.t0.begin() + r.s0, s.t0.begin() + r.s1);
        TileRange t;
        t.s0 = r.s0;
        t.s1 = r.s1;
        t.steps = r.steps;
        std::vector<int32_t> tiles;
        for (int dir = 0; dir < 2; ++dir) {
            std::vector<int32_t> &all = dir ? tile_b : tile_f;
            plan_tiles(sub, offsets, dir != 0, tiles);
            for (int32_t &e : tiles)
                e = e < 0 ? -1 : e + r.s0;
            (dir ? t.b0 : t.f0) = (int)(all.size() / 16);
            (dir ? t.nb : t.nf) = (int)(tiles.size() / 16);
            all.insert(all.end(), tiles.begin(), tiles.end());
        }
        out.push_back(t);
    }
}

// ---- the forgetting probe (k_forget_probe up to 8 states, k_wide_probe at 9..64) ----
// It runs two differently started chains over Wmax steps from P sample positions and leaves, per direction and
// step, the largest deviation between them: curve[w] forward, curve[Wmax + w] backward.

// Longest warm-up the probe measures: half the longest trajectory, at most 1024 steps in multiples of 4 (up to 8
// states) or 8192 in multiples of 8 (9..64 states).  0: the trajectories are too short to probe.
inline int probe_wmax(int64_t maxT)
{
    const int Wmax = (int)std::min<int64_t>(1024, maxT / 2) / 4 * 4;
    return Wmax < 32 ? 0 : Wmax;
}
inline int probe_wmax_wide(int64_t maxT)
{
    const int Wmax = (int)std::min<int64_t>(8192, maxT / 2) / 8 * 8;
    return Wmax < 64 ? 0 : Wmax; // (trajectories of fewer than 128 steps)
}

// The P sample positions (in time steps, like the offsets): the trajectories of at least Wmax steps in turn, each
// visited `reps` times at starts spread evenly over the room that leaves Wmax steps to its end.  Wmax from
// probe_wmax / probe_wmax_wide, not 0: at least one trajectory is that long.
inline void probe_starts(const std::vector<int64_t> &offsets, int K, int Wmax, int P, std::vector<int64_t> &starts)
{
    std::vector<int> longk;
    for (int k = 0; k < K; ++k)
        if (offsets[k + 1] - offsets[k] >= Wmax)
            longk.push_back(k);
    starts.resize(P);
    for (int i = 0; i < P; ++i) {
        const int k = longk[i % longk.size()];
        const int64_t room = offsets[k + 1] - offsets[k] - Wmax + 1;
        const int64_t rep = i / (int64_t)longk.size(), reps = (P + longk.size() - 1) / longk.size();
        starts[i] = offsets[k] + (room - 1) * rep / std::max<int64_t>(reps - 1, 1);
    }
}

// The last step at which the chains are still `target` apart (-1: never), in the forward direction or in the
// worse of the two.
inline int curve_last(const float *curve, int Wmax, float target, bool both)
{
    int last = -1;
    for (int w = 0; w < Wmax; ++w)
        if (curve[w] >= target || (both && curve[Wmax + w] >= target))
            last = w;
    return last;
}

// Warm-up from that reading, last + 2 steps to get below the target and stay there.  Up to 8 states: + 15 %, a
// multiple of 4, at least 16, at most Wmax.  9..64 states: times PROBE_WIDE_MARGIN -- the check looks at every
// boundary, the probe at P positions, and the worst boundary lags the worst sample (measured: 1.3 x in warm-up
// steps) --, a multiple of 8, at least 16; what a reading near Wmax means is the caller's decision.
constexpr double PROBE_WIDE_MARGIN = 1.5;
inline int warmup_of(int last, int Wmax)
{
    const int w = (int)std::ceil(1.15 * (last + 2));
    return std::min(std::max(16, (w + 3) / 4 * 4), Wmax);
}
inline int warmup_wide_of(int last)
{
    const int w = (int)std::ceil(PROBE_WIDE_MARGIN * (last + 2));
    return std::max(16, (w + 7) / 8 * 8);
}

// ---- the acceptance protocol of a verified pass (bhmm_filter, bhmm_posterior_decode, bhmm_posterior_marginals) ----
// `pass(W, &v)` runs the kernels at warm-up W and returns a BHMM code (non-zero: returned at once); v says what its
// boundary check found.  verified: the results stand (*verified).  failed: the call counts one fallback -- once,
// after the first pass -- and runs once more at doubled(W, Wcap); failed again: *verified stays false and the
// caller takes its last-resort path.  abandon (a segment outside the kernels' number range): the same ending at
// once, and nothing is counted.  bhmm_score runs the protocol per model of a batch (score_api.hip: retry_failed)
// and takes only the doubling from here.
//
// What the callers do NOT share is how they round the W they start from; unifying it would change results:
//   up to 8 states (filter, decode, marginals; score)  the option or the probe's reading as it is; cap 1 << 30
//   9..64 states, filter                 (filter_W + 7) / 8 * 8 (not clamped before rounding), then max(W, 8); 1 << 30
//   9..64 states, decode / marginals     smooth_W rounded up to 8 in 64 bits and clamped to 1 << 30, then max(W, 8);
//                                        1 << 30; may abandon
//   9..64 states, score                  (score_W + 3) & ~3 per model; 1 << 30
//   65..128 states, filter / score       (W + 3) & ~3, or 0 for a plan without a boundary; cap SCORE_TILE_W_MAX
//   65..128 states, decode / marginals   the same, clamped to SCORE_TILE_W_MAX before the pass; may abandon
constexpr int SCORE_TILE_W_MAX = 1 << 20; // longest warm-up of the matrix-core passes at 65..128 states
enum class Verdict { verified, failed, abandon };
inline Verdict verdict_of(unsigned int fails) { return fails == 0 ? Verdict::verified : Verdict::failed; } // of a count
inline int doubled(int W, int64_t cap) { return (int)std::min<int64_t>(2 * (int64_t)W, cap); }
template <class Pass>
int two_attempts(int W, int Wcap, int *fallbacks, Pass pass, bool *verified)
{
    *verified = false;
    for (int attempt = 0; attempt < 2; ++attempt) {
        Verdict v = Verdict::failed;
        if (const int rc = pass(W, &v))
            return rc;
        if (v != Verdict::failed) {
            *verified = v == Verdict::verified;
            return 0; // (BHMM_OK)
        }
        if (attempt == 0)
            ++*fallbacks; // boundaries that did not verify at the first warm-up
        W = doubled(W, Wcap);
    }
    return 0;
}

// ---- the integer rules of the segment-parallel backward draw (path_api.hip: seg_draw) ----
// Every warm-up is exact (segments that did not continue their successor's state are drawn again), so these only
// trade warm-up steps against fix-up rounds.  Segment length: `want` (>= 1) segments over the observation set's
// `total` steps, none shorter than DRAW_SEGLEN_MIN.  Warm-up: DRAW_W_START on new observations; the next call's
// is twice as long while the first round left more than a tenth of the `nseg` segments to the fix-up, up to
// DRAW_W_MAX.  DRAW_MAX_ROUNDS fix-up rounds, then the serial kernel.
constexpr int64_t DRAW_SEGLEN_MIN = 64;
constexpr int DRAW_W_START = 64;
constexpr int DRAW_W_MAX = 4096;
constexpr int DRAW_MAX_ROUNDS = 16;
inline int64_t draw_seglen(int64_t total, int64_t want) { return std::max((total + want - 1) / want, DRAW_SEGLEN_MIN); }
inline int draw_next_warmup(int W, int64_t mismatch, int64_t nseg) { return mismatch * 10 > nseg && W < DRAW_W_MAX ? 2 * W : W; }

// ---- the integer rules of the Viterbi passes (path_api.hip, gen_api.hip, viterbi_host.hpp) ----
// Every accepted path is the serial kernel's, so these only trade warm-up steps against fix-up rounds and lost
// passes.  W0: the E-step's warm-up as the segment passes take it, a multiple of 8 and at least 64 (128 unprobed).
inline int vit_w_estep(int spec_W) { return std::max(64, spec_W > 0 ? (spec_W + 7) / 8 * 8 : 128); }
// steps per segment that give `want` (>= 1) segments over `total` steps; ... rounded up to a multiple of 8
inline int64_t vit_fill(int64_t total, int64_t want) { return (total + want - 1) / want; }
inline int64_t vit_fill8(int64_t total, int64_t want) { return (vit_fill(total, want) + 7) / 8 * 8; }
// 9..64 states: per_simd lane groups of np lanes (16, 32, 64) per SIMD, no segment shorter than `warmups` warm-ups
inline int64_t vit_wide_seglen(int64_t total, int np, int num_simd, int per_simd, int warmups, int W)
{
    return std::max<int64_t>(vit_fill(total, (int64_t)per_simd * num_simd * (64 / np)), warmups * (int64_t)W);
}
// 65..128 states: per_simd segments per SIMD (with the margin rule on, `warmups` is one: segments as short as a warm-up)
inline int64_t vit_gen_fill(int64_t total, int num_simd, int per_simd) { return vit_fill8(total, (int64_t)per_simd * num_simd); }
inline int64_t vit_gen_seglen(int64_t total, int num_simd, int per_simd, int warmups, int W)
{
    return std::max<int64_t>(vit_fill(total, (int64_t)per_simd * num_simd), warmups * (int64_t)W);
}
// 129..256 states: VIT_ROWS segments per workgroup, one workgroup per compute unit; a multiple of 8
constexpr int VIT_ROWS = 4;
inline int64_t vit_rows_fill(int64_t total, int num_simd) { return vit_fill8(total, (int64_t)VIT_ROWS * (num_simd / 4)); }
inline int64_t vit_rows_seglen(int64_t fill0, int W) { return std::max<int64_t>(fill0, W); }
// 9..64 states start at 128 steps, less if the filter forgets faster (vit_W: what the last call left, 0: none)
inline int vit_wide_w_start(int vit_W, int W0) { return vit_W > 0 ? vit_W : std::min(128, W0); }
// 65..128 states: the survivors of these larger models meet later than the filter forgets -- up to four times the
// E-step's length, but never longer than the segments that fill the chip (fill0 = vit_gen_fill).  With the mending
// round the E-step's length is where a new set of observations starts, without it the cap.
inline int vit_gen_w_cap(int W0, int64_t fill0) { return (int)std::max<int64_t>(W0, std::min<int64_t>(4 * (int64_t)W0, fill0)); }
inline int vit_gen_w_start(int vit_W, int W0, int W_cap, bool margin, bool mend)
{
    return vit_W > 0 ? vit_W : ((margin && !mend) ? W_cap : W0);
}
// 129..256 states: with the mending round the E-step's length, else six of them, at most one and a half fill
// lengths (fill0 = vit_rows_fill)
inline int vit_rows_w_start(int vit_W, int W0, int64_t fill0, bool mend)
{
    if (vit_W > 0)
        return vit_W;
    return mend ? W0 : (int)std::max<int64_t>(W0, std::min<int64_t>(6 * (int64_t)W0, (3 * fill0 / 2 + 7) / 8 * 8));
}
// ... a pass that was not accepted, the `fails`-th in a row: given up after the second, or when twice the warm-up
// would exceed half the longest trajectory; else the next call tries 2 W
inline bool vit_rows_give_up(int fails, int W, int64_t maxT) { return fails >= 2 || 4 * (int64_t)W > maxT; }
// 9..128 states, the next call's warm-up after an accepted pass (longer: far boundaries kept the margin rule from
// being asked, or three or more rounds)
inline int vit_next_warmup(int W, bool longer, int cap) { return (longer && W < cap) ? std::min(2 * W, cap) : W; }

// 8 states and fewer, the warm-up of the chunk-parallel run.  The first call on new observations starts from the
// E-step's length (spec_W); every later call that verified tries three quarters of the last good length (vit_W),
// rounded to 8 and at least 32, while that is below vit_W and above a length that failed before (vit_bad) -- until
// one does not verify: that attempt is repeated with the last good length in the same call and the search ends (at
// most one lost pass per set of observations).  An attempt out of tolerance otherwise doubles the warm-up; three
// attempts, then the serial kernel.  `attempt(W, first, &v)` runs the kernels and returns a BHMM code (non-zero:
// returned at once); *last is the verdict of the last attempt.
struct ChunkVerdict {
    bool accepted = false; // every boundary bit-identical, or all within tolerance and no close decision
    bool within = false;   // every boundary within tolerance
};
inline int vit_chunk_w_first(int vit_W, int vit_bad, bool &vit_explore, int spec_W, bool W_fixed, bool *exploring)
{
    *exploring = false;
    if (vit_W > 0 && vit_explore && !W_fixed) {
        const int Wn = std::max(32, (vit_W * 3 / 4 + 7) / 8 * 8);
        if (Wn < vit_W && Wn > vit_bad) {
            *exploring = true;
            return Wn;
        }
        vit_explore = false;
    }
    return vit_W > 0 ? vit_W : spec_W;
}
template <class Attempt>
int vit_chunk_attempts(int &vit_W, int &vit_bad, bool &vit_explore, int spec_W, bool W_fixed, Attempt attempt,
                       ChunkVerdict *last)
{
    bool exploring;
    int W = vit_chunk_w_first(vit_W, vit_bad, vit_explore, spec_W, W_fixed, &exploring);
    for (int a = 0; a < 3; ++a) {
        if (a > 0 && exploring) { // the shorter warm-up did not verify: back to the one that did
            vit_bad = W;
            vit_explore = exploring = false;
            W = vit_W;
        } else if (a > 0) {
            W *= 2;
        }
        if (const int rc = attempt(W, a == 0, last))
            return rc;
        if (exploring && !last->accepted)
            continue; // (a shorter warm-up must be as good as the longer one was, not merely tolerable)
        if (last->within) {
            vit_W = W; // (what worked is where the next call on these observations starts)
            break;     // every boundary within tolerance: a longer warm-up changes nothing
        }
    }
    return 0;
}

// For every segment of the plan with `seglen`: the start of a segment of the twice-as-fine plan
// strictly inside it (-1: none).  Cuts the trajectories exactly like plan_segments(.., 1).
inline void plan_forward_mids(const std::vector<int64_t> &offsets, int K, int64_t seglen,
                              std::vector<int64_t> &mid)
{
    mid.clear();
    for (int k = 0; k < K; ++k) {
        const int64_t T = offsets[k + 1] - offsets[k];
        if (T <= 0)
            continue;
        const int64_t ns = (T + seglen - 1) / seglen;
        int64_t prev = 0;
        for (int64_t q = 1; q <= ns; ++q) {
            const int64_t b = q == ns ? T : ((q * T) / ns) & ~(int64_t)3;
            if (b <= prev)
                continue;
            const int64_t m2 = (((2 * q - 1) * T) / (2 * ns)) & ~(int64_t)3;
            mid.push_back(m2 > prev && m2 < b ? m2 : -1);
            prev = b;
        }
    }
}

} // namespace plan
} // namespace bhmm
