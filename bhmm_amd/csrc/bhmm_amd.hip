// bhmm_amd.hip -- C ABI (include/bhmm_amd.h) over the gfx950 kernels: context management,
// chunk planning, launches.  Host code only orchestrates; all arithmetic on trajectories is
// in estep_kernels.hpp / path_kernels.hpp.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "host_internal.hpp"
#include "plan.hpp"
#include "runs_host.hpp"
#include "seg_host.hpp"
#include "estep_sweep.hpp"

namespace bhmm {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int hip_fail(hipError_t e, const char *what)
{
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? BHMM_ERR_NO_MEM : BHMM_ERR_HIP;
}

int invalid_arg(const std::string &msg)
{
    g_err = msg;
    return BHMM_ERR_INVALID;
}

Chunks chunks_of(const bhmm_ctx *c)
{
    Chunks ch;
    ch.traj = c->d_ctraj.p;
    ch.t0 = c->d_ct0.p;
    ch.len = c->d_clen.p;
    ch.goff = c->d_cgoff.p;
    ch.Lmax = c->Lmax;
    return ch;
}

int64_t longest_traj(const bhmm_ctx *c)
{
    int64_t maxT = 0;
    for (int k = 0; k < c->K; ++k)
        maxT = std::max(maxT, c->offsets[k + 1] - c->offsets[k]);
    return maxT;
}

int ensure_specres(bhmm_ctx *c, size_t words)
{
    if (int rc = c->d_specres.ensure(words))
        return rc;
    if (!c->h_specres)
        BHMM_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_specres), 4 * sizeof(unsigned int), hipHostMallocDefault));
    return BHMM_OK;
}

int specres_reset(bhmm_ctx *c, int words)
{
    BHMM_HIP(hipMemsetAsync(c->d_specres.p, 0, words * sizeof(unsigned int), c->stream));
    return BHMM_OK;
}

int specres_read(bhmm_ctx *c, int words, bool wait)
{
    BHMM_HIP(hipMemcpyAsync(c->h_specres, c->d_specres.p, words * sizeof(unsigned int), hipMemcpyDeviceToHost,
                            c->stream));
    if (wait)
        BHMM_HIP(hipStreamSynchronize(c->stream));
    return BHMM_OK;
}

template <int N, int KIND>
static size_t smem_fwdbwd(int M, int dcopies = 1)
{
    // [wavefronts per workgroup][S] reduction scratch + (discrete) B^T and the count table +
    // the gather exchange area of k_estep (one 16-byte slot per thread)
    return (size_t)(((N / 2 * 64 + 63) / 64) * StatLayout<N, KIND>::S +
                    (KIND == EMIT_DISC ? (1 + dcopies) * M * N : 0) + 2 * 32 * N) *
           sizeof(double);
}

// discrete count tables per workgroup: one per wavefront if that fits the LDS, else one
template <int N>
static int disc_copies(int M)
{
    const int NW = (N / 2 * 64 + 63) / 64;
    return smem_fwdbwd<N, EMIT_DISC>(M, NW) <= 150 * 1024 ? NW : 1;
}

static int stats_size(const bhmm_ctx *c);
// symbols whose tables live in the LDS of the sweep kernels: all of them, or none (big alphabets)
static int lds_symbols(const bhmm_ctx *c) { return c->bt_global ? 0 : c->M; }
static int64_t ci_records(const bhmm_ctx *c) { return (int64_t)(c->Gp / 64) * c->Lmax; }
// the unconditional refills of the sweeps (estep_sweep.hpp) stay inside the guards of the buffers they read
static_assert(SWEEP_REACH_BACK <= (int)bhmm_ctx::SWEEP_GUARD_BACK && SWEEP_REACH_FRONT <= (int)bhmm_ctx::SWEEP_GUARD_FRONT,
              "a deeper prefetch needs wider guards around d_obs_ci, d_obs16, d_ws and d_ea (ctx.hpp)");
// ... and the loops on the 16-bit copy move in whole blocks of OBS16_BLK steps: two blocks behind a chunk's last
// record (forward), two before its first (backward quads)
static_assert(SWEEP_REACH_BACK % OBS16_BLK == 0 && SWEEP_REACH_FRONT % OBS16_BLK == 0 && SWEEP_REACH_BACK >= 2 * OBS16_BLK &&
                  SWEEP_REACH_FRONT >= 2 * OBS16_BLK,
              "the guards of d_obs16 are whole blocks and cover two of them on either side");

int replan_coarse(bhmm_ctx *c, bool half = false, int chunk = 0); // (defined with bhmm_ctx_set_observations)
int replan_for_warmup(bhmm_ctx *c);

#ifndef ESTEP_SPLIT
#define ESTEP_SPLIT 1 // statistics-only speculative E-step in two launches (PH_P1, PH_P2)
#endif

// componentwise relative tolerance of the boundary check (k_spec_check / k_tail)
// boundary tolerance of the time-split E-step, N <= 8: the context's spec_tol (option, default 1e-11)
#define SPEC_TOL (c->opt.spec_tol)

// One E-step launch sequence for a fixed padded N.
template <int N>
struct Runner {
    template <int KIND>
    static int prescan_stitch(bhmm_ctx *c, const Model<N> &m)
    {
        const Chunks ch = chunks_of(c);
        const size_t sm0 = (size_t)(N * N + 64 * N + (KIND == EMIT_DISC ? lds_symbols(c) * N : 0)) *
                           sizeof(double);
        BHMM_HIP(hipEventRecord(c->ev[0], c->stream));
        BHMM_HIP(launch(k_prescan<N, KIND>, dim3(c->Gp / 64), dim3(64 * N), sm0, c->stream, m, ch, c->d_obs_ci.p,
                        c->d_Bt.p, c->d_M.p));
        BHMM_HIP(hipEventRecord(c->ev[1], c->stream));
        const int gp = 64 / N;
        if (c->nG == 0) {
            // one level: every trajectory stitched serially over its chunks
            const int nb = (c->K + gp - 1) / gp;
            BHMM_HIP(launch(k_stitch<N>, dim3(2 * nb), dim3(64), 0, c->stream, c->d_traj_c0.p, c->d_traj_c0.p + 1, c->K,
                            nb, c->n, c->d_M.p, nullptr, nullptr, c->d_aentry.p, c->d_bexit.p));
        } else {
            // two levels: group products, stitch over groups, stitch inside all groups
            const int ngb = (c->nG + gp - 1) / gp;
            BHMM_HIP(launch(k_compose<N>, dim3(ngb), dim3(64), 0, c->stream, c->d_grp_c0.p, c->d_grp_c1.p, c->nG,
                            c->d_M.p, c->d_P.p));
            const int nb = (c->K + gp - 1) / gp;
            BHMM_HIP(launch(k_stitch<N>, dim3(2 * nb), dim3(64), 0, c->stream, c->d_grp_traj0.p, c->d_grp_traj0.p + 1,
                            c->K, nb, c->n, c->d_P.p, nullptr, nullptr, c->d_agrp.p, c->d_bgrp.p));
            BHMM_HIP(launch(k_stitch<N>, dim3(2 * ngb), dim3(64), 0, c->stream, c->d_grp_c0.p, c->d_grp_c1.p, c->nG, ngb,
                            c->n, c->d_M.p, c->d_agrp.p, c->d_bgrp.p, c->d_aentry.p, c->d_bexit.p));
        }
        BHMM_HIP(hipEventRecord(c->ev[2], c->stream));
        return BHMM_OK;
    }

    template <int KIND, int MODE, bool SPEC = false>
    static int fwdbwd(bhmm_ctx *c, const Model<N> &m, bool store_gamma,
                      unsigned int *flag_words = nullptr)
    {
        if (!flag_words)
            flag_words = c->d_specres.p;
        const Chunks ch = chunks_of(c);
        const int nblk = c->Gp / 64; // one workgroup per CI record group (64 chunks)
        const size_t sm = smem_fwdbwd<N, KIND>(lds_symbols(c), KIND == EMIT_DISC ? m.dcopies : 1);
        if (KIND == EMIT_DISC && c->bt_global && MODE == MODE_ESTEP) // the global count tables
            BHMM_HIP(hipMemsetAsync(c->d_dpartials.p, 0,
                                    (size_t)DISC_GLOBAL_TABLES * c->M * N * sizeof(double), c->stream));
        if constexpr (MODE == MODE_ESTEP) {
            // (every E-step kernel takes the same arguments)
            const void *o16 = nullptr; // (set for the split launches below when they read the 16-bit observations)
            c->last.obs16_used = false;
            auto estep = [&](auto kern, int grid, const Model<N> &mm, size_t smem, double *gam, const Carry &cy) {
                return launch(kern, dim3(grid), dim3(32 * N), smem, c->stream, mm, ch, c->d_obs_ci.p, c->d_obs_rm.p,
                              o16, c->d_offsets.p, c->d_Bt.p, c->d_aentry.p, c->d_bexit.p, c->d_aexit.p, c->d_bentry.p,
                              c->ds.spec_W, c->d_ws.p, gam, c->d_logLc.p, c->d_gamma0.p, c->d_partials.p,
                              c->d_dpartials.p, flag_words, c->d_ea.p, cy);
            };
            double *gam = store_gamma ? c->d_gamma_ci.p : nullptr;
            // the branch-free instantiation needs the verdict round trip of the speculative
            // path to report zero / denormal vectors; everything else runs the careful one
            // (it rescales only every few steps: emission values must stay far from the
            // exponent range -- caller-supplied pobs and very narrow gaussians do not qualify)
            bool fast = SPEC && !store_gamma && !c->ds.careful && KIND != EMIT_EXPL;
            if (KIND == EMIT_GAUSS)
                for (int i = 0; i < c->n; ++i)
                    fast = fast && m.e2[i] < 1048576.0;
            if (fast) {
                if constexpr (SPEC && ESTEP_SPLIT) {
                    // two launches: forward sweeps + backward warm-ups side by side (four
                    // wavefronts per SIMD), then the backward sweeps
                    // P1 keeps no emission counts: without the count tables its workgroups need
                    // less LDS (discrete kind: four of them fit a CU again) and the exchange area of
                    // the all-gather sits right behind B^T
                    Model<N> m1 = m;
                    m1.dcopies = 0;
                    const size_t sm1 = KIND == EMIT_DISC ? smem_fwdbwd<N, KIND>(lds_symbols(c), 0) : sm;
                    // boundary vectors carried between E-steps (decided by estep_kind): P1 starts its
                    // warm-ups from them, P2 captures beta for the next E-step
                    if (KIND == EMIT_DISC && c->obs16 && c->opt.obs16_enabled && !c->bt_global) {
                        o16 = c->d_obs16.p;
                        c->last.obs16_used = true;
                    }
                    Carry c1, c2;
                    if (c->ds.carry_use > 0) {
                        c1.a_in = c->d_carry_a.p;
                        c1.b_in = c->d_carry_b.p;
                        c1.da = c->d_carry_da.p;
                        c1.db = c->d_carry_db.p;
                    }
                    BHMM_HIP(estep(k_estep_light<N, KIND, SPEC, false, false, PH_P1>, 2 * nblk, m1, sm1, nullptr, c1));
                    c2.cap = c->ds.carry_cap;
                    if (c->ds.carry_cap > 0 && c->carry_store) {
                        // (P1 has consumed the old vectors: the same buffers take the new ones)
                        BHMM_HIP(hipMemsetAsync(c->d_carry_db.p, 0, (size_t)c->Gp * sizeof(int32_t),
                                                c->stream));
                        c2.b_out = c->d_carry_b.p;
                        c2.db_out = c->d_carry_db.p;
                    }
                    BHMM_HIP(estep(k_estep<N, KIND, SPEC, false, false, PH_P2>, nblk, m, sm, nullptr, c2));
                    if (c->ds.carry_cap > 0 && c->carry_store)
                        BHMM_HIP(launch(k_carry_alpha<N>, dim3((c->G + 255) / 256), dim3(256), 0, c->stream, ch, c->G,
                                        c->d_ws.p, c->carry_Wout, c->d_carry_a.p, c->d_carry_da.p));
                } else {
                    c->ds.carry_cap = 0;
                    BHMM_HIP(estep(k_estep<N, KIND, SPEC, false, false>, nblk, m, sm, gam, Carry()));
                }
            } else {
                // the exact fallback always uses the gamma-capable, careful instantiation
                c->ds.carry_cap = 0; // (no capture outside the split launches)
                BHMM_HIP(estep(k_estep<N, KIND, SPEC, true, true>, nblk, m, sm, gam, Carry()));
            }
        } else {
            static_assert(MODE == MODE_ESTEP || !SPEC, "row passes take exact boundaries");
            const size_t smr = (size_t)(KIND == EMIT_DISC ? lds_symbols(c) * N : 0) * sizeof(double);
            BHMM_HIP(launch(k_rows<N, KIND, MODE>, dim3(nblk), dim3(32 * N), smr, c->stream, m, ch, c->d_obs_ci.p,
                            c->d_Bt.p, c->d_aentry.p, c->d_bexit.p, c->d_ws.p, c->d_logLc.p));
        }
        BHMM_HIP(hipEventRecord(c->ev[3], c->stream));
        return BHMM_OK;
    }

    template <int KIND>
    static int finish(bhmm_ctx *c, const Model<N> &m, double *stats_dev)
    {
        BHMM_HIP(launch(k_logl, dim3(c->K), dim3(64), 0, c->stream, c->d_traj_c0.p, c->K, c->d_logLc.p, c->d_logLk.p));
        const int nfin = StatLayout<N, KIND>::S + (KIND == EMIT_DISC ? c->M * N : 0) + N + 1;
        BHMM_HIP(launch(k_finalize<N, KIND>, dim3(nfin), dim3(64), 0, c->stream, m, c->K, c->Gp / 64, c->d_partials.p,
                        c->d_dpartials.p, c->d_logLk.p, c->d_gamma0.p, stats_dev));
        return BHMM_OK;
    }

    // Speculative E-step: no prescan / stitch; chunk boundaries from warm-ups, verified.
    // Returns BHMM_OK with *verified = false when the caller has to run the exact pipeline.
    template <int KIND>
    static int estep_spec(bhmm_ctx *c, const Model<N> &m, double *stats_dev, int flags,
                          bool *verified)
    {
        *verified = false;
#ifdef ESTEP_CLOCKPROBE
        int rc = spec_prepare(c);
#else
        int rc = spec_prepare(c, false); // the tail kernel clears the verdict words itself
#endif
        if (rc)
            return rc;
#ifdef ESTEP_CLOCKPROBE
        // instrumented build: separate tail kernels, probe records behind the verdict words
        BHMM_HIP(hipEventRecord(c->ev[0], c->stream));
        BHMM_HIP(hipEventRecord(c->ev[1], c->stream));
        BHMM_HIP(hipEventRecord(c->ev[2], c->stream));
        rc = fwdbwd<KIND, MODE_ESTEP, true>(c, m, (flags & BHMM_FLAG_STORE_GAMMA) != 0);
        if (rc)
            return rc;
        if ((rc = finish<KIND>(c, m, stats_dev)))
            return rc;
        BHMM_HIP(hipEventRecord(c->ev[4], c->stream));
        c->ev_lean = false;
        if ((rc = spec_verdict(c, true, verified, stats_dev)))
            return rc;
#else
        // sweep kernel, one tail kernel (statistics, log-likelihoods, boundary check), one
        // device-to-host copy of [verdict words | statistics | logL_k], one synchronisation
        const int S = stats_size(c);
        const size_t ntail = 4 + (size_t)S + std::max(c->K, 1);
        if (!c->tail_ready) {
            if ((rc = c->d_tail.ensure(ntail)))
                return rc;
            BHMM_HIP(hipMemsetAsync(c->d_tail.p, 0, 4 * sizeof(double), c->stream));
            c->tail_slot = 0;
            c->tail_ready = true;
        }
        const int slot = c->tail_slot;
        c->tail_slot ^= 1;
        unsigned int *words = reinterpret_cast<unsigned int *>(c->d_tail.p) + 4 * slot;
        unsigned int *words_next = reinterpret_cast<unsigned int *>(c->d_tail.p) + 4 * (slot ^ 1);
        BHMM_HIP(hipEventRecord(c->ev[2], c->stream));
        rc = fwdbwd<KIND, MODE_ESTEP, true>(c, m, (flags & BHMM_FLAG_STORE_GAMMA) != 0, words);
        if (rc)
            return rc;
        const int nfin = StatLayout<N, KIND>::S + (KIND == EMIT_DISC ? c->M * N : 0) + N + 1;
        const int tpb = tail_tpb(c->G, c->K);
        const int nTB = (c->K + tpb - 1) / tpb;
        const bool fused_total = nTB <= 1024; // beyond: a fence + ticket per block costs more than a launch
        if ((rc = c->d_tbpart.ensure((size_t)nTB * (1 + N))))
            return rc;
        // very many sweep workgroups: fold their partial statistics 128 rows at a time first
        int nrows = c->Gp / 64;
        const double *part_src = c->d_partials.p, *dpart_src = c->d_dpartials.p;
        if (nrows > 2048) {
            constexpr int SS = StatLayout<N, KIND>::S;
            const int MN = (KIND == EMIT_DISC && !m.bt_global) ? c->M * N : 0;
            const int nf = (nrows + FOLD_ROWS - 1) / FOLD_ROWS;
            if ((rc = c->d_fold.ensure((size_t)nf * (SS + MN))))
                return rc;
            BHMM_HIP(launch(k_fold_rows, dim3(nf), dim3(256), 0, c->stream, c->d_partials.p, nrows, SS, c->d_fold.p));
            part_src = c->d_fold.p;
            if (MN) {
                BHMM_HIP(launch(k_fold_rows, dim3(nf), dim3(256), 0, c->stream, c->d_dpartials.p, nrows, MN,
                                c->d_fold.p + (size_t)nf * SS));
                dpart_src = c->d_fold.p + (size_t)nf * SS;
            }
            nrows = nf;
        }
        BHMM_HIP(launch(k_tail<N, KIND>, dim3((nfin + nTB + (c->G + 63) / 64 + TAIL_WAVES - 1) / TAIL_WAVES),
                        dim3(64 * TAIL_WAVES), 0, c->stream, m, chunks_of(c), c->K, c->G, nrows, nfin, c->d_traj_c0.p,
                        part_src, dpart_src, c->d_logLc.p, c->d_gamma0.p, c->d_aentry.p, c->d_aexit.p, c->d_bexit.p,
                        c->d_bentry.p, SPEC_TOL, stats_dev, c->d_logLk.p, c->d_tail.p + 4, S, words, words_next,
                        c->d_tbpart.p, fused_total, tpb));
        if (!fused_total)
            BHMM_HIP(launch(k_tail_total<N>, dim3(1 + N), dim3(64), 0, c->stream, c->n, nTB, c->d_tbpart.p, stats_dev,
                            c->d_tail.p + 4));
        BHMM_HIP(hipEventRecord(c->ev[4], c->stream));
        c->ev_lean = true;
        // many trajectories: their log-likelihoods (K doubles) stay on the device until somebody asks
        // for them (bhmm_estep_fetch) -- a million of them are 8 MB over the host link per E-step,
        // and an EM loop needs only their sum
        c->logLk_prefetched = c->K <= 4096;
        BHMM_HIP(hipMemcpyAsync(c->h_raw, c->d_tail.p,
                                (c->logLk_prefetched ? ntail : 4 + (size_t)S) * sizeof(double),
                                hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        if ((rc = apply_verdict(c, reinterpret_cast<const unsigned int *>(c->h_raw) + 4 * slot,
                                verified, true)))
            return rc;
#endif
        if (*verified)
            c->ev_pending = true;
        return BHMM_OK;
    }

    // Warm-up length from the measured forgetting curve (k_forget_probe): the smallest length
    // after which two differently started chains agree to 1e-13 on every sampled stretch, in
    // both directions, plus 15 %.  The boundary check of every E-step remains the judge.
    template <int KIND>
    static int probe_warmup(bhmm_ctx *c, const Model<N> &m, int *W_out, double target = 0.0)
    {
        if (!(target > 0.0))
            target = 0.01 * c->opt.spec_tol; // (default: 1e-13)
        *W_out = 0;
        const int Wmax = plan::probe_wmax(longest_traj(c));
        if (Wmax == 0)
            return BHMM_OK;
        Probe pr;
        int rc;
        if ((rc = probe_stage(c, c->d_probe, Wmax, 1, pr)))
            return rc;
        BHMM_HIP(launch(k_forget_probe<N, KIND>, dim3((2 * PROBE_P + 63) / 64), dim3(64), 0, c->stream, m,
                        c->d_obs_rm.p, c->d_Bt.p, pr.d_starts, PROBE_P, Wmax, pr.d_curve));
        std::vector<float> curve;
        if ((rc = probe_read(c, pr, curve)))
            return rc;
        *W_out = plan::warmup_of(plan::curve_last(curve.data(), Wmax, (float)target, true), Wmax);
        return BHMM_OK;
    }

    template <int KIND>
    static int estep_kind(bhmm_ctx *c, const Model<N> &m, double *stats_dev, int flags)
    {
        int rc;
        if (c->opt.spec_enabled && !c->ds.spec_calibrated) {
            // first E-step on these observations: measure how fast this model forgets
            c->ds.spec_calibrated = true;
            c->spec_probes_left = 2;
            int W = 0;
            if ((rc = probe_warmup<KIND>(c, m, &W)))
                return rc;
            if (W > 0)
                c->ds.spec_W = W;
            if (c->chunk_mult > 1 && (int64_t)c->ds.spec_W * 16 > c->L && (rc = replan_coarse(c)))
                return rc;
            if ((rc = replan_for_warmup(c)))
                return rc;
        }
        if (c->opt.spec_enabled) {
            // ---- boundary vectors carried from the previous E-step (estep_sweep.hpp: Carry) ----
            // decades of forgetting per step, from the calibrated warm-up (1e-13 after W / 1.15 steps)
            // (the calibration is conservative -- 1e-13 on 256 sampled stretches plus 15 % --; what the
            // boundary check of a full warm-up actually measured is the better estimate, when known)
            double rdec = -log10(0.01 * c->opt.spec_tol) * 1.15 / std::max(c->ds.spec_W, 16);
            if (c->ds.carry_rdec > 0.0)
                rdec = std::min(rdec, c->ds.carry_rdec);
            bool eligible = c->opt.carry_enabled && ESTEP_SPLIT && KIND != EMIT_EXPL && !c->ds.careful &&
                            !(flags & BHMM_FLAG_STORE_GAMMA) && c->G > c->K;
            if (KIND == EMIT_GAUSS) // (the branch-free split launches only, see fwdbwd)
                for (int i = 0; i < c->n; ++i)
                    eligible = eligible && m.e2[i] < 1048576.0;
            const double delta = c->carry_delta;
            c->ds.carry_use = 0;
            if (eligible && c->ds.carry_valid && delta > 0.0 && delta <= 0.05) {
                // predicted boundary deviation of a warm-up of carry_Wc steps from vectors that are
                // off by kappa * delta
                const double pred = c->ds.carry_kappa * delta * pow(10.0, -rdec * c->carry_Wc);
                if (pred <= 0.3 * SPEC_TOL)
                    c->ds.carry_use = c->carry_Wc;
            }
            auto plan_capture = [&]() {
                // capture for the NEXT E-step, sized for twice this step's model change
                c->ds.carry_cap = c->carry_Wout = 0;
                c->carry_store = false;
                if (!eligible || (c->d_carry_a.ensure((size_t)c->Gp * N)) ||
                    (c->d_carry_b.ensure((size_t)c->Gp * N)) || (c->d_carry_da.ensure(c->Gp)) ||
                    (c->d_carry_db.ensure(c->Gp)))
                    return;
                const double dn = delta > 0.0 ? 2.0 * delta : 1e-3;
                const double need = (log10(c->ds.carry_kappa * dn) - log10(0.1 * SPEC_TOL)) / rdec;
                int Wc = ((int)ceil(std::max(need, 16.0)) + 7) / 8 * 8;
                if (Wc > (int)(0.85 * c->ds.spec_W) || Wc + 16 > c->L)
                    return; // not worth it / chunks too short
                c->carry_Wout = Wc;
                c->ds.carry_cap = Wc; // beta at local step Wc: Wc + 1 warm-up steps
                // a model identical to the previous call's: the sweep is split at the same place (it
                // must round like the call before, see Carry::cap) but nothing is stored -- carried
                // starts are only used after a change, and a caller that repeats E-steps on a fixed
                // model should not pay for the two small launches
                c->carry_store = delta != 0.0;
            };
            for (int attempt = 0; attempt < 3; ++attempt) {
                bool ok = false;
                const int W_tried = c->ds.spec_W;
                const int carried = c->ds.carry_use;
                plan_capture();
                if ((rc = estep_spec<KIND>(c, m, stats_dev, flags, &ok)))
                    return rc;
                if (ok) {
                    if (carried > 0) {
                        // what the check measured bounds the sensitivity for the next prediction
                        const double keff = (double)c->last.spec_last_dev /
                                            (delta * pow(10.0, -rdec * carried));
                        c->ds.carry_kappa = std::min(std::max(std::max(0.5 * c->ds.carry_kappa, 8.0 * keff), 1.0), 1e8);
                        c->last.carry_ok++;
                    }
                    if (carried == 0 && c->last.spec_last_dev > 0.f && c->last.spec_last_dev < 1e-6f) {
                        // a full warm-up of spec_W steps from the uniform vector (start error O(1))
                        // left this deviation at the worst boundary
                        const double rr = -log10((double)c->last.spec_last_dev) / std::max(c->ds.spec_W, 16);
                        c->ds.carry_rdec = c->ds.carry_rdec > 0.0 ? std::min(c->ds.carry_rdec, rr) : rr;
                    }
                    c->last.carry_last_W = carried;
                    c->ds.carry_valid = c->ds.carry_cap > 0 && c->carry_store;
                    c->carry_Wc = c->carry_Wout;
                    c->ds.carry_use = 0;
                    return BHMM_OK;
                }
                c->ds.carry_valid = false;
                if (carried > 0 && !c->ds.careful_retry) {
                    // shortened warm-ups did not verify: same call again with full ones
                    c->ds.carry_kappa = std::min(c->ds.carry_kappa * 30.0, 1e8);
                    c->ds.carry_use = 0;
                    continue;
                }
                c->ds.carry_use = 0;
                if (!c->ds.careful_retry) {
                    // boundaries did not verify: exact pipeline now; for the next call measure
                    // the curve again (the model has moved), never below +25 %
                    if (c->opt.spec_enabled && !c->opt.spec_W_fixed && c->spec_probes_left > 0) {
                        --c->spec_probes_left;
                        int W = 0;
                        if ((rc = probe_warmup<KIND>(c, m, &W)))
                            return rc;
                        if (W > 0)
                            c->ds.spec_W = std::max(W, (W_tried * 5 / 4 + 3) / 4 * 4);
                    }
                    break;
                }
                c->ds.careful_retry = false; // zero / denormal vectors: same path, careful kernel
            }
        }
        rc = prescan_stitch<KIND>(c, m);
        if (rc)
            return rc;
        rc = fwdbwd<KIND, MODE_ESTEP>(c, m, (flags & BHMM_FLAG_STORE_GAMMA) != 0);
        if (rc)
            return rc;
        BHMM_HIP(launch(k_logl, dim3(c->K), dim3(64), 0, c->stream, c->d_traj_c0.p, c->K, c->d_logLc.p, c->d_logLk.p));
        const int nfin = StatLayout<N, KIND>::S + (KIND == EMIT_DISC ? c->M * N : 0) + N + 1;
        BHMM_HIP(launch(k_finalize<N, KIND>, dim3(nfin), dim3(64), 0, c->stream, m, c->K, c->Gp / 64, c->d_partials.p,
                        c->d_dpartials.p, c->d_logLk.p, c->d_gamma0.p, stats_dev));
        BHMM_HIP(hipEventRecord(c->ev[4], c->stream));
        c->ev_pending = true;
        return BHMM_OK;
    }

    // probe_warmup at another target (the fp32 E-step, estep_f32.hip)
    static int probe_at(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                        double target, int *W)
    {
        Model<N> m;
        fill_model<N>(m, c->n, c->kind, c->M, A, pi, par0, par1);
        if (c->kind == EMIT_DISC) {
            m.dcopies = disc_copies<N>(c->M);
            m.bt_global = c->bt_global ? 1 : 0;
            return probe_warmup<EMIT_DISC>(c, m, W, target);
        }
        return probe_warmup<EMIT_GAUSS>(c, m, W, target);
    }

    static int estep(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                     const double *par1, double *stats_dev, int flags)
    {
        Model<N> m;
        fill_model<N>(m, c->n, c->kind, c->M, A, pi, par0, par1);
        if (c->kind == EMIT_DISC) {
            m.dcopies = disc_copies<N>(c->M);
            m.bt_global = c->bt_global ? 1 : 0;
        }
        switch (c->kind) {
        case EMIT_GAUSS:
            return estep_kind<EMIT_GAUSS>(c, m, stats_dev, flags);
        case EMIT_DISC:
            return estep_kind<EMIT_DISC>(c, m, stats_dev, flags);
        default:
            return estep_kind<EMIT_EXPL>(c, m, stats_dev, flags);
        }
    }

    // forward-only / backward-only passes on explicit pobs (hidden/api.py forward, backward)
    template <int MODE>
    static int sweep_explicit(bhmm_ctx *c, const double *A, const double *pi)
    {
        Model<N> m;
        fill_model<N>(m, c->n, EMIT_EXPL, 0, A, pi, nullptr, nullptr);
        int rc = prescan_stitch<EMIT_EXPL>(c, m);
        if (rc)
            return rc;
        rc = fwdbwd<EMIT_EXPL, MODE>(c, m, false);
        if (rc)
            return rc;
        if (MODE == MODE_FWD)
            BHMM_HIP(launch(k_logl, dim3(c->K), dim3(64), 0, c->stream, c->d_traj_c0.p, c->K, c->d_logLc.p,
                            c->d_logLk.p));
        return BHMM_OK;
    }

    // verdict of a speculative pass (synchronises the stream)
    static int spec_verdict(bhmm_ctx *c, bool with_beta, bool *verified,
                            const double *stats_src = nullptr)
    {
        BHMM_HIP(launch(k_spec_check<N>, dim3((c->G + 255) / 256), dim3(256), 0, c->stream, chunks_of(c), c->G,
                        c->d_aentry.p, c->d_aexit.p, with_beta ? c->d_bexit.p : nullptr, c->d_bentry.p, SPEC_TOL,
                        c->d_specres.p));
        if (int rc = specres_read(c, 4, false))
            return rc;
        c->prefetched = false;
        if (stats_src) { // the results ride on the same synchronisation as the verdict
            const int S = stats_size(c);
            c->logLk_prefetched = true;
            BHMM_HIP(hipMemcpyAsync(c->h_pinned, stats_src, S * sizeof(double),
                                    hipMemcpyDeviceToHost, c->stream));
            BHMM_HIP(hipMemcpyAsync(c->h_pinned + S, c->d_logLk.p, c->K * sizeof(double),
                                    hipMemcpyDeviceToHost, c->stream));
        }
        BHMM_HIP(hipStreamSynchronize(c->stream));
#ifdef ESTEP_CLOCKPROBE
        {
            const int nb = c->Gp / 64;
            std::vector<unsigned long long> pr(8 * (size_t)nb);
            BHMM_HIP(hipMemcpy(pr.data(), c->d_specres.p + 4, pr.size() * 8, hipMemcpyDeviceToHost));
            unsigned long long r0 = ~0ull, r1 = 0;
            for (int b = 0; b < nb; ++b) {
                r0 = std::min(r0, pr[8 * b + 2]);
                r1 = std::max(r1, pr[8 * b + 3]);
            }
            // early finishers (first half by end time) and late finishers separately
            std::vector<double> ends(nb);
            for (int b = 0; b < nb; ++b)
                ends[b] = (double)(pr[8 * b + 3] - r0);
            std::vector<double> se = ends;
            std::sort(se.begin(), se.end());
            const double med = se[nb / 2];
            double ph[2][4] = {{0}}, cnt[2] = {0, 0}, fr = 0;
            for (int b = 0; b < nb; ++b) {
                const int cls = ends[b] < med ? 0 : 1;
                const unsigned long long t[5] = {pr[8 * b + 2], pr[8 * b + 4], pr[8 * b + 5],
                                                 pr[8 * b + 6], pr[8 * b + 3]};
                for (int k = 0; k < 4; ++k)
                    ph[cls][k] += (double)(t[k + 1] - t[k]) * 0.01;
                cnt[cls] += 1;
                fr += (double)(pr[8 * b + 1] - pr[8 * b]) / (double)(t[4] - t[0]);
            }
            fprintf(stderr, "[probe] span %.0f us, counter/realtime %.2f | early blocks (wave 0): warmF %.0f "
                            "mainF %.0f warmB %.0f mainB %.0f us | late: %.0f %.0f %.0f %.0f us\n",
                    (r1 - r0) * 0.01, fr / nb, ph[0][0] / cnt[0], ph[0][1] / cnt[0], ph[0][2] / cnt[0],
                    ph[0][3] / cnt[0], ph[1][0] / cnt[1], ph[1][1] / cnt[1], ph[1][2] / cnt[1],
                    ph[1][3] / cnt[1]);
        }
#endif
        return apply_verdict(c, c->h_specres, verified, stats_src != nullptr);
    }

    // words: [0] boundaries out of tolerance, [1] largest deviation (float bits), [2] chunks of
    // the branch-free sweep that met a zero / tiny vector
    static int apply_verdict(bhmm_ctx *c, const unsigned int *words, bool *verified,
                             bool results_on_host)
    {
        float dev;
        memcpy(&dev, &words[1], sizeof(float));
        c->last.spec_last_dev = dev;
        *verified = words[0] == 0;
        if (words[2] != 0) {
            // the branch-free sweep met a zero / denormal vector (an all-zero emission row,
            // outputmodel.py:126-130): its statistics are void, repeat with the careful kernel
            // and keep using that one for this set of observations
            *verified = false;
            c->ds.careful = true;
            c->ds.careful_retry = true;
            return BHMM_OK;
        }
        if (*verified) {
            c->prefetched = results_on_host;
            c->last.spec_ok++;
        } else if (c->ds.carry_use > 0) {
            // the shortened warm-ups from carried vectors did not verify: the caller repeats with
            // full warm-ups; this says nothing about the warm-up length itself
            c->last.carry_fail++;
        } else {
            // lengthen the warm-up for the next call; give up once it would cost more than the
            // prescan (slowly mixing model / uninformative data)
            c->last.spec_fail++;
            if (c->ds.spec_W >= 8192 || c->ds.spec_W >= 2 * c->Lmax) {
                c->opt.spec_enabled = false;
            } else {
                // the deviation decays geometrically with the warm-up length: extrapolate to a
                // tenth of the tolerance (at least +25 %, at most x8 per failure)
                const double d = std::min(std::max((double)c->last.spec_last_dev, 1e-300), 0.5);
                const double f = std::min(std::max(log(0.1 * SPEC_TOL) / log(d), 1.25), 8.0);
                c->ds.spec_W = std::max(c->ds.spec_W + 4, ((int)ceil(c->ds.spec_W * f) + 3) / 4 * 4);
            }
        }
        return BHMM_OK;
    }

    static int spec_prepare(bhmm_ctx *c, bool clear_words = true)
    {
        int rc;
        if ((rc = c->d_aexit.ensure((size_t)c->Gp * N)) || (rc = c->d_bentry.ensure((size_t)c->Gp * N)) ||
#ifdef ESTEP_CLOCKPROBE
            (rc = ensure_specres(c, 4 + 16 * (size_t)(c->Gp / 64))))
#else
            (rc = ensure_specres(c)))
#endif
            return rc;
        return clear_words ? specres_reset(c) : BHMM_OK;
    }

    // forward sweep only with k_estep<..., FWDONLY> (alpha rows up to a power of two)
    template <int KIND, bool CAREFUL>
    static int forward_launch(bhmm_ctx *c, const Model<N> &m_in)
    {
        const Chunks ch = chunks_of(c);
        Model<N> m = m_in; // no emission counts in this pass: no count tables in LDS
        m.dcopies = 0;
        const size_t sm = smem_fwdbwd<N, KIND>(lds_symbols(c), KIND == EMIT_DISC ? 0 : 1);
        // every alpha row in fp32 (in the gamma_ci slot of the kernel), every FWD_CKPT-th in fp64
        int rc = c->d_ws32.ensure((size_t)ci_records(c) * N * 64);
        if (rc)
            return rc;
        BHMM_HIP(launch(k_estep_light<N, KIND, true, false, CAREFUL, PH_FWDROWS>, dim3(c->Gp / 64), dim3(32 * N), sm,
                        c->stream, m, ch, c->d_obs_ci.p, c->d_obs_rm.p, nullptr, c->d_offsets.p, c->d_Bt.p, c->d_aentry.p,
                        c->d_bexit.p, c->d_aexit.p, c->d_bentry.p, c->ds.spec_W, c->d_ws.p,
                        reinterpret_cast<double *>(c->d_ws32.p), c->d_logLc.p, c->d_gamma0.p, c->d_partials.p,
                        c->d_dpartials.p, c->d_specres.p, c->d_ea.p, Carry()));
        c->rows32_valid = true;
        return BHMM_OK;
    }

    template <int KIND>
    static int forward_kind(bhmm_ctx *c, const Model<N> &m)
    {
        int rc;
        if (c->opt.spec_enabled && !c->ds.spec_calibrated) {
            c->ds.spec_calibrated = true;
            c->spec_probes_left = 2;
            int W = 0;
            if ((rc = probe_warmup<KIND>(c, m, &W)))
                return rc;
            if (W > 0)
                c->ds.spec_W = W;
            if (c->chunk_mult > 1 && (int64_t)c->ds.spec_W * 16 > c->L && (rc = replan_coarse(c)))
                return rc;
            if ((rc = replan_for_warmup(c)))
                return rc;
        }
        if (c->opt.spec_enabled) {
            for (int attempt = 0; attempt < 2; ++attempt) {
                bool ok = false;
                bool fast = !c->ds.careful && KIND != EMIT_EXPL;
                if (KIND == EMIT_GAUSS)
                    for (int i = 0; i < c->n; ++i)
                        fast = fast && m.e2[i] < 1048576.0;
                if ((rc = spec_prepare(c)))
                    return rc;
                rc = fast ? forward_launch<KIND, false>(c, m) : forward_launch<KIND, true>(c, m);
                if (rc)
                    return rc;
                if (c->fwd_defer && attempt == 0) {
                    // the caller keeps launching on the stream and reads the verdict with its own
                    // results (forward_ci_verdict): one host round trip less per Gibbs sweep
                    BHMM_HIP(launch(k_spec_check<N>, dim3((c->G + 255) / 256), dim3(256), 0, c->stream, chunks_of(c),
                                    c->G, c->d_aentry.p, c->d_aexit.p, nullptr, c->d_bentry.p, SPEC_TOL, c->d_specres.p));
                    if ((rc = specres_read(c, 4, false)))
                        return rc;
                    c->prefetched = false;
                    c->fwd_pending = true;
                    return BHMM_OK;
                }
                if ((rc = spec_verdict(c, false, &ok)))
                    return rc;
                if (ok)
                    return BHMM_OK;
                if (!c->ds.careful_retry)
                    break;
                c->ds.careful_retry = false;
            }
        }
        if ((rc = prescan_stitch<KIND>(c, m)))
            return rc;
        c->rows32_valid = false; // the exact pass writes every row in fp64
        return fwdbwd<KIND, MODE_FWD>(c, m, false);
    }

    // forward pass only, alpha (any scale per row; _hidden.c:16-66 up to that) left in the CI workspace
    static int forward_only(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
                            const double *par1)
    {
        Model<N> m;
        fill_model<N>(m, c->n, c->kind, c->M, A, pi, par0, par1);
        if (c->kind == EMIT_DISC) {
            m.dcopies = disc_copies<N>(c->M);
            m.bt_global = c->bt_global ? 1 : 0;
        }
        switch (c->kind) {
        case EMIT_GAUSS:
            return forward_kind<EMIT_GAUSS>(c, m);
        case EMIT_DISC:
            return forward_kind<EMIT_DISC>(c, m);
        default:
            return forward_kind<EMIT_EXPL>(c, m);
        }
    }

    // verdict of a deferred forward-only pass, after the caller synchronised the stream
    static int forward_verdict(bhmm_ctx *c, bool *ok)
    {
        return apply_verdict(c, c->h_specres, ok, false);
    }

    static int pack_rows(bhmm_ctx *c, const double *src_dev)
    {
        BHMM_HIP(launch(k_pack_rows<N>, dim3(c->Gp / BLOCK), dim3(BLOCK), 0, c->stream, chunks_of(c), src_dev, c->n,
                        reinterpret_cast<double *>(c->d_obs_ci.p)));
        return BHMM_OK;
    }

    static int unpack_rows(bhmm_ctx *c, const double *src_ci, double *dst_dev, int only_traj,
                           int64_t shift)
    {
        BHMM_HIP(launch(k_unpack_rows<N>, dim3(c->Gp / BLOCK), dim3(BLOCK), 0, c->stream, chunks_of(c), src_ci, c->n,
                        dst_dev, only_traj, shift));
        return BHMM_OK;
    }
};

#define BHMM_DISPATCH_N(c, expr)            \
    ((c)->N == 2 ? Runner<2>::expr          \
     : (c)->N == 4 ? Runner<4>::expr        \
                   : Runner<8>::expr)

// ---- chunk planning ----------------------------------------------------------------------
// Every trajectory is cut into ceil(T/L) chunks whose lengths differ by at most one.
static int plan_chunks(bhmm_ctx *c, int chunk, bool allow_mult = true, bool half = false)
{
    // the tables come from plan.hpp (pure host code, also built under the CPU sanitizers); here
    // they are adopted and uploaded
    const int K = c->K;
    plan::ChunkPlan p;
    if (!plan::plan_chunks(c->offsets, K, c->N, c->total, chunk, allow_mult, BLOCK, p, half))
        return invalid_arg("too many chunks");
    c->chunk_mult = p.chunk_mult;
    c->L = p.L;
    c->traj_c0 = p.traj_c0;
    c->G = p.G;
    c->Gp = p.Gp;
    c->Lmax = p.Lmax;
    int rc;
    if ((rc = c->d_ctraj.ensure(c->Gp)) || (rc = c->d_clen.ensure(c->Gp)) ||
        (rc = c->d_ct0.ensure(c->Gp)) || (rc = c->d_cgoff.ensure(c->Gp)) ||
        (rc = c->d_traj_c0.ensure(K + 1)))
        return rc;
    BHMM_HIP(hipMemcpy(c->d_ctraj.p, p.ctraj.data(), c->Gp * sizeof(int32_t), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(c->d_clen.p, p.clen.data(), c->Gp * sizeof(int32_t), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(c->d_ct0.p, p.ct0.data(), c->Gp * sizeof(int64_t), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(c->d_cgoff.p, p.cgoff.data(), c->Gp * sizeof(int64_t), hipMemcpyHostToDevice));
    BHMM_HIP(hipMemcpy(c->d_traj_c0.p, c->traj_c0.data(), (K + 1) * sizeof(int32_t),
                       hipMemcpyHostToDevice));
    if ((rc = c->d_offsets.ensure(K + 1)))
        return rc;
    BHMM_HIP(hipMemcpy(c->d_offsets.p, c->offsets.data(), (K + 1) * sizeof(int64_t),
                       hipMemcpyHostToDevice));
    // two-level stitch: groups of R consecutive chunks; serial depth 2R + n/R instead of n
    c->nG = p.nG;
    if (c->nG > 0) {
        const size_t MSz = (size_t)c->N * c->N + c->N;
        if ((rc = c->d_grp_c0.ensure(c->nG)) || (rc = c->d_grp_c1.ensure(c->nG)) ||
            (rc = c->d_grp_traj0.ensure(K + 1)) || (rc = c->d_P.ensure((size_t)c->nG * MSz)) ||
            (rc = c->d_agrp.ensure((size_t)c->nG * c->N)) ||
            (rc = c->d_bgrp.ensure((size_t)c->nG * c->N)))
            return rc;
        BHMM_HIP(hipMemcpy(c->d_grp_c0.p, p.g0.data(), c->nG * sizeof(int32_t), hipMemcpyHostToDevice));
        BHMM_HIP(hipMemcpy(c->d_grp_c1.p, p.g1.data(), c->nG * sizeof(int32_t), hipMemcpyHostToDevice));
        BHMM_HIP(hipMemcpy(c->d_grp_traj0.p, p.gt.data(), (K + 1) * sizeof(int32_t),
                           hipMemcpyHostToDevice));
    }
    return BHMM_OK;
}

static int stats_size(const bhmm_ctx *c)
{
    const int n = c->n;
    int s = 1 + n + n * n + n;
    if (c->kind == EMIT_GAUSS)
        s += 2 * n;
    else if (c->kind == EMIT_DISC)
        s += n * c->M;
    return s;
}

// pinned landing zone: 4 doubles of verdict words in front of [stats | logL_k]
static int ensure_pinned(bhmm_ctx *c, size_t need)
{
    if (need > c->h_pinned_n) {
        if (c->h_raw)
            (void)hipHostFree(c->h_raw);
        c->h_raw = c->h_pinned = nullptr;
        BHMM_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_raw), (need + 4) * sizeof(double),
                               hipHostMallocDefault));
        c->h_pinned = c->h_raw + 4;
        c->h_pinned_n = need;
    }
    return BHMM_OK;
}

static int alloc_work(bhmm_ctx *c)
{
    const int N = c->N;
    int rc;
    const int S = N * N + 3 * N;
    if ((rc = c->d_M.ensure((size_t)c->Gp * (N * N + N))) ||
        (rc = c->d_aentry.ensure((size_t)c->Gp * N)) || (rc = c->d_bexit.ensure((size_t)c->Gp * N)) ||
        (rc = c->d_ws.ensure((size_t)ci_records(c) * N * 64)) ||
        (rc = c->d_ea.ensure((size_t)c->Gp + (size_t)ci_records(c) * 64)) ||
        (rc = c->d_logLc.ensure(c->Gp)) || (rc = c->d_logLk.ensure(std::max(c->K, 1))) ||
        (rc = c->d_gamma0.ensure((size_t)std::max(c->K, 1) * N)) ||
        (rc = c->d_partials.ensure((size_t)(c->Gp / 64) * S)) ||
        (rc = c->d_stats.ensure(stats_size(c))))
        return rc;
    if (c->kind == EMIT_DISC) {
        const size_t ntab = c->bt_global ? (size_t)DISC_GLOBAL_TABLES : (size_t)(c->Gp / 64);
        if ((rc = c->d_dpartials.ensure(ntab * c->M * N)) ||
            (rc = c->d_Bt.ensure((size_t)c->M * N)))
            return rc;
    }
    // chunks past G (padding) never write logL: clear once
    BHMM_HIP(hipMemsetAsync(c->d_logLc.p, 0, c->Gp * sizeof(double), c->stream));
    BHMM_HIP(hipMemsetAsync(c->d_gamma0.p, 0, (size_t)std::max(c->K, 1) * N * sizeof(double),
                            c->stream));
    c->tail_ready = false;
    return ensure_pinned(c, (size_t)stats_size(c) + c->K);
}

static int upload_Bt(bhmm_ctx *c, const double *B)
{
    std::vector<double> bt((size_t)c->M * c->N, 0.0);
    fill_Bt_padded(c->n, c->N, c->M, B, bt.data());
    BHMM_HIP(hipMemcpyAsync(c->d_Bt.p, bt.data(), bt.size() * sizeof(double),
                            hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream)); // bt is a temporary
    return BHMM_OK;
}

int forward_ci(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
               const double *par1)
{
    int rc;
    if (c->kind == BHMM_EMIT_DISCRETE && (rc = upload_Bt(c, par0)))
        return rc;
    return BHMM_DISPATCH_N(c, forward_only(c, A, pi, par0, par1));
}

int forward_ci_verdict(bhmm_ctx *c, bool *ok)
{
    return BHMM_DISPATCH_N(c, forward_verdict(c, ok));
}

int unpack_ws_rows(bhmm_ctx *c, double *dst_dev)
{
    return BHMM_DISPATCH_N(c, unpack_rows(c, c->d_ws.p, dst_dev, -1, 0));
}

int probe_warmup_target(bhmm_ctx *c, const double *A, const double *pi, const double *par0, const double *par1,
                        double target, int *W)
{
    return BHMM_DISPATCH_N(c, probe_at(c, A, pi, par0, par1, target, W));
}

static void collect_timing(bhmm_ctx *c)
{
    if (!c->ev_pending)
        return;
    c->ev_pending = false;
    float ms = 0.f;
    if (c->ev_lean) { // sweep kernel, tail kernel; no prescan / stitch
        c->last.ms[0] = c->last.ms[1] = 0.0;
        if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess)
            c->last.ms[2] = ms;
        if (hipEventElapsedTime(&ms, c->ev[3], c->ev[4]) == hipSuccess)
            c->last.ms[3] = ms;
        if (hipEventElapsedTime(&ms, c->ev[2], c->ev[4]) == hipSuccess)
            c->last.ms[4] = ms;
        (void)hipGetLastError();
        return;
    }
    for (int i = 0; i < 4; ++i)
        if (hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]) == hipSuccess)
            c->last.ms[i] = ms;
    if (hipEventElapsedTime(&ms, c->ev[0], c->ev[4]) == hipSuccess)
        c->last.ms[4] = ms;
    (void)hipGetLastError();
}

} // namespace bhmm

using namespace bhmm;

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

const char *bhmm_last_error(void) { return g_err.c_str(); }

const char *bhmm_version(void) { return "bhmm_amd 0.1 gfx950"; }

int bhmm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int bhmm_ctx_create(bhmm_ctx **out, int device, void *stream)
{
    if (!out)
        return invalid_arg("out == NULL");
    *out = nullptr;
    int ndev = bhmm_device_count();
    if (ndev <= 0) {
        g_err = "no HIP device visible";
        return BHMM_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev)
        return invalid_arg("device ordinal out of range");
    BHMM_HIP(hipSetDevice(device));
    bhmm_ctx *c = new (std::nothrow) bhmm_ctx();
    if (!c)
        return BHMM_ERR_NO_MEM;
    c->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            c->num_simd = 4 * cus;
        (void)hipGetLastError();
    }
    if (const char *e = getenv("BHMM_AMD_CARRY"))
        c->opt.carry_enabled = atoi(e) != 0;
    if (const char *e = getenv("BHMM_AMD_SPEC"))
        c->opt.spec_enabled = atoi(e) != 0;
    if (const char *e = getenv("BHMM_AMD_TILE"))
        c->opt.tile_enabled = atoi(e) != 0;
    if (const char *e = getenv("BHMM_AMD_TILE_PER_CU"))
        c->opt.tile_per_cu = std::max(1, std::min(4, atoi(e)));
    // (sweeps: the watched-draw machinery of draw_verify.hpp with a wide watch / with every watched draw treated as
    // a decision that did not stand, on whatever problems the sweep draws)
    if (const char *e = getenv("BHMM_AMD_DRAW_WATCH_TOL"))
        c->opt.draw_watch_tol = std::min(0.5, std::max(0.0, atof(e)));
    if (const char *e = getenv("BHMM_AMD_DRAW_TEST_REDO"))
        c->opt.draw_test_redo = atoi(e) != 0;
    if (const char *e = getenv("BHMM_AMD_SPEC_W")) {
        c->ds.spec_W = std::max(1, atoi(e));
        c->opt.spec_W_fixed = true;
    }
    if (stream) {
        c->stream = static_cast<hipStream_t>(stream);
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete c;
            return hip_fail(e, "hipStreamCreate");
        }
        c->own_stream = true;
    }
    for (auto &ev : c->ev) {
        hipError_t e = hipEventCreate(&ev);
        if (e != hipSuccess) {
            bhmm_ctx_destroy(c);
            return hip_fail(e, "hipEventCreate");
        }
    }
    *out = c;
    return BHMM_OK;
}

int bhmm_ctx_destroy(bhmm_ctx *c)
{
    if (!c)
        return BHMM_OK;
    (void)hipSetDevice(c->device);
    if (c->stream)
        (void)hipStreamSynchronize(c->stream);
    if (c->h_specres)
        (void)hipHostFree(c->h_specres);
    if (c->h_small)
        (void)hipHostFree(c->h_small);
    if (c->h_raw)
        (void)hipHostFree(c->h_raw);
    for (auto &ev : c->ev)
        if (ev)
            (void)hipEventDestroy(ev);
    if (c->own_stream && c->stream)
        (void)hipStreamDestroy(c->stream);
    delete c; // (every DevBuf frees its allocation)
    return BHMM_OK;
}

extern "C++" {
// re-lay the trajectory-major observations at src_dev (device) out chunk-interleaved for the
// current chunk plan
static int pack_observations(bhmm_ctx *c, const char *src_dev)
{
    const int kind = c->kind;
    int rc;
    const size_t ci_elems = (size_t)ci_records(c) * 64;
    const Chunks ch = chunks_of(c);
    const int nblk = c->Gp / BLOCK;
    if ((rc = c->d_obsnan.ensure(2))) // [1]: a discrete symbol outside [0, M) (k_pack_obs16)
        return rc;
    BHMM_HIP(hipMemsetAsync(c->d_obsnan.p, 0, 2 * sizeof(int32_t), c->stream));
    c->obs16 = false;
    if (kind == BHMM_EMIT_GAUSSIAN) {
        if ((rc = c->d_obs_ci.ensure(ci_elems * sizeof(double))))
            return rc;
        BHMM_HIP(launch(k_pack_scalar<double>, dim3(nblk), dim3(BLOCK), 0, c->stream, ch,
                        reinterpret_cast<const double *>(src_dev), reinterpret_cast<double *>(c->d_obs_ci.p),
                        c->d_obsnan.p));
    } else if (kind == BHMM_EMIT_DISCRETE) {
        if ((rc = c->d_obs_ci.ensure(ci_elems * sizeof(int32_t))))
            return rc;
        BHMM_HIP(launch(k_pack_scalar<int32_t>, dim3(nblk), dim3(BLOCK), 0, c->stream, ch,
                        reinterpret_cast<const int32_t *>(src_dev), reinterpret_cast<int32_t *>(c->d_obs_ci.p),
                        c->d_obsnan.p));
        // the second, 16-bit copy (2 bytes per step more) for the main loops of the split E-step: B^T in LDS and
        // every row offset within 16 bits; the int32 copy above stays for everything else
        if (c->opt.obs16_enabled && !c->bt_global && obs16_fits(c->N, c->M)) {
            if ((rc = c->d_obs16.ensure((size_t)(c->Gp / 64) * obs16_blocks(c->Lmax) * 64 * OBS16_BLK)))
                return rc;
            BHMM_HIP(launch(k_pack_obs16, dim3(nblk), dim3(BLOCK), 0, c->stream, ch,
                            reinterpret_cast<const int32_t *>(src_dev), c->d_obs16.p, c->N, c->M, c->d_obsnan.p + 1));
            c->obs16 = true; // (until pack_settle has looked at the symbols)
        }
    } else {
        if ((rc = c->d_obs_ci.ensure(ci_elems * sizeof(double) * c->N)))
            return rc;
        rc = BHMM_DISPATCH_N(c, pack_rows(c, reinterpret_cast<const double *>(src_dev)));
        if (rc)
            return rc;
    }
    return BHMM_OK;
}

// after pack_observations, once the stream has been waited for: a symbol outside [0, M) keeps the context off the
// 16-bit copy (it holds such a symbol modulo 2^16, the int32 copy as it is)
static int pack_settle(bhmm_ctx *c, int32_t *has_nan)
{
    int32_t words[2] = {0, 0};
    BHMM_HIP(hipMemcpyAsync(words, c->d_obsnan.p, sizeof(words), hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    if (words[1])
        c->obs16 = false;
    if (has_nan)
        *has_nan = words[0];
    return BHMM_OK;
}

// The automatic plan took two or three times the default chunk count because the chunks were very
// long (plan_chunks), assuming a warm-up of a few hundred steps.  The model turned out to forget
// slowly (the calibrated warm-up exceeds 1/16 of the chunk): back to the default count -- the
// observations are re-laid out from the trajectory-major copy on the device.
// The automatic plan cuts every batch into the default number of chunks.  Once the warm-up of the
// model is known: if those chunks are shorter than about 1.6 warm-ups, half as many are faster
// (plan.hpp).  Only for a plan that did reach the default count -- below it the device is not full
// and more chunks mean more parallelism -- and only once per set of observations.
int bhmm::replan_for_warmup(bhmm_ctx *c)
{
    if (!c->ds.chunk_auto || c->ds.replanned_half || c->chunk_mult > 1 || c->wide || c->gen)
        return BHMM_OK;
    if ((int64_t)c->G * 10 < plan::default_chunk_count(c->N) * 9 || (double)c->L >= 1.6 * c->ds.spec_W)
        return BHMM_OK;
    c->ds.replanned_half = true;
    return replan_coarse(c, true);
}

int bhmm::replan_coarse(bhmm_ctx *c, bool half, int chunk)
{
    int rc;
    BHMM_HIP(hipStreamSynchronize(c->stream));
    if ((rc = plan_chunks(c, chunk, false, half)) || (rc = alloc_work(c)))
        return rc;
    if ((rc = pack_observations(c, c->d_obs_rm.p)) || (rc = pack_settle(c, nullptr)))
        return rc;
    // rows stored under the old plan are gone; an E-step in flight that stores gamma (this runs
    // inside its first call) gets rows of the new plan's size -- bhmm_estep sets gamma_valid
    // when that E-step has been enqueued
    c->ds.gamma_valid = false;
    if (c->gamma_wanted && (rc = c->d_gamma_ci.ensure((size_t)ci_records(c) * c->N * 64)))
        return rc;
    c->ds.carry_valid = false; // (vectors of the old plan's chunks)
    c->rows32_valid = false;
    return BHMM_OK;
}
} // extern "C++"

// The adaptive state of a new observation set (ctx.hpp, bhmm_ctx::ObservationSet): the defaults, except
// for what follows from the options and from the number of states.
static void new_observation_set(bhmm_ctx *c)
{
    const int spec_W = c->ds.spec_W;
    c->ds = {};
    if (c->opt.spec_W_fixed)
        c->ds.spec_W = spec_W; // (the caller's choice: no probe)
    c->ds.spec_calibrated = c->opt.spec_W_fixed;
    c->ds.tile_latched = c->opt.tile_enabled; // (ctx.hpp: one decision per set of observations)
    // 33..64 states: the margin rule from the first call on (round 6).  On observations that follow the model --
    // what a Viterbi pass after EM sees -- most boundaries of the first pass carry rounding noise and a fix-up round
    // runs for half a pass (6.7 ms at configs[3]) where margins + mending take 2.6; on white-noise data the round is
    // 0.5 ms cheaper.  Below 33 states a round is short either way: there the rule waits for a call that needed it.
    // (BHMM_AMD_VIT_MARGIN_FORCE: the rule at every state count, for the sweeps)
    c->ds.vit.margin_want = getenv("BHMM_AMD_VIT_MARGIN_FORCE") != nullptr || (c->n > 32 && c->n <= 64);
}

int bhmm_ctx_set_observations(bhmm_ctx *c, int kind, const void *obs, const int64_t *offsets, int K,
                              int nstates, int nsymbols, int chunk, int obs_on_device)
{
    if (!c || !offsets || K < 1)
        return invalid_arg("bad context / offsets / K");
    if (kind < 0 || kind > 2)
        return invalid_arg("unknown emission kind");
    if (nstates < 1 || nstates > 4096)
        return invalid_arg("1..4096 hidden states are supported");
    if (kind == BHMM_EMIT_DISCRETE && nsymbols < 1)
        return invalid_arg("nsymbols must be >= 1 for discrete emissions");
    BHMM_HIP(hipSetDevice(c->device));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    if (!c->mvn.reloading && c->mvn.active) { // observations of another kind: the multivariate set ends (mvn_api.hip)
        auto &b = c->mvn;                     // and gives its memory back
        b.active = b.rows_valid = false;
        b.X.release(), b.rows.release(), b.m.release(), b.shift.release(), b.d_offsets.release();
        b.tab.release(), b.part.release(), b.out.release();
        c->gmm.forget(), c->gmm.resp.release(), c->gmm.tab.release(), c->gmm.labels.release();
    }
    c->d_soff.release(); // random-stream positions belong to the previous trajectories
    c->last_stats = nullptr;
    c->kind = kind;
    c->n = nstates;
    c->gen = nstates > 64; // any-N family (gen_kernels.hpp); 9..64: the wide family
    c->wide = nstates > 8 && !c->gen;
    c->N = pad_states(nstates);
    c->M = kind == BHMM_EMIT_DISCRETE ? nsymbols : 0;
    c->K = K;
    for (int k = 0; k < K; ++k)
        if (offsets[k + 1] < offsets[k])
            return invalid_arg("offsets must be non-decreasing");
    c->offsets.resize(K + 1);
    for (int k = 0; k <= K; ++k) // positions relative to the first element handed over
        c->offsets[k] = offsets[k] - offsets[0];
    c->total = c->offsets[K];
    if (c->total <= 0)
        return invalid_arg("no observations");
    if (obs == nullptr)
        return invalid_arg("obs == NULL");
    new_observation_set(c);
    // discrete alphabets whose emission / count tables do not fit the LDS of the sweep kernels
    // (M above ~1200 at 8 states) keep them in global memory instead (estep_sweep.hpp, BtSrc)
    c->obs16 = false;
    c->bt_global = kind == BHMM_EMIT_DISCRETE && !c->wide && !c->gen &&
                   smem_fwdbwd<8, EMIT_DISC>(c->M) > (size_t)150 * 1024;
    int rc;
    if (c->wide || c->gen) {
        // 9..64 states: trajectory-parallel kernels on trajectory-major data, no chunk plan
        const size_t esz_w = kind == BHMM_EMIT_GAUSSIAN ? sizeof(double)
                             : kind == BHMM_EMIT_DISCRETE ? sizeof(int32_t)
                                                          : sizeof(double) * (size_t)c->n;
        const size_t bytes_w = (size_t)c->total * esz_w;
        const char *base_w = static_cast<const char *>(obs) + (size_t)offsets[0] * esz_w;
        if ((rc = c->d_obs_rm.ensure(bytes_w)) || (rc = c->d_offsets.ensure(K + 1)))
            return rc;
        BHMM_HIP(hipMemcpyAsync(c->d_obs_rm.p, base_w, bytes_w,
                                obs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                c->stream));
        BHMM_HIP(hipMemcpyAsync(c->d_offsets.p, c->offsets.data(), (K + 1) * sizeof(int64_t),
                                hipMemcpyHostToDevice, c->stream));
        c->G = c->Gp = 0;
        c->Lmax = 0;
        if ((rc = c->gen ? gen_alloc(c) : wide_alloc(c)))
            return rc;
        if ((rc = ensure_pinned(c, (size_t)stats_size(c) + c->K)))
            return rc;
        BHMM_HIP(hipStreamSynchronize(c->stream));
        return BHMM_OK;
    }
    c->ds.chunk_auto = chunk <= 0;
    rc = plan_chunks(c, chunk);
    if (rc)
        return rc;
    if ((rc = alloc_work(c)))
        return rc;

    // bring the trajectory-major observations to the device, then re-lay them out CI
    const size_t esz = kind == BHMM_EMIT_GAUSSIAN ? sizeof(double)
                       : kind == BHMM_EMIT_DISCRETE ? sizeof(int32_t)
                                                    : sizeof(double) * (size_t)c->n;
    const size_t bytes = (size_t)c->total * esz;
    const char *src_dev;
    const char *base = static_cast<const char *>(obs) + (size_t)offsets[0] * esz;
    if (obs_on_device) {
        src_dev = base;
    } else {
        if ((rc = c->d_obs_rm.ensure(bytes)))
            return rc;
        BHMM_HIP(hipMemcpyAsync(c->d_obs_rm.p, base, bytes, hipMemcpyHostToDevice, c->stream));
        src_dev = c->d_obs_rm.p;
    }
    if ((rc = pack_observations(c, src_dev)))
        return rc;
    if (obs_on_device) {
        // keep a trajectory-major copy for the path kernels
        if ((rc = c->d_obs_rm.ensure(bytes)))
            return rc;
        BHMM_HIP(hipMemcpyAsync(c->d_obs_rm.p, src_dev, bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    int32_t has_nan = 0;
    if ((rc = pack_settle(c, &has_nan)))
        return rc;
    if (kind == BHMM_EMIT_GAUSSIAN && has_nan)
        c->ds.careful = true; // gauss_pdf(): the branch-free kernels take NaN for a perfect hit
    return BHMM_OK;
}

// ---- lagged views (bhmm/api.py:70-94) ---------------------------------------------------
namespace bhmm {
// view v, element i  <-  source element src_start[v] + i * lag  (elements of `words` 4-byte words)
static __global__ void k_lag_gather(const uint32_t *src, uint32_t *dst, const int64_t *src_start,
                                    const int64_t *dst_off, int lag, int words, int V)
{
    // gridDim.y is capped (HIP: 65535), so a grid row serves views v, v + gridDim.y, ...
    for (int v = blockIdx.y; v < V; v += gridDim.y) {
        const int64_t len = dst_off[v + 1] - dst_off[v];
        const int64_t s0 = src_start[v], d0 = dst_off[v];
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len;
             i += (int64_t)gridDim.x * blockDim.x) {
            const uint32_t *ps = src + (s0 + i * lag) * words;
            uint32_t *pd = dst + (d0 + i) * words;
            for (int w = 0; w < words; ++w)
                pd[w] = ps[w];
        }
    }
}
} // namespace bhmm

int bhmm_ctx_set_observations_lagged(bhmm_ctx *c, int kind, const void *obs, const int64_t *offsets,
                                     int K, int lag, const int32_t *view_traj,
                                     const int32_t *view_shift, int V, int nstates, int nsymbols,
                                     int chunk, int obs_on_device)
{
    if (!c || !obs || !offsets || K < 1 || !view_traj || !view_shift || V < 1)
        return invalid_arg("bad context / observations / views");
    if (lag < 1)
        return invalid_arg("lag must be >= 1");
    if (kind < 0 || kind > 2 || nstates < 1)
        return invalid_arg("unknown emission kind / nstates");
    BHMM_HIP(hipSetDevice(c->device));
    const size_t esz = kind == BHMM_EMIT_GAUSSIAN ? sizeof(double)
                       : kind == BHMM_EMIT_DISCRETE ? sizeof(int32_t)
                                                    : sizeof(double) * (size_t)nstates;
    std::vector<int64_t> src_start(V), dst_off(V + 1, 0);
    for (int v = 0; v < V; ++v) {
        const int k = view_traj[v], sh = view_shift[v];
        if (k < 0 || k >= K || sh < 0)
            return invalid_arg("view refers to a trajectory / shift that does not exist");
        const int64_t T = offsets[k + 1] - offsets[k];
        const int64_t len = T > sh ? (T - sh + lag - 1) / lag : 0; // len(obs[sh::lag])
        src_start[v] = offsets[k] - offsets[0] + sh;
        dst_off[v + 1] = dst_off[v] + len;
    }
    const int64_t total_src = offsets[K] - offsets[0], total_dst = dst_off[V];
    if (total_dst <= 0)
        return invalid_arg("the views are empty");
    // ONE upload of the original observations; the views are cut on the device
    DevBuf<char> d_src, d_dst;
    DevBuf<int64_t> d_tab;
    int rc;
    if ((rc = d_dst.ensure((size_t)total_dst * esz)) || (rc = d_tab.ensure(2 * (size_t)V + 1)))
        return rc;
    struct Free {
        DevBuf<char> &a, &b;
        DevBuf<int64_t> &t;
        ~Free() { a.release(); b.release(); t.release(); }
    } guard{d_src, d_dst, d_tab};
    const char *src_dev = static_cast<const char *>(obs) + (size_t)offsets[0] * esz;
    if (!obs_on_device) {
        if ((rc = d_src.ensure((size_t)total_src * esz)))
            return rc;
        BHMM_HIP(hipMemcpyAsync(d_src.p, src_dev, (size_t)total_src * esz, hipMemcpyHostToDevice,
                                c->stream));
        src_dev = d_src.p;
    }
    BHMM_HIP(hipMemcpyAsync(d_tab.p, src_start.data(), (size_t)V * sizeof(int64_t),
                            hipMemcpyHostToDevice, c->stream));
    BHMM_HIP(hipMemcpyAsync(d_tab.p + V, dst_off.data(), ((size_t)V + 1) * sizeof(int64_t),
                            hipMemcpyHostToDevice, c->stream));
    // x covers the longest view in 256-element blocks (at most 64 of them, grid-stride beyond),
    // y the views (at most 32768 grid rows, strided beyond): any number of views launches
    int64_t longest = 0;
    for (int v = 0; v < V; ++v)
        longest = std::max(longest, dst_off[v + 1] - dst_off[v]);
    const unsigned gx = (unsigned)std::min<int64_t>(64, (longest + 255) / 256);
    const unsigned gy = (unsigned)std::min(V, 32768);
    BHMM_HIP(launch(k_lag_gather, dim3(gx, gy), dim3(256), 0, c->stream, reinterpret_cast<const uint32_t *>(src_dev),
                    reinterpret_cast<uint32_t *>(d_dst.p), d_tab.p, d_tab.p + V, lag, (int)(esz / 4), V));
    BHMM_HIP(hipStreamSynchronize(c->stream)); // the host tables are temporaries
    return bhmm_ctx_set_observations(c, kind, d_dst.p, dst_off.data(), V, nstates, nsymbols, chunk, 1);
}

int bhmm_diag_gauss_pdf(double *y, const double *o, int64_t n, double mu, double sigma,
                        int nansafe)
{
    if (!y || !o || n < 0)
        return invalid_arg("bhmm_diag_gauss_pdf: bad arguments");
    Model<2> m;
    const double A[1] = {1.0}, pi[1] = {1.0};
    fill_model<2>(m, 1, EMIT_GAUSS, 0, A, pi, &mu, &sigma);
    double *dx = nullptr, *dy = nullptr;
    hipError_t e = hipMalloc(&dx, n * sizeof(double));
    if (e == hipSuccess)
        e = hipMalloc(&dy, n * sizeof(double));
    if (e == hipSuccess)
        e = hipMemcpy(dx, o, n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = launch(k_gauss_pdf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dy, n, m.e0[0], m.e4[0],
                   m.e5[0], m.emg, nansafe);
    if (e == hipSuccess)
        e = hipMemcpy(y, dy, n * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(dx);
    (void)hipFree(dy);
    return e == hipSuccess ? BHMM_OK : hip_fail(e, "bhmm_diag_gauss_pdf");
}

int bhmm_diag_exp_nonpos(double *y, const double *x, int64_t n)
{
    if (!y || !x || n < 1)
        return invalid_arg("NULL argument or empty problem");
    double *dx = nullptr, *dy = nullptr;
    BHMM_HIP(hipMalloc(reinterpret_cast<void **>(&dx), (size_t)n * sizeof(double)));
    if (hipMalloc(reinterpret_cast<void **>(&dy), (size_t)n * sizeof(double)) != hipSuccess) {
        (void)hipFree(dx);
        return hip_fail(hipErrorOutOfMemory, "hipMalloc");
    }
    hipError_t e = hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = launch(k_exp_nonpos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dy, n);
    if (e == hipSuccess)
        e = hipMemcpy(y, dy, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(dx);
    (void)hipFree(dy);
    return e == hipSuccess ? BHMM_OK : hip_fail(e, "bhmm_diag_exp_nonpos");
}

int bhmm_ctx_set_option(bhmm_ctx *c, const char *name, double value)
{
    if (!c || !name)
        return invalid_arg("NULL argument");
    const std::string n(name);
    if (n == "spec_enabled") {
        c->opt.spec_enabled = value != 0.0;
        c->ds.carry_valid = false; // (an E-step outside the verified split path leaves no vectors to carry)
    } else if (n == "carry") { // warm-ups from the previous E-step's boundary vectors (EM sequences)
        c->opt.carry_enabled = value != 0.0;
        c->ds.carry_valid = false;
    } else if (n == "obs16") {
        // discrete kind, up to 8 states: 0 keeps the split E-step on the int32 observations (same statistics, bit
        // for bit; tests).  Takes effect at the next E-step; switching it back on needs new observations if they
        // were loaded while it was off (the 16-bit copy is made with them).
        c->opt.obs16_enabled = value != 0.0;
    } else if (n == "carry_kappa") { // (tests: the sensitivity bound that sizes the carried warm-ups)
        c->ds.carry_kappa = value;
    } else if (n == "spec_tol") {
        // N <= 8: componentwise relative tolerance of the boundary check of the time-split E-step (and
        // what the warm-up is calibrated for, a hundred times inside it).  Default 1e-11; the parity
        // contract is 1e-6, so 1e-9 still leaves three decades -- and shortens the warm-ups by a sixth.
        if (!(value >= 1e-13 && value <= 1e-7))
            return invalid_arg("spec_tol outside [1e-13, 1e-7]");
        c->opt.spec_tol = value;
        c->ds.spec_calibrated = c->opt.spec_W_fixed; // (the next E-step measures the warm-up for it)
        c->ds.carry_valid = false;
    } else if (n == "sample_seg_per_simd") { // 9..64 states: segments per SIMD of the backward draw
        if (value < 1 || value > 64)
            return BHMM_ERR_INVALID;
        c->opt.smp_seg_per_simd = (int)value;
        c->ds.pplan[1].nseg = 0;
    } else if (n == "viterbi_seg_warmups") { // 9..64 states: a Viterbi segment is at least this many warm-ups long
        if (value < 1 || value > 64)
            return BHMM_ERR_INVALID;
        c->opt.vit_seg_warmups = (int)value;
        c->ds.pplan[0].nseg = 0;
    } else if (n == "viterbi_W") { // warm-up of the next segment-parallel Viterbi pass (0: from the E-step's)
        if (value < 0 || value > (1 << 20))
            return BHMM_ERR_INVALID;
        c->ds.vit.W = (int)value;
    } else if (n == "viterbi_margin") { // 9..128 states: the path-margin acceptance of the segment-parallel first pass
        c->opt.vit_margin = value != 0.0;
        if (value == 2.0) // (up to 64 states: from the next call on, not only after a call with two or more rounds)
            c->ds.vit.margin_want = true;
    } else if (n == "viterbi_mend") { // 9..64 states: segments further than 1e-12 from their predecessors run again alone
        c->opt.vit_mend = value != 0.0;
    } else if (n == "viterbi_seg_per_simd") { // 9..64 states: segments per SIMD of the Viterbi pass
        if (value < 1 || value > 64)
            return BHMM_ERR_INVALID;
        c->opt.vit_seg_per_simd = (int)value;
        c->ds.pplan[0].nseg = 0;
        c->ds.vit.seg_given_up = false;
    } else if (n == "f32_tol") { // BHMM_FLAG_SINGLE: relative tolerance of the fp32 boundary check
        if (!(value >= 1e-7 && value <= 1e-3))
            return invalid_arg("f32_tol outside [1e-7, 1e-3]");
        c->opt.f32_tol = value;
        c->ds.f32_W = 0; // (the next fp32 E-step measures the warm-up for it)
    } else if (n == "f32_W") { // BHMM_FLAG_SINGLE: fixed fp32 warm-up length (0: measured)
        if (!(value >= 0 && value <= (1 << 20)))
            return invalid_arg("f32_W outside [0, 2^20]");
        c->opt.f32_W = (int)value;
    } else if (n == "spec_W") {
        c->ds.carry_valid = false;
        c->ds.spec_W = std::max(1, (int)value);
        c->ds.vit.W = 0;
        c->opt.spec_W_fixed = c->ds.spec_calibrated = true; // the caller's choice: no probe
    }
    else if (n == "draw_watch") // draws inside the reach of the alpha rows' verified deviation are decided again (draw_verify.hpp)
        c->opt.draw_watch = value != 0.0;
    else if (n == "draw_watch_tol") { // (tests) watch tolerance instead of 64 x the measured deviation; 0: automatic
        if (!(value >= 0.0 && value <= 0.5))
            return invalid_arg("draw_watch_tol outside [0, 0.5]");
        c->opt.draw_watch_tol = value;
    } else if (n == "draw_test_redo") // (tests) every watched draw counts as a decision that did not stand
        c->opt.draw_test_redo = value != 0.0;
    else if (n == "wide_segments")
        c->opt.wseg_enabled = value != 0.0;
    else if (n == "wide_segment_len")
        c->opt.wseg_len = std::max(0, (int)value); // takes effect at the next set_observations
    else if (n == "wide_split")
        c->opt.wseg_split = value != 0.0; // 64 states: own, finer segment plan for the forward pass
    else if (n == "tile")
        c->opt.tile_enabled = value != 0.0; // row-batched matrix-core recursions (next set_observations)
    else if (n == "tile_per_cu")
        c->opt.tile_per_cu = std::max(1, std::min(4, (int)value)); // (next set_observations)
    else if (n == "score_W") // bhmm_score only: fixed warm-up (0: measured per model); no E-step state changes
        c->opt.score_W = std::max(0, (int)value);
    else if (n == "score_layout") { // bhmm_score, N <= 8: 1 = one lane per chunk, 2 = N/2 lanes per chunk
        if (value != 1.0 && value != 2.0)
            return invalid_arg("score_layout must be 1 or 2");
        c->opt.score_layout = (int)value;
    } else if (n == "score_seglen") { // bhmm_score, 9..128 states: segment length of its plan from the next call on (0: automatic)
        if (!(value >= 0 && value <= (1 << 30)))
            return invalid_arg("score_seglen outside [0, 2^30]");
        c->opt.score_seglen = ((int)value + 3) & ~3;
    } else if (n == "score_lazy") // ... first pass on the lazily scaled kernel (default) or summing every step
        c->opt.score_lazy = value != 0.0;
    else if (n == "post_W") // bhmm_posterior_decode only: fixed warm-up (0: measured); no E-step state changes
        c->opt.post_W = std::max(0, (int)value);
    else if (n == "post_ws_mb") { // ... budget of its alpha-row workspace in MiB (0: unbounded)
        if (!(value >= 0.0) || value > (double)(1 << 30))
            return invalid_arg("post_ws_mb outside [0, 2^30]");
        c->opt.post_ws_mb = (int)value;
    } else if (n == "marg_W") // bhmm_posterior_marginals only: fixed warm-up (0: measured); no E-step state changes
        c->opt.marg_W = std::max(0, (int)value);
    else if (n == "marg_ws_mb") { // ... budget of its alpha-row workspace in MiB (0: unbounded)
        if (!(value >= 0.0) || value > (double)(1 << 30))
            return invalid_arg("marg_ws_mb outside [0, 2^30]");
        c->opt.marg_ws_mb = (int)value;
    } else if (n == "pair_W") // bhmm_posterior_transitions only: fixed warm-up (0: measured); no E-step state changes
        c->opt.pair_W = std::max(0, (int)value);
    else if (n == "pair_ws_mb") { // ... budget of its alpha-row workspace in MiB (0: unbounded)
        if (!(value >= 0.0) || value > (double)(1 << 30))
            return invalid_arg("pair_ws_mb outside [0, 2^30]");
        c->opt.pair_ws_mb = (int)value;
    } else if (n == "pair_fused") // ... 0: never the fused path (the generic route answers every call)
        c->opt.pair_fused = value != 0.0;
    else if (n == "pair_rows") { // ... row kernel of the generic path: 0 k_pair_rows, 1 k_pair_tile (n <= 128), -1 by class
        if (value != -1.0 && value != 0.0 && value != 1.0)
            return invalid_arg("pair_rows is -1, 0 or 1");
        c->opt.pair_rows = (int)value;
    } else if (n == "filter_W") // bhmm_filter only: fixed warm-up (0: measured); no E-step state changes
        c->opt.filter_W = std::max(0, (int)value);
    else if (n == "filter_seglen") { // ... 9..64 states: segment length of its plan from the next call on (0: automatic)
        if (!(value >= 0 && value <= (1 << 30)))
            return invalid_arg("filter_seglen outside [0, 2^30]");
        c->opt.filter_seglen = ((int)value + 3) & ~3;
    } else if (n == "filter_parallel") { // ... the time-parallel path: 0 never, 1 always when eligible, -1 automatic
        if (value != 0.0 && value != 1.0 && value != -1.0)
            return invalid_arg("filter_parallel must be -1, 0 or 1");
        c->opt.filter_parallel = (int)value;
    } else if (n == "filter_tile") { // ... 65..128 states, the matrix-core path: 0 never, 1 always when eligible, -1 automatic
        if (value != 0.0 && value != 1.0 && value != -1.0)
            return invalid_arg("filter_tile must be -1, 0 or 1");
        c->opt.filter_tile = (int)value;
    } else if (n == "smooth_wide") { // posterior calls, 9..64 states: the time-segmented path: 0 never, 1 always when eligible, -1 automatic
        if (value != 0.0 && value != 1.0 && value != -1.0)
            return invalid_arg("smooth_wide must be -1, 0 or 1");
        c->opt.smooth_wide = (int)value;
    } else if (n == "smooth_tile") { // ... 65..128 states, the matrix-core path: 0 never, 1 always when eligible, -1 automatic
        if (value != -1 && value != 0 && value != 1)
            return invalid_arg("smooth_tile must be -1, 0 or 1");
        c->opt.smooth_tile = (int)value;
    } else if (n == "smooth_seglen") { // ... segment length of its plan from the next call on (0: automatic)
        if (!(value >= 0 && value <= (1 << 30)))
            return invalid_arg("smooth_seglen outside [0, 2^30]");
        c->opt.smooth_seglen = ((int)value + 3) & ~3;
    } else if (n == "smooth_W") // ... fixed warm-up (0: measured); no E-step state changes
        c->opt.smooth_W = std::max(0, (int)std::min(value, (double)(1 << 30)));
    else if (n == "smooth_ws_mb") { // ... budget of its alpha-row workspace in MiB (0: unbounded)
        if (!(value >= 0.0) || value > (double)(1 << 30))
            return invalid_arg("smooth_ws_mb outside [0, 2^30]");
        c->opt.smooth_ws_mb = (int)value;
    } else
        return invalid_arg("unknown or read-only option: " + n);
    return BHMM_OK;
}

int bhmm_ctx_get_option(bhmm_ctx *c, const char *name, double *value)
{
    if (!c || !name || !value)
        return invalid_arg("NULL argument");
    const std::string n(name);
    if (n == "spec_enabled")
        *value = c->opt.spec_enabled ? 1.0 : 0.0;
    else if (n == "spec_W")
        *value = c->ds.spec_W;
    else if (n == "spec_tol")
        *value = c->opt.spec_tol;
    else if (n == "spec_ok")
        *value = c->last.spec_ok;
    else if (n == "spec_fail")
        *value = c->last.spec_fail;
    else if (n == "spec_last_dev")
        *value = c->last.spec_last_dev;
    else if (n == "f32_used")
        *value = c->last.f32_used ? 1.0 : 0.0;
    else if (n == "f32_fallbacks")
        *value = c->last.f32_fallbacks;
    else if (n == "f32_tol")
        *value = c->opt.f32_tol;
    else if (n == "f32_W")
        *value = c->opt.f32_W > 0 ? c->opt.f32_W : c->ds.f32_W;
    else if (n == "f32_last_dev")
        *value = c->last.f32_last_dev;
    else if (n == "careful")
        *value = (c->ds.careful || c->ds.wide_careful) ? 1.0 : 0.0;
    else if (n == "viterbi_chunked")
        *value = c->last.viterbi_chunked ? 1.0 : 0.0;
    else if (n == "viterbi_close")
        *value = c->last.viterbi_close;
    else if (n == "viterbi_W") // warm-up the chunk-parallel Viterbi last verified with
        *value = c->ds.vit.W;
    else if (n == "viterbi_segments") // 9..64 states: time segments of the last Viterbi pass's plan
        *value = c->ds.pplan[0].nseg;
    else if (n == "sample_segmented") // 9..64 states: the last path sampling ran over time segments
        *value = c->last.smp_segmented ? 1.0 : 0.0;
    else if (n == "sample_forward_segmented")
        *value = c->last.draw_fwd_segmented ? 1.0 : 0.0;
    else if (n == "sample_segments")
        *value = c->ds.pplan[1].nseg;
    else if (n == "sample_W")
        *value = c->ds.smp_W;
    else if (n == "sample_mismatch") // ... segments its first pass left to the fix-up rounds
        *value = c->last.smp_seg_mismatch;
    else if (n == "sample_rounds")
        *value = c->last.smp_seg_rounds;
    else if (n == "viterbi_rounds") // ... fix-up rounds its last pass needed
        *value = c->last.vit_seg_rounds;
    else if (n == "viterbi_mismatch") // ... boundaries of its last attempt that were not bit-identical
        *value = c->last.vit_seg_mismatch;
    else if (n == "viterbi_margin")
        *value = c->opt.vit_margin ? 1.0 : 0.0;
    else if (n == "viterbi_mended") // ... segments its last call ran again up to a kept vector of the first pass
        *value = c->last.vit_mended;
    else if (n == "viterbi_far") // ... boundaries of its first pass that were not equal to 1e-12
        *value = c->last.vit_far;
    else if (n == "viterbi_margin_used") // ... accepted by the margins of the decisions on its path (no fix-up rounds)
        *value = c->last.vit_margin_used;
    else if (n == "viterbi_margin_close") // ... segments with a close decision on the path (the rounds ran instead)
        *value = c->last.vit_margin_close;
    else if (n == "draw_watch")
        *value = c->opt.draw_watch ? 1.0 : 0.0;
    else if (n == "draw_events") // last path sampling: draws inside the watch tolerance
        *value = c->last.draw_events;
    else if (n == "draw_checked") // ... of them decided again on the windowed serial recursion
        *value = c->last.draw_checked;
    else if (n == "draw_redone") // ... the call was repeated on the exact alpha rows
        *value = c->last.draw_redone;
    else if (n == "draw_alpha_dev") // ... largest boundary deviation of the forward pass the draws read
        *value = c->last.draw_alpha_dev;
    else if (n == "carry")
        *value = c->opt.carry_enabled ? 1.0 : 0.0;
    else if (n == "obs16")
        *value = c->opt.obs16_enabled ? 1.0 : 0.0;
    else if (n == "obs16_used") // the sweeps of the last E-step read the 16-bit copy of the observations
        *value = c->last.obs16_used ? 1.0 : 0.0;
    else if (n == "carry_W") // warm-up steps of the last E-step's carried starts (0: full warm-ups)
        *value = c->last.carry_last_W;
    else if (n == "carry_cap") // where the last E-step's backward sweep was split for the capture (0: not split)
        *value = c->ds.carry_cap;
    else if (n == "carry_ok")
        *value = c->last.carry_ok;
    else if (n == "carry_fail")
        *value = c->last.carry_fail;
    else if (n == "carry_kappa")
        *value = c->ds.carry_kappa;
    else if (n == "wide_segments")
        *value = (c->opt.wseg_enabled && !c->ds.wseg_given_up && c->w_nseg[1] > c->w_nseg[0]) ? c->w_nseg[1] : 0;
    else if (n == "wide_segment_len") // segment length of the current time-segmented plan (0: none)
        *value = (c->opt.wseg_enabled && !c->ds.wseg_given_up && c->w_nseg[1] > c->w_nseg[0]) ? (double)c->wseg_cur_len : 0.0;
    else if (n == "wide_trouble") // which self-check of the lazily scaled kernels fired last (bit mask)
        *value = c->last.wide_trouble;
    else if (n == "tile_reason") // more than 64 states: why the tile kernels were left (ctx.hpp), 0: they were not
        *value = c->tile_reason;
    else if (n == "tile") // 1: the last E-step ran on the row-batched matrix-core kernels
        *value = c->last.tile_used ? 1.0 : 0.0;
    else if (n == "wide_fwd_segments") // the forward pass's own, finer plan (64 states), 0 if none
        *value = (c->opt.wseg_enabled && !c->ds.wseg_given_up && c->w_nseg[1] > c->w_nseg[0] &&
                  c->w_nseg[2] > c->w_nseg[1]) ? c->w_nseg[2] : 0;
    else if (n == "score_W")
        *value = c->opt.score_W;
    else if (n == "score_layout")
        *value = c->opt.score_layout;
    else if (n == "score_fallbacks") // bhmm_score: models whose boundaries did not verify at the first warm-up
        *value = c->last.score_fallbacks;
    else if (n == "score_seglen")
        *value = c->opt.score_seglen;
    else if (n == "score_lazy")
        *value = c->opt.score_lazy ? 1.0 : 0.0;
    else if (n == "score_segments") // ... segments of the score plan the last call ran on (0: the serial kernel, N <= 8)
        *value = c->last.score_segments;
    else if (n == "score_W_max") // ... longest warm-up of its first pass at 9..128 states (0: no boundary, other paths)
        *value = c->last.score_W_max;
    else if (n == "post_W")
        *value = c->opt.post_W;
    else if (n == "post_ws_mb")
        *value = c->opt.post_ws_mb;
    else if (n == "post_fallbacks") // bhmm_posterior_decode: calls whose boundaries did not verify at the first warm-up
        *value = c->last.post_fallbacks;
    else if (n == "post_path") // ... first pass of the last call: 2 time segments (9..64 states), 1 fused kernel (up to 8 states), 0 E-step + gamma rows
        *value = c->last.post_path;
    else if (n == "marg_W")
        *value = c->opt.marg_W;
    else if (n == "marg_ws_mb")
        *value = c->opt.marg_ws_mb;
    else if (n == "marg_fallbacks") // bhmm_posterior_marginals: calls whose boundaries did not verify at the first warm-up
        *value = c->last.marg_fallbacks;
    else if (n == "marg_path") // ... first pass of the last call: 2 time segments (9..64 states), 1 fused kernel (up to 8 states), 0 E-step + gamma rows
        *value = c->last.marg_path;
    else if (n == "pair_W")
        *value = c->opt.pair_W;
    else if (n == "pair_ws_mb")
        *value = c->opt.pair_ws_mb;
    else if (n == "pair_fused")
        *value = c->opt.pair_fused ? 1.0 : 0.0;
    else if (n == "pair_rows")
        *value = c->opt.pair_rows;
    else if (n == "pair_fallbacks") // bhmm_posterior_transitions: calls whose boundaries did not verify at the first warm-up
        *value = c->last.pair_fallbacks;
    else if (n == "pair_path") // ... first pass of the last call: 1 fused kernel, 0 filter + marginals + pair rows
        *value = c->last.pair_path;
    else if (n == "pair_rows_kernel") // ... row kernel of the last generic pass: 0 k_pair_rows, 1 k_pair_tile
        *value = c->last.pair_rows_kernel;
    else if (n == "filter_W")
        *value = c->opt.filter_W;
    else if (n == "filter_fallbacks") // bhmm_filter: calls whose boundaries did not verify at the first warm-up
        *value = c->last.filter_fallbacks;
    else if (n == "filter_path") // ... first pass of the last call: 3 k_filter_tile (65..128 states), 2 k_filter_wide (9..64 states), 1 fused kernel (up to 8 states), 0 serial kernel
        *value = c->last.filter_path;
    else if (n == "filter_seglen")
        *value = c->opt.filter_seglen;
    else if (n == "filter_parallel")
        *value = c->opt.filter_parallel;
    else if (n == "filter_segments") // ... segments of the filter plan the last call ran on (0: another path)
        *value = c->last.filter_segments;
    else if (n == "filter_wide_min_total") // ... steps from which filter_parallel = -1 takes the time-parallel path
        *value = (double)FILTER_WIDE_MIN_TOTAL;
    else if (n == "filter_tile")
        *value = c->opt.filter_tile;
    else if (n == "filter_tile_min_total") // ... steps from which filter_tile = -1 takes the matrix-core path (65..128 states)
        *value = (double)FILTER_TILE_MIN_TOTAL;
    else if (n == "filter_redone") // ... trajectories of the last call that path did again on the serial kernel
        *value = c->last.filter_redone;
    else if (n == "smooth_wide")
        *value = c->opt.smooth_wide;
    else if (n == "smooth_tile")
        *value = c->opt.smooth_tile;
    else if (n == "smooth_tile_min_total") // ... steps below which smooth_tile = -1 never takes the matrix-core path (65..128 states)
        *value = (double)SMOOTH_TILE_MIN_TOTAL;
    else if (n == "smooth_seglen")
        *value = c->opt.smooth_seglen;
    else if (n == "smooth_W")
        *value = c->opt.smooth_W;
    else if (n == "smooth_ws_mb")
        *value = c->opt.smooth_ws_mb;
    else if (n == "smooth_segments") // posterior calls: segments of the smoothing plan the last call ran on (0: another path)
        *value = c->last.smooth_segments;
    else if (n == "smooth_wide_min_total") // ... steps below which smooth_wide = -1 never takes the time-segmented path
        *value = (double)SMOOTH_WIDE_MIN_TOTAL;
    else if (n == "score_path") // ... first pass of the last call: 0 serial kernel, 1 chunk kernels (N <= 8), 2 k_score_wide, 3 k_score_tile
        *value = c->last.score_path;
    else if (n == "runs_tile") // bhmm_path_runs / bhmm_decode_runs: steps of the path per workgroup
        *value = runs::TILE;
    else if (n == "runs_lane") // ... per lane
        *value = runs::LANE;
    else if (n == "runs_count") // ... runs of the last call on these observations
        *value = (double)c->ds.runs_count;
    else if (n == "runs_ms") // ... device time of its count, scan and scatter passes
        *value = c->last.runs_ms;
    else if (n == "pathlp_tile") // bhmm_path_logprob / bhmm_decode_logprob: steps of the path per workgroup
        *value = runs::TILE;
    else if (n == "pathlp_lane") // ... consecutive steps per lane
        *value = runs::LANE;
    else if (n == "pathlp_table") // ... 1: the last call kept the log-transition table in LDS, 0: it read it through L2
        *value = c->last.pathlp_table;
    else if (n == "pathlp_ms") // ... device time of the last call's prepare, tile and finish passes
        *value = c->last.pathlp_ms;
    else if (n == "mvn_rows_ms") // multivariate gaussian emissions: device time of the last k_mvn_rows + k_mvn_shift
        *value = c->mvn.rows_ms;
    else if (n == "mvn_reload_ms") // ... host time of the explicit re-load that followed them
        *value = c->mvn.reload_ms;
    else if (n == "mvn_moments_ms") // ... device time of the last k_mvn_moments + k_mvn_moments_finish
        *value = c->mvn.moments_ms;
    else if (n == "gmm_weights_ms") // gaussian-mixture emissions: device time of the last k_gmm_weights
        *value = c->gmm.weights_ms;
    else if (n == "gmm_draw_ms") // ... device time of the last k_gmm_draw_components
        *value = c->gmm.draw_ms;
    else if (n == "mvn_path_moments_ms") // ... device time of the last k_mvn_path_moments + k_mvn_moments_finish
        *value = c->mvn.path_moments_ms;
    else
        return invalid_arg("unknown option: " + n);
    return BHMM_OK;
}

int bhmm_ctx_stats_size(const bhmm_ctx *c) { return (c && c->kind >= 0) ? stats_size(c) : 0; }
int64_t bhmm_ctx_total_steps(const bhmm_ctx *c) { return c ? c->total : 0; }
int bhmm_ctx_num_chunks(const bhmm_ctx *c) { return c ? c->G : 0; }
int bhmm_ctx_chunk_len(const bhmm_ctx *c) { return c ? c->Lmax : 0; }
void *bhmm_ctx_stream(bhmm_ctx *c) { return c ? (void *)c->stream : nullptr; }

int bhmm_ctx_sync(bhmm_ctx *c)
{
    if (!c)
        return invalid_arg("ctx == NULL");
    BHMM_HIP(hipSetDevice(c->device));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    collect_timing(c);
    return BHMM_OK;
}

double bhmm_ctx_last_kernel_ms(bhmm_ctx *c, int which)
{
    if (!c || which < 0 || which > 4)
        return -1.0;
    return c->last.ms[which];
}

int bhmm_ctx_last_kernel_ms_all(bhmm_ctx *c, double *out)
{
    if (!c || !out)
        return invalid_arg("bad arguments");
    for (int i = 0; i < 5; ++i)
        out[i] = c->last.ms[i];
    return BHMM_OK;
}

// Safety net for the one situation in which a chunked evaluation cannot follow the reference
// (reducible transition matrices whose blocks' relative weight leaves the double
// range -- the reference's result depends on the order in which ITS recursions lose a block): finite
// log-likelihoods but non-finite counts.  The observations are re-planned with one chunk per
// trajectory -- the plain sequential recursions -- and the E-step is repeated with the model of the
// last bhmm_estep call (kept in the context) into the same statistics buffer, once per set of
// observations.  *retried (optional) reports whether that happened.
static int nonfinite_retry(bhmm_ctx *c, bool *retried)
{
    if (retried)
        *retried = false;
    if (c->wide || c->gen || c->G <= c->K || c->ds.serial_retry_done || !c->last_stats)
        return BHMM_OK;
    const int S = stats_size(c);
    const int n = c->n;
    const int ncheck = std::min(S, 1 + n + n * n + n);
    if (!c->prefetched) {
        BHMM_HIP(hipMemcpyAsync(c->h_pinned, c->last_stats, S * sizeof(double), hipMemcpyDeviceToHost,
                                c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
    }
    bool finite = true;
    for (int e = 0; e < ncheck; ++e)
        finite = finite && std::isfinite(c->h_pinned[e]);
    const int64_t maxT = longest_traj(c);
    if (finite || !std::isfinite(c->h_pinned[0]) || maxT >= ((int64_t)1 << 30))
        return BHMM_OK;
    c->ds.serial_retry_done = true;
    // does the one-chunk-per-trajectory plan fit?  Its workspace is (K padded to 64) x maxT records (few
    // long trajectories: hundreds of GB): if not, leave the plan alone -- the fetch then reports the
    // non-finite statistic instead of an allocation failure on a half-replaced plan
    const double recs = (double)((c->K + 63) / 64) * (double)maxT * 64.0;
    const double need = recs * ((double)c->N * 8.0 * 1.5 + 16.0);
    size_t free_b = 0, total_b = 0;
    BHMM_HIP(hipMemGetInfo(&free_b, &total_b));
    const double held = (double)c->d_ws.n * 8.0 + (double)c->d_obs_ci.n + (double)c->d_gamma_ci.n * 8.0;
    const size_t ne = c->kind == BHMM_EMIT_GAUSSIAN ? 2 * (size_t)n
                      : (c->kind == BHMM_EMIT_DISCRETE ? (size_t)n * c->M : 0);
    if (need > 0.9 * ((double)free_b + held) || c->ds.prev_model.size() != (size_t)n * n + ne ||
        c->last_pi.size() != (size_t)n)
        return BHMM_OK;
    c->ds.chunk_auto = false;
    c->gamma_wanted = (c->last_flags & BHMM_FLAG_STORE_GAMMA) != 0; // (the re-plan re-sizes the gamma rows)
    int rc;
    if ((rc = replan_coarse(c, false, (int)maxT))) {
        c->kind = -1; // (a failed re-plan leaves no usable plan: the context needs new observations)
        return rc;
    }
    c->prefetched = false;
    const double *A = c->ds.prev_model.data();
    const double *p0 = ne ? A + (size_t)n * n : nullptr;
    const double *p1 = c->kind == BHMM_EMIT_GAUSSIAN ? p0 + n : nullptr;
    if (retried)
        *retried = true;
    return BHMM_DISPATCH_N(c, estep(c, A, c->last_pi.data(), p0, p1, c->last_stats, c->last_flags));
}

extern "C++" {
int bhmm::enter_model_call(bhmm_ctx *c, bool given, const char *null_msg, bool emissions, const double *par0,
                           const double *par1)
{
    if (c)
        lds_poison(c->stream); // (debugging aid, BHMM_AMD_POISON=1 only)
    if (!c || c->kind < 0)
        return invalid_arg("no observations loaded");
    if (!given)
        return invalid_arg(null_msg);
    if (emissions && c->kind == BHMM_EMIT_GAUSSIAN && (!par0 || !par1))
        return invalid_arg("gaussian emissions need means and sigmas");
    if (emissions && c->kind == BHMM_EMIT_DISCRETE && !par0)
        return invalid_arg("discrete emissions need B");
    BHMM_HIP(hipSetDevice(c->device));
    return BHMM_OK;
}
} // extern "C++"

int bhmm_estep(bhmm_ctx *c, const double *A, const double *pi, const double *par0,
               const double *par1, double *stats_dev, int flags)
{
    int rc = enter_model_call(c, A && pi, "A / pi == NULL", true, par0, par1);
    if (rc)
        return rc;
    if (!c->wide && !c->gen && c->kind == BHMM_EMIT_DISCRETE && (rc = upload_Bt(c, par0)))
        return rc;
    if (!c->wide && !c->gen && (flags & BHMM_FLAG_STORE_GAMMA)) {
        if ((rc = c->d_gamma_ci.ensure((size_t)ci_records(c) * c->N * 64)))
            return rc;
    }
    c->ds.gamma_valid = false;
    c->gamma_wanted = (flags & BHMM_FLAG_STORE_GAMMA) != 0;
    c->wide_retry = 0;
    {
        // how far the model moved since the previous E-step on these observations (max norm;
        // emission parameters in units of sigma): sizes the warm-ups from carried boundary vectors
        const int n = c->n;
        const size_t ne = c->kind == BHMM_EMIT_GAUSSIAN ? 2 * (size_t)n
                          : (c->kind == BHMM_EMIT_DISCRETE ? (size_t)n * c->M : 0);
        std::vector<double> cur((size_t)n * n + ne);
        memcpy(cur.data(), A, (size_t)n * n * sizeof(double));
        if (c->kind == BHMM_EMIT_GAUSSIAN) {
            memcpy(cur.data() + (size_t)n * n, par0, n * sizeof(double));
            memcpy(cur.data() + (size_t)n * n + n, par1, n * sizeof(double));
        } else if (c->kind == BHMM_EMIT_DISCRETE) {
            memcpy(cur.data() + (size_t)n * n, par0, ne * sizeof(double));
        }
        double delta = -1.0;
        if (c->ds.prev_model.size() == cur.size()) {
            delta = 0.0;
            for (size_t e = 0; e < cur.size(); ++e) {
                double d = fabs(cur[e] - c->ds.prev_model[e]);
                if (c->kind == BHMM_EMIT_GAUSSIAN && e >= (size_t)n * n)
                    d /= fabs(par1[(e - (size_t)n * n) % n]);
                if (!(d <= delta))
                    delta = d == d ? d : 1e300;
            }
        }
        c->carry_delta = delta;
        c->ds.prev_model.swap(cur);
        c->last_pi.assign(pi, pi + n); // (with prev_model: the model of this call, for nonfinite_retry)
        c->last_flags = flags;
    }
    double *sd = stats_dev ? stats_dev : c->d_stats.p;
    c->last_stats_internal = (stats_dev == nullptr);
    c->last_stats_checked = false;
    c->last_stats = sd;
    c->prefetched = false;
    c->ev_lean = false;
    // BHMM_FLAG_SINGLE: the fp32 kernels where they apply and verify (estep_f32.hip), else this fp64 path
    bool single_done = false;
    c->last.f32_used = false;
    c->last.obs16_used = false; // (set by the split launches of the discrete kind, Runner::fwdbwd)
    if ((flags & BHMM_FLAG_SINGLE) && (rc = estep_f32(c, A, pi, par0, par1, sd, flags, &single_done)))
        return rc;
    if (flags & BHMM_FLAG_SINGLE) {
        c->last.f32_used = single_done;
        c->last.f32_fallbacks += single_done ? 0 : 1;
    }
    if (single_done)
        rc = BHMM_OK;
    else if (c->gen)
        rc = gen_estep(c, A, pi, par0, par1, sd, flags);
    else if (c->wide)
        rc = wide_estep(c, A, pi, par0, par1, sd, flags);
    else
        rc = BHMM_DISPATCH_N(c, estep(c, A, pi, par0, par1, sd, flags));
    if (rc == BHMM_OK && (c->prefetched || c->last_stats_internal))
        // (the statistics are on the host already, or are the library's own and fetched next anyway: look
        // now.  An E-step launched into a CALLER's device buffer stays asynchronous; bhmm_estep_fetch, which
        // such a caller uses to wait for it, takes the same look -- so a sharded caller is repaired too,
        // BEFORE its all-reduce)
        rc = nonfinite_retry(c, nullptr);
    c->ds.gamma_valid = rc == BHMM_OK && c->gamma_wanted;
    c->gamma_wanted = false;
    return rc;
}

int bhmm_estep_fetch(bhmm_ctx *c, double *stats, double *logL_k)
{
    if (!c || c->kind < 0)
        return invalid_arg("no observations loaded");
    BHMM_HIP(hipSetDevice(c->device));
    const int S = stats_size(c);
    // statistics come from the buffer the E-step wrote (the caller's, if it gave one: a caller that
    // all-reduces that buffer in place fetches before reducing, or asks for logL_k only)
    bool have_logLk = true;
    if (!c->prefetched && !c->last_stats)
        return invalid_arg("no E-step has run on these observations");
    if (!c->last_stats_internal && !c->last_stats_checked) {
        // an E-step launched into the caller's buffer: the FIRST fetch after the launch is where this rank's
        // result is looked at (and, if the counts are not finite, repaired in place) -- once per launch, so a
        // later fetch never inspects what an in-place all-reduce has made of the buffer since.  The header's
        // contract: fetch (statistics or logL_k only, as the sharded estimators do) BEFORE reducing.
        c->last_stats_checked = true;
        bool retried = false;
        int rc = nonfinite_retry(c, &retried);
        if (retried) { // (what bhmm_estep does at its end)
            c->ds.gamma_valid = rc == BHMM_OK && c->gamma_wanted;
            c->gamma_wanted = false;
        }
        if (rc)
            return rc;
    }
    if (!c->prefetched) {
        BHMM_HIP(hipMemcpyAsync(c->h_pinned, c->last_stats, S * sizeof(double), hipMemcpyDeviceToHost,
                                c->stream));
        BHMM_HIP(hipMemcpyAsync(c->h_pinned + S, c->d_logLk.p, c->K * sizeof(double),
                                hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
    } else {
        have_logLk = c->logLk_prefetched;
    }
    c->prefetched = false;
    collect_timing(c);
    if (stats)
        memcpy(stats, c->h_pinned, S * sizeof(double));
    // a non-finite trajectory makes the total non-finite: look for it only then (K can be 1e6)
    const bool scan = !std::isfinite(c->h_pinned[0]);
    if (!have_logLk && (logL_k || scan)) {
        BHMM_HIP(hipMemcpyAsync(c->h_pinned + S, c->d_logLk.p, c->K * sizeof(double),
                                hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
    }
    if (logL_k)
        memcpy(logL_k, c->h_pinned + S, c->K * sizeof(double));
    if (!scan) {
        // finite log-likelihoods but a non-finite statistic: fail loudly rather than hand NaN counts
        // to an M-step.  Known to happen only for reducible transition matrices (A = I) with
        // emission probabilities hundreds of decades apart, where the blocks' likelihood ratio
        // leaves the double range inside one chunk and the transfer matrices of the exact pipeline
        // (one exponent per matrix) lose a block.
        // (log-likelihood, sum gamma_0, counts, sum gamma -- not the emission sums: an infinite
        // observation that the outlier rule lets through makes those infinite in the reference too)
        const int ncheck = std::min(S, 1 + c->n + c->n * c->n + c->n);
        for (int e = 0; e < ncheck; ++e)
            if (!std::isfinite(c->h_pinned[e])) {
                g_err = "sufficient statistic " + std::to_string(e) + " of the E-step is not finite";
                return BHMM_ERR_NONFINITE;
            }
    }
    if (scan)
    for (int k = 0; k < c->K; ++k)
        if (!std::isfinite(c->h_pinned[S + k])) {
            g_err = "log-likelihood of trajectory " + std::to_string(k) + " is not finite";
            return BHMM_ERR_NONFINITE;
        }
    return BHMM_OK;
}

int bhmm_get_gamma(bhmm_ctx *c, int k, double *gamma)
{
    if (!c || c->kind < 0 || !gamma)
        return invalid_arg("bad arguments");
    if (!c->ds.gamma_valid)
        return invalid_arg("last E-step did not store gamma (BHMM_FLAG_STORE_GAMMA)");
    if (k < 0 || k >= c->K)
        return invalid_arg("trajectory index out of range");
    BHMM_HIP(hipSetDevice(c->device));
    const int64_t T = c->offsets[k + 1] - c->offsets[k];
    if (T == 0)
        return BHMM_OK;
    if (c->wide || c->gen) { // already trajectory-major
        BHMM_HIP(hipMemcpyAsync(gamma, c->d_gamma_ci.p + c->offsets[k] * c->n,
                                (size_t)T * c->n * sizeof(double), hipMemcpyDeviceToHost,
                                c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        return BHMM_OK;
    }
    int rc = c->d_scratch.ensure((size_t)T * c->n * sizeof(double));
    if (rc)
        return rc;
    rc = BHMM_DISPATCH_N(c, unpack_rows(c, c->d_gamma_ci.p, reinterpret_cast<double *>(c->d_scratch.p),
                                        k, c->offsets[k]));
    if (rc)
        return rc;
    BHMM_HIP(hipMemcpyAsync(gamma, c->d_scratch.p, (size_t)T * c->n * sizeof(double),
                            hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    return BHMM_OK;
}

// ---- single-trajectory, reference-shaped entry points -------------------------------------
namespace {
struct TmpCtx {
    bhmm_ctx *c = nullptr;
    ~TmpCtx() { bhmm_ctx_destroy(c); }
};

int current_device()
{
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) {
        (void)hipGetLastError();
        d = 0;
    }
    return d;
}

int explicit_ctx(TmpCtx &t, const double *pobs, int N, int64_t T)
{
    if (!pobs || N < 1 || T < 1)
        return invalid_arg("pobs == NULL or empty problem");
    int rc = bhmm_ctx_create(&t.c, current_device(), nullptr);
    if (rc)
        return rc;
    const int64_t off[2] = {0, T};
    return bhmm_ctx_set_observations(t.c, BHMM_EMIT_EXPLICIT, pobs, off, 1, N, 0, 0, 0);
}

int download_rows(bhmm_ctx *c, const double *src_ci, double *dst_host)
{
    const size_t bytes = (size_t)c->total * c->n * sizeof(double);
    int rc = c->d_scratch.ensure(bytes);
    if (rc)
        return rc;
    rc = BHMM_DISPATCH_N(c, unpack_rows(c, src_ci, reinterpret_cast<double *>(c->d_scratch.p), -1, 0));
    if (rc)
        return rc;
    BHMM_HIP(hipMemcpyAsync(dst_host, c->d_scratch.p, bytes, hipMemcpyDeviceToHost, c->stream));
    BHMM_HIP(hipStreamSynchronize(c->stream));
    return BHMM_OK;
}
} // namespace

int bhmm_forward(double *alpha, double *logprob, const double *A, const double *pobs,
                 const double *pi, int N, int64_t T)
{
    if (!alpha || !A || !pi)
        return invalid_arg("NULL argument");
    TmpCtx t;
    int rc = explicit_ctx(t, pobs, N, T);
    if (rc)
        return rc;
    bhmm_ctx *c = t.c;
    if (c->wide || c->gen) {
        if ((rc = c->gen ? gen_forward(c, A, pi, nullptr, nullptr)
                         : wide_forward(c, A, pi, nullptr, nullptr)))
            return rc;
        BHMM_HIP(hipMemcpyAsync(alpha, c->d_alpha_rm.p, (size_t)T * N * sizeof(double),
                                hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
    } else {
        rc = BHMM_DISPATCH_N(c, template sweep_explicit<MODE_FWD>(c, A, pi));
        if (rc)
            return rc;
        rc = download_rows(c, c->d_ws.p, alpha);
        if (rc)
            return rc;
    }
    double ll = 0.0;
    BHMM_HIP(hipMemcpy(&ll, c->d_logLk.p, sizeof(double), hipMemcpyDeviceToHost));
    if (logprob)
        *logprob = ll;
    return BHMM_OK;
}

int bhmm_backward(double *beta, const double *A, const double *pobs, int N, int64_t T)
{
    if (!beta || !A)
        return invalid_arg("NULL argument");
    TmpCtx t;
    int rc = explicit_ctx(t, pobs, N, T);
    if (rc)
        return rc;
    bhmm_ctx *c = t.c;
    if (c->wide || c->gen) {
        if ((rc = c->gen ? gen_backward(c, A) : wide_backward(c, A)))
            return rc;
        BHMM_HIP(hipMemcpyAsync(beta, c->d_alpha_rm.p, (size_t)T * N * sizeof(double),
                                hipMemcpyDeviceToHost, c->stream));
        BHMM_HIP(hipStreamSynchronize(c->stream));
        return BHMM_OK;
    }
    std::vector<double> pi(N, 1.0 / N); // the backward recursion does not involve pi
    rc = BHMM_DISPATCH_N(c, template sweep_explicit<MODE_BWD>(c, A, pi.data()));
    if (rc)
        return rc;
    return download_rows(c, c->d_ws.p, beta);
}

} // extern "C"

