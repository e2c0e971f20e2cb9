/*
 * bhmm_amd.h -- C ABI of the MI355X (gfx950) forward-backward / Baum-Welch engine.
 *
 * This is the drop-in boundary for the hot path of bhmm: plain
 * pointers and sizes, no torch / numpy types.  Two families of entry points:
 *
 *  (1) Single-trajectory, host-pointer kernels with the argument meaning of the
 *      reference's native layer (bhmm/hidden/impl_c/_hidden.h:10-63,
 *      bhmm/output_models/impl_c/_gaussian.h:5, discrete.pyx:25).  They are what
 *      bhmm/hidden/impl_c/hidden.pyx binds today; a maintainer can bind these instead
 *      (INTEGRATION.md shows the ctypes / Cython stubs).  Lengths are int64 here; the
 *      reference uses 32-bit int T (T*N < 2^31).
 *
 *  (2) A batched, device-resident context: observations are uploaded once (they are
 *      constant across EM iterations, maximum_likelihood.py:101) and every EM iteration /
 *      Gibbs sweep is ONE call that processes all trajectories on the GPU and returns
 *      only the reduced sufficient statistics.  It replaces the Python loops at
 *      bhmm/estimators/maximum_likelihood.py:221-282,383-385 (E-step),
 *      :332-352 (Viterbi) and bhmm/estimators/bayesian_sampling.py:283-331 (Gibbs
 *      hidden-path step).
 *
 * All functions return an int status (never exit(), unlike _hidden.c:299-304):
 */
#ifndef BHMM_AMD_H_
#define BHMM_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BHMM_OK 0
#define BHMM_ERR_NO_MEM 2      /* same value as _BHMM_ERR_NO_MEM, _hidden.h:5 */
#define BHMM_ERR_INVALID 3     /* bad argument (shape, NULL, unsupported size) */
#define BHMM_ERR_HIP 4         /* HIP runtime error; see bhmm_last_error() */
#define BHMM_ERR_NONFINITE 5   /* log-likelihood not finite (maximum_likelihood.py:385) */
#define BHMM_ERR_CHOICE 6      /* inverse-CDF draw found no state (_hidden.c:299-304) */
#define BHMM_ERR_NO_DEVICE 7   /* no HIP device / library built without one visible */
#define BHMM_ERR_SIGMA 8       /* M-step: a sigma fell below eps (gaussian.py:271-272, RuntimeError) */
#define BHMM_ERR_DISCONNECTED 9 /* reversible sampling of a disconnected count matrix
                                  (bayesian_sampling.py:347-350, NotImplementedError) */

/* emission model kinds */
#define BHMM_EMIT_GAUSSIAN 0 /* obs: double[T];  par0 = means[N], par1 = sigmas[N]            */
#define BHMM_EMIT_DISCRETE 1 /* obs: int32[T];   par0 = B[N*M] row-major, par1 unused         */
#define BHMM_EMIT_EXPLICIT 2 /* obs: double[T*N] = pobs rows (hidden/api.py signatures)       */

/* flags for bhmm_estep */
#define BHMM_FLAG_STORE_GAMMA 1 /* keep gamma (T,N) per trajectory on the device            */
#define BHMM_FLAG_SINGLE 2      /* the caller accepts single-precision accuracy for this E-step: up to 8
                                 * states, gaussian or discrete, without STORE_GAMMA, it runs the fp32
                                 * kernels (a permission, not a demand: anything else, or an fp32 run whose
                                 * boundary check or ranges do not hold, runs the fp64 path).  Currently
                                 * SLOWER than the fp64 path                     */

const char *bhmm_last_error(void);
int bhmm_device_count(void);
/* library version / build info: "bhmm_amd <ver> gfx950" */
const char *bhmm_version(void);

/* ------------------------------------------------------------------------------------
 * (1) reference-shaped single-trajectory kernels, host pointers, row-major (T,N) arrays.
 *     Each runs on the current HIP device, synchronously.
 * ---------------------------------------------------------------------------------- */

/* replaces _forward (_hidden.h:10-15, _hidden.c:16-66): fills alpha[T*N], *logprob */
int bhmm_forward(double *alpha, double *logprob, const double *A, const double *pobs,
                 const double *pi, int N, int64_t T);
/* replaces _backward (_hidden.h:17-21, _hidden.c:69-110): fills beta[T*N] */
int bhmm_backward(double *beta, const double *A, const double *pobs, int N, int64_t T);
/* replaces hidden/api.py:133-188 (numpy) / _computeGamma (_hidden.c:113-131) */
int bhmm_state_probabilities(double *gamma, const double *alpha, const double *beta, int N,
                             int64_t T);
/* replaces _compute_transition_counts (_hidden.h:34-40, _hidden.c:148-183); C overwritten */
int bhmm_transition_counts(double *C, const double *A, const double *pobs, const double *alpha,
                           const double *beta, int N, int64_t T);
/* replaces _compute_viterbi (_hidden.h:42-47, _hidden.c:203-281); path is int32[T] */
int bhmm_viterbi(int32_t *path, const double *A, const double *pobs, const double *pi, int N,
                 int64_t T);
/* replaces _sample_path (_hidden.h:49-54, _hidden.c:330-378).  u[T] are the uniforms in
 * [0,1), u[t] used for step t (the reference draws them from libc rand(), T-1 first). */
int bhmm_sample_path(int32_t *path, const double *alpha, const double *A, const double *u,
                     int N, int64_t T);
/* The uniforms the reference's _sample_path would consume after set_seed(seed)
 * (_hidden.c:283-327: r = rand()/(RAND_MAX+1.0), first draw used for t = T-1).  Host-only
 * helper on the C library generator; seed < 0 leaves the generator state untouched
 * (hidden.pyx:181-182 seeds only when a seed is given). */
int bhmm_libc_uniforms(double *u, int64_t T, int seed);
/* replaces _p_obs (_gaussian.h:5, _gaussian.c:45-70) + outputmodel.py:119-131 */
int bhmm_pobs_gaussian(double *pobs, const double *obs, const double *mu, const double *sigma,
                       int N, int64_t T, int ignore_outliers);
/* replaces _update_pout (discrete.pyx:25, _discrete.c:1-32): pout[N*M] += scatter */
int bhmm_update_pout(double *pout, const int32_t *obs, const double *weights, int64_t T, int N,
                     int M);

/* Multivariate gaussian log-densities, beside bhmm_pobs_gaussian: logp[t*N + i] =
 * log N(x_t; mu_i, Sigma_i) for X[T*D] row-major, means[N*D] and covs as below, formed by the kernel of
 * bhmm_mvn_emissions (centred, whitened with the inverse Cholesky factor, fp64).  Host pointers, synchronous. */
#define BHMM_COV_FULL 0  /* covs[N*D*D]: symmetric positive definite matrices, row-major */
#define BHMM_COV_DIAG 1  /* covs[N*D]: variances                                          */
#define BHMM_MVN_MAX_D 64
int bhmm_logpdf_mvn(double *logp, const double *X, int64_t T, int D, int N, const double *means,
                    const double *covs, int cov_type);

/* Gaussian-mixture log-densities, beside bhmm_logpdf_mvn: logp[t*N + i] =
 * log sum_c w_ic N(x_t; mu_ic, Sigma_ic) for M components per state, weights[N*M], means[N*M*D] and covs
 * ([N*M*D*D] or [N*M*D]) component (i, c) at i * M + c, formed by the kernel of bhmm_gmm_emissions (below, where
 * the arguments are described).  Host pointers, synchronous. */
int bhmm_logpdf_gmm(double *logp, const double *X, int64_t T, int D, int N, int M, const double *weights,
                    const double *means, const double *covs, int cov_type);

/* Poisson log-densities of counts, beside bhmm_logpdf_mvn: logp[t*N + i] =
 * sum_d [x_td log lambda_id - lambda_id - log(x_td !)] for X[T*D] row-major (counts held as doubles) and
 * rates[N*D], formed by the kernel of bhmm_pois_emissions (below, where the rules are described).  A rate that is
 * negative or not finite, a count that is negative or not an integer, D outside 1..BHMM_MVN_MAX_D: BHMM_ERR_INVALID.
 * Host pointers, synchronous. */
int bhmm_logpdf_poisson(double *logp, const double *X, int64_t T, int D, int N, const double *rates);

/* ------------------------------------------------------------------------------------
 * (2) batched device-resident context
 * ---------------------------------------------------------------------------------- */
typedef struct bhmm_ctx bhmm_ctx;

/* device: HIP ordinal.  stream: a hipStream_t to launch on (NULL = the context creates
 * its own).  The context owns every device buffer it allocates. */
int bhmm_ctx_create(bhmm_ctx **out, int device, void *stream);
int bhmm_ctx_destroy(bhmm_ctx *ctx);

/* Upload K trajectories.  obs is the concatenation of all trajectories (element type per
 * `kind`), offsets[K+1] the element offsets of each trajectory in time steps.
 * nstates = N (1 .. 4096: N <= 8 chunk-parallel kernels, 9 .. 64 the lane-per-state family, above
 * that the any-N family -- E-step on the matrix cores up to 512 states, order-faithful kernels of
 * gen_kernels.hpp beyond and for the bit-exact passes; the reference's _hidden.c has no limit either),
 * nsymbols = M (discrete only).  chunk = time-chunk length used for the
 * parallel-in-time decomposition (0 = choose automatically).  obs_on_device != 0 means
 * `obs` is already a device pointer on the context's device (offsets stay on the host). */
int bhmm_ctx_set_observations(bhmm_ctx *ctx, int kind, const void *obs, const int64_t *offsets,
                              int K, int nstates, int nsymbols, int chunk, int obs_on_device);

/* Lagged views of the observations (bhmm/api.py:70-94, lag_observations): view v is the
 * sub-sampled trajectory obs_k[shift::lag] with k = view_traj[v], shift = view_shift[v], and
 * becomes trajectory v of the context.  The ORIGINAL observations (obs, offsets[K+1], as for
 * bhmm_ctx_set_observations) are uploaded once and the views are cut on the device by strided
 * reads, instead of lag host-side copies uploaded one by one. */
int bhmm_ctx_set_observations_lagged(bhmm_ctx *ctx, int kind, const void *obs,
                                     const int64_t *offsets, int K, int lag,
                                     const int32_t *view_traj, const int32_t *view_shift, int V,
                                     int nstates, int nsymbols, int chunk, int obs_on_device);

/* Number of doubles in the packed statistics vector produced by bhmm_estep for the loaded
 * observations:  [0] sum_k logL_k | [1..N] sum_k gamma_k[0] | N*N transition counts C |
 * N state counts sum_t gamma | emission block:
 *   gaussian: N sum gamma*(o-mu_old), N sum gamma*(o-mu_old)^2     (2N)
 *   discrete: N*M weighted symbol counts (row-major, unnormalised) (N*M)
 *   explicit: none. */
int bhmm_ctx_stats_size(const bhmm_ctx *ctx);

/* One E-step over all loaded trajectories with the given model (host pointers):
 * fused emission probabilities + scaled forward + backward + gamma/xi/emission statistics
 * (maximum_likelihood.py:221-282).  Asynchronous on the context's stream.
 *   stats_dev : device buffer of bhmm_ctx_stats_size() doubles, or NULL to use the
 *               context's internal buffer (read back with bhmm_estep_fetch).  A caller
 *               running several ranks all-reduces this buffer (RCCL) before fetching.
 *   flags     : BHMM_FLAG_* */
int bhmm_estep(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0,
               const double *par1, double *stats_dev, int flags);
/* Wait for the last E-step and copy results to the host.  stats (packed vector) and/or
 * logL_k[K] may be NULL.  Returns BHMM_ERR_NONFINITE if any logL_k is not finite.  With more than
 * 4096 trajectories the K log-likelihoods cross the host link only when logL_k is asked for (or the
 * total is not finite and the offending trajectory has to be named): an EM loop needs stats[0].
 * BHMM_ERR_NONFINITE also if the log-likelihoods are finite but a count (sum gamma_0, C, sum gamma) is
 * not even after bhmm_estep's own retry on one chunk per trajectory (reducible
 * transition matrices with emission probabilities hundreds of decades apart) -- refused loudly instead
 * of handing NaN counts to an M-step.
 * ORDER when bhmm_estep wrote into the caller's stats_dev: the FIRST fetch after the launch (with `stats`, or
 * with logL_k only as a sharded caller does) is where this rank's result is inspected, once per launch --
 * the retry above re-runs the local E-step into the same buffer -- so call it BEFORE reducing the buffer in
 * place; later fetches of the same launch do not look at the buffer's counts again. */
int bhmm_estep_fetch(bhmm_ctx *ctx, double *stats, double *logL_k);
/* After an E-step run with BHMM_FLAG_STORE_GAMMA: copy gamma of trajectory k, (T_k,N)
 * row-major, to the host.  (All trajectories at once, in float or projected, for any model and without
 * an E-step: bhmm_posterior_marginals.) */
int bhmm_get_gamma(bhmm_ctx *ctx, int k, double *gamma);

/* log-likelihood of every loaded trajectory under each of nmodels models, stacked:
   A[nmodels*N*N], pi[nmodels*N], par0/par1 as bhmm_estep per model (gaussian: mu, sigma [N];
   discrete: B [N*M], par1 NULL).  logL[nmodels*K] (host, row s = model s).
   Leaves every carried state of the context untouched.  A trajectory of probability zero under a
   model scores -inf there; a non-finite or non-stochastic model entry is BHMM_ERR_INVALID.
   Forward pass only, no statistics; synchronous.  Up to 8 states (gaussian, discrete): chunk-parallel
   with verified warm-up boundaries (options score_W, score_layout, score_fallbacks).  9 to 64 states
   (gaussian, discrete): parallel over time segments of a plan of its own, same verification and fallbacks
   (options score_seglen: segment length, 0 = automatic; score_lazy; read-only score_segments, score_W_max
   and score_path: 0 serial, 1 chunk kernels, 2 segment kernel, 3 matrix-core kernel).  65 to 128 states
   (gaussian, discrete): the same on the fp64 matrix cores, sixteen segments per workgroup (score_path 3;
   score_seglen, score_W, score_segments, score_W_max, score_fallbacks as above) -- so up to 128 states run
   parallel over time.  Otherwise (more than 128 states, explicit pobs) the exact serial recursion, one
   workgroup per trajectory and model. */
int bhmm_score(bhmm_ctx *ctx, int nmodels, const double *A, const double *pi,
               const double *par0, const double *par1, double *logL);

/* Posterior (maximum-posterior-marginal) decoding of every loaded trajectory under ONE model (A, pi,
   par0, par1 as for bhmm_viterbi_batch): path[t] = argmax_i gamma_t(i), on exactly equal gamma the lowest
   index; conf[t] = max_i gamma_t(i) as float, or nothing when conf == NULL.  path and conf are host buffers
   concatenated over the trajectories like the observations; path holds int32_t, or with path_u8 != 0 one
   byte per step (more than 256 states: BHMM_ERR_INVALID).  The model is validated as by bhmm_score
   (BHMM_ERR_INVALID); synchronous.
   Up to 8 states (gaussian, discrete): one fused forward-backward kernel over the chunk plan with verified
   warm-up boundaries in both directions; no gamma row is stored and every state that E-step, Viterbi,
   sampling and scoring calls use stays untouched.  Options: post_W (warm-up in steps, 0 = measured),
   post_ws_mb (budget of the alpha-row workspace in MiB, default 8192, 0 = unbounded: the call loops over
   ranges of chunk groups, the result does not depend on it); read-only post_fallbacks (calls whose
   boundaries did not verify at the first warm-up: they run again with twice the warm-up, then take the
   generic path) and post_path (first pass of the last call: 3 matrix cores, 2 time segments, 1 fused, 0 generic).
   9 to 64 states (gaussian, discrete), the time-segmented path (post_path 2): k_filter_wide leaves the filtered
   rows of the segments of a plan of its own in a workspace, k_smooth_wide_bwd walks the same segments back and
   decodes; warm-up boundaries of both directions verified, the same retry protocol (post_fallbacks).  No gamma
   row is stored, no statistic is formed and nothing of the state that E-step, Viterbi, sampling, scoring and
   filtering calls use is read or written.  A segment of probability zero or a NaN observation: the generic path
   answers (nothing counted).  Options: smooth_wide (1: always when eligible, 0: never, -1, the default:
   automatic -- only from smooth_wide_min_total steps on and only for the lane-group classes and call forms
   measured faster than the generic path, which is none: it wins at 128 x 1e5 steps but loses at 128 x 1e4, DESIGN.md section 17, so -1 behaves like 0), smooth_seglen (segment length of the plan, 0 = automatic), smooth_W (warm-up in
   steps, 0 = measured), smooth_ws_mb (budget of the workspace in MiB, default 8192, 0 = unbounded: the call
   loops over ranges of whole segments, the result does not depend on it); read-only smooth_segments (segments of
   the plan the last call ran on; 0: another path) and smooth_wide_min_total.
   65 to 128 states (gaussian, discrete), the matrix-core path (post_path 3): k_filter_tile leaves the filtered rows
   of a range of segments in the workspace, k_smooth_tile_bwd walks the same segments back on the fp64 matrix cores
   (sixteen segments per workgroup) and decodes; boundaries of both directions verified, the same retry protocol
   (post_fallbacks); nothing of another call's state is read or written.  A segment either kernel flags (probability
   zero, an outlier, a NaN observation) sends the whole call to the generic path (nothing counted).  Options:
   smooth_tile (1: always when eligible, 0: never, -1, the default: automatic -- only from smooth_tile_min_total
   steps on and only for the call forms measured faster than the generic path in every shape, DESIGN.md section
   18), smooth_seglen, smooth_W (rounded up to a multiple of four) and smooth_ws_mb as above -- here the ranges of
   whole segments also decide which segments share a tile; results are bitwise reproducible at a fixed budget,
   across budgets that is not promised; read-only smooth_segments and smooth_tile_min_total.
   Generic path (9 states and more unless a path above is taken, explicit pobs): a bhmm_estep with BHMM_FLAG_STORE_GAMMA followed by a
   kernel over the stored rows.  It counts as an E-step for the context (last statistics, carried
   boundaries, timers, stored gamma) exactly like the caller's own, needs total * N * 8 bytes for gamma
   (BHMM_ERR_NO_MEM if they are not there) and returns BHMM_ERR_NONFINITE where bhmm_estep_fetch would. */
int bhmm_posterior_decode(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0,
                          const double *par1, void *path, int path_u8, float *conf);

/* Posterior state probabilities of every step of every loaded trajectory under ONE model (A, pi, par0, par1 as
   for bhmm_posterior_decode; validated the same way): the quantity bhmm_posterior_decode takes the argmax of.
   out is trajectory-major, out[(offset_k + t) * Q' + q]:
     V == NULL, Q == 0 : Q' = N, the row is gamma_t(0 .. N-1) and sums to one;
     V[N*Q] row-major, 1 <= Q <= 8 : Q' = Q, the row is sum_i gamma_t(i) * V[i*Q + q], accumulated over i in
       ASCENDING order in fp64 (fused multiply-add) -- set memberships, state means, any few columns.
   flags: BHMM_MARG_F32    rows of float instead of double (the conversion is the last operation: the float
                           result is the rounded double result);
          BHMM_MARG_DEVICE out is a device pointer on the context's device, aligned to 16 bytes: the kernels
                           write it directly, nothing is copied, and the rows are complete in the order of
                           the context's stream (bhmm_ctx_sync, or work enqueued on bhmm_ctx_stream).
   Without BHMM_MARG_DEVICE out is a host buffer of total * Q' values: the rows are staged on the device
   (BHMM_ERR_NO_MEM if they do not fit; nothing is truncated) and cross the link in ONE copy -- pass pinned
   memory for the full link rate, a pageable buffer of 8 MiB or more is pinned for the duration of the copy --
   and the call is synchronous.
   Up to 8 states (gaussian, discrete): the fused forward-backward sweep of bhmm_posterior_decode with the
   normalised row (or its projection) as last stage, the same verified warm-up boundaries and retry protocol;
   nothing of the state that E-step, Viterbi, sampling, scoring and decoding calls use is read or written and no
   gamma row is kept beyond out.  Options: marg_W (warm-up in steps, 0 = measured), marg_ws_mb (budget of the
   alpha-row workspace in MiB, default 8192, 0 = unbounded; the result does not depend on it); read-only
   marg_fallbacks (calls whose boundaries did not verify at the first warm-up: they run again with twice the
   warm-up, then take the generic path) and marg_path (first pass of the last call: 3 matrix cores, 2 time
   segments, 1 fused, 0 generic).
   9 to 64 states (gaussian, discrete), the time-segmented path (marg_path 2): k_filter_wide forward and
   k_smooth_wide_bwd backward over the segments of a plan of its own, as for bhmm_posterior_decode, with the
   normalised row or its projection as last stage; a projection is summed over the states by a fixed tree over
   the lanes, NOT in ascending order (the same bound holds).  Verified in both directions, the same retry
   protocol (marg_fallbacks); no gamma row beyond out, no statistic, nothing of another call's state read or
   written; a segment of probability zero or a NaN observation: the generic path answers.  Options: smooth_wide
   (1: always when eligible, 0: never, -1, the default: automatic -- only from smooth_wide_min_total steps on and only for the lane-group classes and call forms
   measured faster than the generic path, which is none: it wins at 128 x 1e5 steps but loses at 128 x 1e4, DESIGN.md section 17, so -1 behaves like 0), smooth_seglen, smooth_W,
   smooth_ws_mb (as for bhmm_posterior_decode); read-only smooth_segments and smooth_wide_min_total.
   65 to 128 states (gaussian, discrete), the matrix-core path (marg_path 3): k_filter_tile forward and
   k_smooth_tile_bwd backward, as for bhmm_posterior_decode, with the normalised row or its projection as last stage;
   a projection is summed over the states by a fixed tree over sixteen lanes, NOT in ascending order (the same bound
   holds).  Verified in both directions, the same retry protocol (marg_fallbacks); a flagged segment: the generic
   path answers for the whole call.  Options: smooth_tile, smooth_seglen, smooth_W, smooth_ws_mb (as for
   bhmm_posterior_decode); read-only smooth_segments and smooth_tile_min_total.
   Generic path (9 states and more unless a path above is taken, explicit pobs): a bhmm_estep with BHMM_FLAG_STORE_GAMMA followed by one
   kernel over the stored rows.  It counts as an E-step for the context (last statistics, carried boundaries,
   timers, stored gamma) exactly like the caller's own, needs total * N * 8 bytes for gamma besides the staged
   result and returns BHMM_ERR_NONFINITE where bhmm_estep_fetch would. */
#define BHMM_MARG_F32 1
#define BHMM_MARG_DEVICE 2
int bhmm_posterior_marginals(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0,
                             const double *par1, const double *V, int Q, void *out, int flags);

/* Pair posteriors of every step of every loaded trajectory under ONE model (A, pi, par0, par1 as for
   bhmm_posterior_marginals; validated the same way): xi_t(i,j) = P(s_t = i, s_t+1 = j | O) of the transition
   t -> t+1, the quantity whose sum over t is the count matrix of the E-step, in one of two forms.
   out is trajectory-major, out[(offset_k + t) * Q' + q], total rows; row t belongs to the pair (t, t+1) and the
   last row of every trajectory, t = T_k - 1, is written as zeros:
     W == NULL, Q == 0 (the jump form): Q' = 1, the row is P(s_t != s_t+1 | O) = sum_{i != j} xi_t(i,j);
     W[N*N*Q] row-major (W[(i*N + j)*Q + q]), 1 <= Q <= 8 (the projected form): Q' = Q, the row is
       sum_i sum_j xi_t(i,j) * W[i][j][q].
   The unnormalised pairs x_ij are accumulated in fp64 with i the OUTER and j the INNER loop, both in ASCENDING
   order (fused multiply-add), and normalised by ONE multiplication with the reciprocal of sum_ij x_ij (summed in
   the same order).  The jump form is by definition, and bitwise, the projection on the off-diagonal 0/1 mask with
   Q = 1 -- the same order, the diagonal terms added as zero; it only leaves out the loads of W.  Full N x N rows
   are not handed out (N * N * 8 bytes per step): eight pair columns per call.
   flags: BHMM_PAIR_F32    rows of float instead of double (the conversion is the last operation: the float
                           result is the rounded double result);
          BHMM_PAIR_DEVICE out is a device pointer on the context's device, aligned to 16 bytes: the kernels
                           write it directly, nothing is copied, and the rows are complete in the order of
                           the context's stream (bhmm_ctx_sync, or work enqueued on bhmm_ctx_stream).
   Without BHMM_PAIR_DEVICE out is a host buffer of total * Q' values: the rows are staged on the device
   (BHMM_ERR_NO_MEM if they do not fit; nothing is truncated) and cross the link in ONE copy, and the call is
   synchronous.  A trajectory of probability zero is out of contract: its rows are whatever
   bhmm_posterior_marginals would give (NaN).
   Up to 8 states (gaussian, discrete), the fused path (pair_path 1): the forward-backward sweep of
   bhmm_posterior_marginals with the pair row hanging off the backward sweep -- alpha_t(i) A_ij p_t+1(j) beta_t+1(j)
   from the stored alpha row and the vector the backward step forms anyway -- the same verified warm-up boundaries
   and retry protocol; the pair that straddles a chunk edge rests on the verified entry vector of the later chunk.
   Nothing of the state that E-step, Viterbi, sampling, scoring, decoding, marginals and filter calls use is read or
   written: the call keeps its buffers in a group of its own in the context, freed by bhmm_ctx_destroy.
   Options, set and read by bhmm_ctx_set_option / bhmm_ctx_get_option like every other call's (they survive
   bhmm_ctx_set_observations; bhmm_pair_set_option / bhmm_pair_get_option below are the same two doors): pair_W
   (warm-up in steps, 0 = measured), pair_ws_mb (budget of the alpha-row workspace in MiB, default 8192,
   0 = unbounded; the result does not depend on it), pair_fused (default 1; 0: never take the fused path);
   read-only pair_fallbacks (calls whose boundaries did not verify at the first warm-up: they run again with twice
   the warm-up, then take the generic path) and pair_path (first pass of the last call: 1 fused, 0 generic).
   Generic path (9 states and more, explicit pobs, pair_fused 0, fused calls that did not verify): with f_t the
   filtered row, xi_t(i,j) = f_t(i) A_ij gamma_t+1(j) / pred_j, pred_j = sum_i f_t(i) A_ij (a term with pred_j == 0
   is zero) -- a bhmm_filter and a bhmm_posterior_marginals through their own entry points, each on the path it
   picks for the class, fp64 rows of both kept on the device (2 * total * N * 8 bytes, BHMM_ERR_NO_MEM if they do
   not fit), then one kernel over the steps, O(N * N) each.  It counts as whatever those two calls count as for the
   context: at 9 states and more (unless bhmm_posterior_marginals takes a path of its own) an E-step.
   That kernel over the steps is one of two row kernels.  k_pair_rows, any N, one thread per step, accumulates in the
   order stated above.  k_pair_tile, N <= 128, takes 16 steps as one tile on the matrix cores: pred = f_t A and
   u_q = f_t (A o W_q) as one fp64 product (for the jump form A with its diagonal zeroed), then
   sum_j u_q(j) r_j / sum_j pred_j r_j with r_j = gamma_t+1(j) / pred_j (0 where pred_j == 0).  It sums in a fixed tree
   order (the matrix core's over i, then column tiles ascending and a butterfly over j; no atomics, repeated calls
   are bitwise equal, a row does not depend on its neighbours, float is the rounded double) and is held to the same
   bound against the oracle, not to bitwise equality with k_pair_rows (the jump form is still bitwise the projection
   on the mask: both give the same matrix).  Option pair_rows: 0 always k_pair_rows; 1 k_pair_tile whenever
   N <= 128 (every kind, explicit pobs and N <= 8 included), k_pair_rows above; -1 (default) k_pair_tile in the
   classes where it was measured faster in every shape (9 to 64 and 65 to 128 states: both), k_pair_rows up to 8
   states and above 128.
   Read-only pair_rows_kernel: the row kernel of the last generic pass, 0 k_pair_rows, 1 k_pair_tile.  pair_path is 0
   for the generic path whichever row kernel runs. */
#define BHMM_PAIR_F32 1
#define BHMM_PAIR_DEVICE 2
int bhmm_posterior_transitions(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0,
                               const double *par1, const double *W, int Q, void *out, int flags);
/* Kept from the first release of bhmm_posterior_transitions.  bhmm_pair_set_option / bhmm_pair_get_option forward a
   name that begins with pair_ to bhmm_ctx_set_option / bhmm_ctx_get_option (BHMM_ERR_INVALID for any other name, and
   for an unknown or read-only one).  bhmm_pair_release frees the buffers the call keeps in ctx early (it waits for
   the context's stream) and puts the pair_ options and counters back to their defaults; the next call works as on a
   fresh context.  It is NOT needed before bhmm_ctx_destroy, which frees everything. */
int bhmm_pair_set_option(bhmm_ctx *ctx, const char *name, double value);
int bhmm_pair_get_option(bhmm_ctx *ctx, const char *name, double *value);
int bhmm_pair_release(bhmm_ctx *ctx);

/* Filtered state probabilities and one-step predictive log-densities of every step of every loaded trajectory
   under ONE model (A, pi, par0, par1 as for bhmm_posterior_marginals; validated the same way): the forward pass
   of bhmm_score with its rows handed out.
     rows[(offset_k + t) * Q' + q], trajectory-major as bhmm_posterior_marginals writes them:
       V == NULL, Q == 0 : Q' = N, the row is P(s_t = . | o_0 .. o_t) and sums to one;
       V[N*Q] row-major, 1 <= Q <= 8 : Q' = Q, the row is sum_i P(s_t = i | o_0 .. o_t) * V[i*Q + q], accumulated
         over i in ASCENDING order in fp64 (fused multiply-add; filter_path 2 and 3: see below);
     logc[offset_k + t] = log p(o_t | o_0 .. o_{t-1}); logc[offset_k] = log sum_i pi_i p_0(i) (pi is not
       normalised, as in the reference's forward); their sum over a trajectory is its log-likelihood.
   Either output may be NULL, not both.  From the first step of a trajectory whose probability is zero on, its
   rows are zero and its logc -inf; the steps before are the ordinary ones.  Gaussian emissions follow
   bhmm_score: an all-zero emission row or a NaN observation counts as a row of ones.
   flags: BHMM_FILT_F32    both outputs are float (the conversion is the last operation);
          BHMM_FILT_DEVICE both outputs are device pointers on the context's device, aligned to 16 bytes: the
                           kernels write them directly and they are complete in the order of the context's
                           stream.
   Without BHMM_FILT_DEVICE the outputs are host buffers: they are staged on the device (BHMM_ERR_NO_MEM if they
   do not fit; nothing is truncated), each crosses the link in ONE copy after the boundaries verified -- a
   pageable buffer of 8 MiB or more is pinned for the duration of its copy -- and the call is synchronous.
   Up to 8 states (gaussian, discrete): one forward sweep over the chunk plan with verified warm-up boundaries
   (filter_path 1).  9 to 64 states (gaussian, discrete): the time-parallel sweep k_filter_wide over a segment
   plan that belongs to filtering alone, with the same verified warm-up boundaries (filter_path 2) -- taken when
   the option filter_parallel is 1, or -1 (the default) and the loaded set has at least filter_wide_min_total
   steps; on this path the columns of a projection are summed over i by a fixed tree, not in ascending order.
   65 to 128 states (gaussian, discrete, loaded observations): the same recursion on the fp64 matrix cores,
   k_filter_tile, over a segment plan and tile table of its own (filter_path 3) -- taken when filter_parallel is
   not 0 and the option filter_tile is 1, or -1 (the default) and the loaded set has at least
   filter_tile_min_total steps.  A trajectory with a segment that leaves the number range of that kernel
   (probability zero, an outlier whose densities all underflow, a NaN observation) is done again, whole, by the
   serial recursion, the others stand (filter_redone counts them); the columns of a projection are summed by a
   fixed tree here too.
   Everything else (more than 128 states, explicit pobs, filter_parallel or filter_tile 0, smaller sets): the
   serial recursion, one workgroup per trajectory (filter_path 0; at most 4096 states).
   Options: filter_W (warm-up in steps, 0 = measured); filter_seglen (9 to 128 states: segment length of the plan
   from the next call on, rounded up to a multiple of four; 0 = automatic); filter_parallel (-1, 0, 1: above);
   filter_tile (-1, 0, 1: above);
   read-only filter_fallbacks (calls whose boundaries did not verify at the first warm-up: they run again with
   twice the warm-up, then take the serial path), filter_path (first pass of the last call: 3 matrix cores,
   2 time segments, 1 fused, 0 serial), filter_segments (segments of the plan the last call ran on; 0: another
   path), filter_redone (filter_path 3: trajectories of the last call done again on the serial recursion),
   filter_wide_min_total and filter_tile_min_total.
   Nothing of the state that E-step, Viterbi, sampling, scoring, decoding and marginals calls use is read or
   written. */
#define BHMM_FILT_F32 1
#define BHMM_FILT_DEVICE 2
int bhmm_filter(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0, const double *par1,
                const double *V, int Q, void *rows, void *logc, int flags);

/* Viterbi paths of all trajectories (maximum_likelihood.py:332-352).  paths is a host
 * buffer of sum_k T_k int32, trajectory-concatenated like obs. */
int bhmm_viterbi_batch(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0,
                       const double *par1, int32_t *paths);

/* Same paths as bhmm_viterbi_batch, one byte per step (for N <= 256 states -- more return
 * BHMM_ERR_INVALID here and use the int32 form; the int32 form
 * above is the reference's return type, hidden.pyx:161-162, and costs four times the copy).
 * paths_on_device == 0: paths is a host buffer of sum_k T_k bytes -- pass pinned memory
 * (hipHostMalloc / torch pin_memory) for the full link rate, a pageable buffer is pinned for the
 * duration of the copy.  paths_on_device != 0: paths is a device buffer on the context's device
 * and the back-trace kernels write it directly (no copy).  Replaces the Python loop at
 * maximum_likelihood.py:332-352 for callers that keep or post-process paths on the GPU. */
int bhmm_viterbi_batch_u8(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0,
                          const double *par1, uint8_t *paths, int paths_on_device);

/* Dwell segments (runs) of a decoded path, compacted on the device.  A run is a maximal
 * stretch of equal states inside one trajectory: a new run begins at step t if t is the first step of its
 * trajectory or path[t] != path[t - 1].  The trajectories are those of the context's offsets (the views of a lagged
 * set count as trajectories).  Of a path of sum_k T_k steps only the runs cross the link:
 *   run_off[K + 1] (host, required): run_off[k] is the index of the first run of trajectory k, run_off[K] = R the
 *     number of runs; an empty trajectory has run_off[k + 1] == run_off[k];
 *   dwell[N * BHMM_DWELL_COLS] (host, or NULL), per state i: the number of runs in the state, the steps in them, the
 *     longest run, the runs that touch the first or the last step of their trajectory (censored: their true dwell
 *     time is not known) and the steps in those;
 *   jumps[N * N] (host, or NULL): jumps[i * N + j] adjacent run pairs i -> j inside one trajectory (zero diagonal);
 *   the runs themselves stay on the device until bhmm_runs_fetch copies them: start (step index inside the
 *     trajectory, int64), length (int64), state (int32), each of R entries, trajectory after trajectory.
 * Integer work throughout: the results do not depend on the order of anything.
 * bhmm_path_runs takes a GIVEN path, flat and trajectory-concatenated as the decoders write it: path_u8 != 0 one
 * byte per step, else int32; paths_on_device == 0: a host buffer, staged on the device; != 0: a device buffer on the
 * context's device, aligned to 16 bytes (BHMM_ERR_INVALID otherwise), read in place.  A state outside [0, N) gives
 * BHMM_ERR_INVALID: the count pass flags it before anything is indexed by it, and no run is delivered.
 * bhmm_decode_runs decodes under one model and compacts without the path crossing the link: method 0 runs what
 * bhmm_viterbi_batch_u8 with paths_on_device != 0 runs, into a buffer of the context; method 1 what
 * bhmm_posterior_decode runs up to the copy to the host -- the same kernels, options, counters and side effects on
 * the context as those calls.  One byte per step: more than 256 states give BHMM_ERR_INVALID (decode with the
 * calls above and hand the int32 path to bhmm_path_runs).
 * The run buffers are sized from R after the count pass; BHMM_ERR_NO_MEM if they do not fit (nothing is delivered
 * then).  The runs belong to the observation set: bhmm_ctx_set_observations discards them, and bhmm_runs_fetch
 * before a successful call of the two above gives BHMM_ERR_INVALID.  bhmm_runs_fetch: any pointer may be NULL.
 * Read-only options: runs_tile (steps per workgroup), runs_lane (steps per lane), runs_count (R of the last call),
 * runs_ms (device time of its count, scan and scatter passes). */
#define BHMM_DWELL_COLS 5
int bhmm_path_runs(bhmm_ctx *ctx, const void *paths, int path_u8, int paths_on_device, int64_t *run_off,
                   int64_t *dwell, int64_t *jumps);
int bhmm_decode_runs(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0, const double *par1,
                     int method, int64_t *run_off, int64_t *dwell, int64_t *jumps);
int bhmm_runs_fetch(bhmm_ctx *ctx, int64_t *start, int64_t *length, int32_t *state);

/* Joint log-probability of GIVEN hidden paths, log p(s, O | model) -- the "Viterbi score" when s is the Viterbi path
 * (DESIGN.md section 22).  For trajectory k with observations o_0 .. o_{T-1}, path s_0 .. s_{T-1} and model m:
 *   logp[m * K + k] = log pi(s_0) + e(s_0, o_0) + sum_{t >= 1} [ log A(s_{t-1}, s_t) + e(s_t, o_t) ]
 * with every term formed in log space: gaussian e(i, o) = -((o - mu_i) / sigma_i)^2 / 2 - log sigma_i - log(2 pi) / 2
 * (the density is never exponentiated), discrete e(i, o) = log B[i, o], explicit pobs e(i, t) = log pobs[t, i].  The
 * gaussian outlier rule of the recursions (an emission row that underflowed to all zeros counts as all ones) is
 * deliberately NOT applied: an outlier gives a very negative finite term here.  A zero probability gives log 0 = -inf
 * and that trajectory's result is -inf, never NaN, and no other trajectory's changes; a NaN gaussian observation makes
 * its own trajectory's result NaN; an empty trajectory gives 0.0.
 * bhmm_path_logprob: paths as for bhmm_path_runs -- flat and trajectory-concatenated, path_u8 != 0 one byte per step
 * (more than 256 states: BHMM_ERR_INVALID), else int32; paths_on_device == 0: a host buffer, staged in a buffer of
 * this call's own; != 0: a device buffer on the context's device, aligned to 16 bytes (BHMM_ERR_INVALID otherwise),
 * read in place.  A state outside [0, N) gives BHMM_ERR_INVALID: it is flagged before anything is indexed by it and
 * nothing is delivered.  The nmodels models are stacked and validated as for bhmm_score (zeros in A, pi and B are
 * legal); all three emission kinds, any N up to 4096.  The trajectories are those of the context's offsets (the views
 * of a lagged set count as trajectories).  The path and the observations are read ONCE for all models.
 * logp[nmodels * K] (host, row m = model m).
 * bhmm_decode_logprob decodes exactly as bhmm_decode_runs does (method 0: what bhmm_viterbi_batch_u8 with
 * paths_on_device != 0 runs, into a buffer of this call's own; method 1: what bhmm_posterior_decode runs up to the
 * copy to the host -- the same kernels, options, counters and side effects) and scores the decoded path under the
 * same model where it lies: only K doubles cross the link.  Up to 256 states (BHMM_ERR_INVALID above).  logp[K].
 * Both calls are synchronous and touch no other call's state (bhmm_decode_logprob: beyond what the decoders touch).
 * No floating-point atomics: the result is bitwise reproducible from call to call, the same for a host and a device
 * path, for bytes and int32 at the same states, and for a model alone and anywhere inside a stack.
 * Read-only options: pathlp_tile (steps per workgroup), pathlp_lane (consecutive steps per lane), pathlp_table (1: the
 * last call kept the log-transition table in LDS, 0: it read it through L2), pathlp_ms (device time of the last
 * call's passes). */
int bhmm_path_logprob(bhmm_ctx *ctx, const void *paths, int path_u8, int paths_on_device, int nmodels,
                      const double *A, const double *pi, const double *par0, const double *par1, double *logp);
int bhmm_decode_logprob(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0, const double *par1,
                        int method, double *logp);

/* Multivariate gaussian emissions: D-dimensional observations, 1 <= D <= BHMM_MVN_MAX_D, one
 * mean vector and one covariance (full or diagonal) per state.  The recursions run on explicit emission rows; these
 * calls are the two passes over the data around them.
 *   bhmm_ctx_set_observations_mvn keeps X[total*D] (row-major, trajectory-concatenated; offsets, K, nstates, chunk and
 *     obs_on_device as for bhmm_ctx_set_observations) on the device in the context, in buffers of its own that the
 *     re-loads below do not touch and bhmm_ctx_destroy frees.  No model call works before the first
 *     bhmm_mvn_emissions.  A later bhmm_ctx_set_observations[_lagged] by the caller ends the multivariate set.
 *   bhmm_mvn_emissions validates means[N*D] and covs (BHMM_COV_FULL: [N*D*D], BHMM_COV_DIAG: [N*D]; non-finite or
 *     asymmetric: BHMM_ERR_INVALID, not positive definite: BHMM_ERR_SIGMA), forms for every step t and state i
 *       l_ti = -|L_i^-1 (x_t - mu_i)|^2 / 2 - sum_d log L_i[d,d] - D log(2 pi) / 2     (L_i L_i^T = Sigma_i)
 *     in fp64 -- the mean is subtracted first, then the difference is whitened -- and m_t = max_i l_ti, writes the
 *     rows exp(l_ti - m_t) (every finite row has maximum exactly 1.0), sums shift_k = sum_t m_t per trajectory in a
 *     fixed order, and loads the rows as the context's BHMM_EMIT_EXPLICIT observations through
 *     bhmm_ctx_set_observations with obs_on_device = 1.  After it every context call works unchanged with
 *     par0 = par1 = NULL; the true log-likelihood of trajectory k is the context's on the scaled rows plus shift_k,
 *     and the filter's increment of step t the context's plus m_t.  A NaN in x_t makes its row, m_t and shift_k NaN.
 *   bhmm_mvn_fetch_scale copies shift_k[K] and, unless NULL, m_t[total] of the last bhmm_mvn_emissions to the host.
 *   bhmm_mvn_moments: gamma_dev is a DEVICE buffer of total*N doubles, trajectory-major -- what
 *     bhmm_posterior_marginals leaves with BHMM_MARG_DEVICE -- means[N*D] the means the moments are taken about.
 *     out (host), per state i: S0 = sum_t g_ti | S1[D] = sum_t g_ti (x_t - mu_i) | S2 = sum_t g_ti (x_t - mu_i)
 *     (x_t - mu_i)^T, its lower triangle row-major (D (D + 1) / 2, BHMM_COV_FULL) or its diagonal (D,
 *     BHMM_COV_DIAG): N * (1 + D + D (D + 1) / 2) or N * (1 + 2 D) doubles.  One partial per workgroup in a fixed
 *     tree order, a second launch adds the partials in ascending order; no floating-point atomics: bitwise the same
 *     from call to call.  Synchronous.
 *   bhmm_mvn_path_moments: the same packed moments for a hidden path: S0_i = #{t : s_t = i},
 *     S1_i and S2_i the sums of (x_t - mu_i) and (x_t - mu_i)(x_t - mu_i)^T over the steps with s_t = i, in exactly the
 *     layout above.  paths / path_u8 / paths_on_device as for bhmm_path_logprob: int32 or one byte per step,
 *     concatenated like the observations, on the host or (aligned to 16 bytes) on the context's device.  The
 *     arithmetic per step is that of ONE state whatever N is; a state that never occurs gives exact zeros; a state
 *     outside [0, N) gives BHMM_ERR_INVALID (found before anything is indexed by it; nothing is delivered).  The order
 *     of every sum is a function of the path's values alone (a stable sort of each tile's steps by state, one slab per
 *     workgroup, the slabs added in ascending order; no floating-point atomics): bitwise the same from call to call
 *     and for the same path as int32 or bytes, on the host or the device.  Useful on its own: moments of a Viterbi
 *     path are hard-assignment training.  Needs no bhmm_mvn_emissions.  Synchronous.
 *   bhmm_mvn_sample_paths: the Gibbs hidden-path step (bhmm_sample_paths with par0 = par1 = emis = NULL) on the
 *     loaded emission rows, followed by bhmm_mvn_path_moments of the drawn path about means[N*D] into moments (host).
 *     The path is read where the draw left it on the device; it is copied to the host only when paths != NULL.
 *     paths, counts and n0 are bitwise those of bhmm_sample_paths for the same arguments.
 * Read-only options: mvn_rows_ms (device time of the last rows and shift kernels), mvn_reload_ms (host time of the
 * explicit re-load that followed), mvn_moments_ms (device time of the last two moment kernels), mvn_path_moments_ms
 * (device time of the last path moments and their finish). */
int bhmm_ctx_set_observations_mvn(bhmm_ctx *ctx, const double *X, const int64_t *offsets, int K, int D,
                                  int nstates, int chunk, int obs_on_device);
int bhmm_mvn_emissions(bhmm_ctx *ctx, const double *means, const double *covs, int cov_type);
int bhmm_mvn_fetch_scale(bhmm_ctx *ctx, double *shift_k, double *m_t);
/* the scaled rows of the last bhmm_mvn_emissions, rows[total*N] (host; tests and diagnostics) */
int bhmm_mvn_fetch_rows(bhmm_ctx *ctx, double *rows);
int bhmm_mvn_moments(bhmm_ctx *ctx, const double *gamma_dev, const double *means, int cov_type, double *out);
int bhmm_mvn_path_moments(bhmm_ctx *ctx, const void *paths, int path_u8, int paths_on_device, const double *means,
                          int cov_type, double *out);
int bhmm_mvn_sample_paths(bhmm_ctx *ctx, const double *A, const double *pi, const double *u, uint64_t seed,
                          int32_t *paths, int64_t *counts, int64_t *n0, const double *means, int cov_type,
                          double *moments);

/* Gaussian-mixture emissions per state, on the observations of
 * bhmm_ctx_set_observations_mvn: every state i has M components (the same M for all), b_i(x) = sum_c w_ic
 * N(x; mu_ic, Sigma_ic), N * M <= 4096; component (i, c) is entry i * M + c of weights[N*M], means[N*M*D] and covs
 * (BHMM_COV_FULL: [N*M*D*D], BHMM_COV_DIAG: [N*M*D]).  The recursions need nothing new: they run on the explicit
 * rows of the mixture densities.
 *   bhmm_gmm_emissions validates its arguments (M < 1, N * M > 4096, a weight that is not finite or negative, a row
 *     of weights that does not sum to 1 within 1e-8: BHMM_ERR_INVALID; means and covs as bhmm_mvn_emissions), forms
 *       a_tic = log w_ic + l_tic      (l_tic: the arithmetic of bhmm_mvn_emissions on component (i, c); log w_ic formed
 *                                      in long double and rounded once; a component of weight zero is skipped)
 *       L_ti  = log sum_c exp(a_tic)  (online: a running maximum and a rescaled sum per state)
 *     and m_t = max_i L_ti, writes the rows exp(L_ti - m_t) (every finite row has maximum exactly 1.0), shift_k, and
 *     loads the rows as the context's BHMM_EMIT_EXPLICIT observations -- all as bhmm_mvn_emissions does, into the same
 *     buffers: bhmm_mvn_fetch_scale and bhmm_mvn_fetch_rows then deliver the mixture's, the read-only option
 *     mvn_rows_ms its device time.  With M = 1 and weight 1 rows, m_t and shift_k are bitwise those of
 *     bhmm_mvn_emissions.  With want_resp it also keeps log r_t(i,c) = a_tic - L_ti for every component in a buffer
 *     of total * N * M doubles in the context (<= 0; -inf for a weight of zero; the normaliser is formed from the
 *     a_tic of the state themselves, so sum_c exp(log r_t(i,c)) = 1 to a few ulp).  A NaN in x_t makes its row, m_t,
 *     shift_k and its log responsibilities NaN.
 *   bhmm_gmm_fetch_resp copies that buffer, out[total*N*M], to the host: log responsibilities before
 *     bhmm_gmm_moments, the weights u_t(i,c) = gamma_t(i) r_t(i,c) after it (tests and diagnostics).
 *   bhmm_gmm_moments: gamma_dev as for bhmm_mvn_moments (DEVICE, total * N doubles).  Turns the log responsibilities
 *     into the weights u in place (k_gmm_weights) and runs the moment kernels of bhmm_mvn_moments over their N * M
 *     columns about means[N*M*D]: out (host) holds N * M blocks S0_ic | S1_ic | S2_ic in the packed layout of
 *     bhmm_mvn_moments; no floating-point atomics, bitwise the same from call to call.  BHMM_ERR_INVALID when the
 *     last emissions were not bhmm_gmm_emissions with want_resp, or when their responsibilities have been used up
 *     by an earlier bhmm_gmm_moments (make the emissions again).  Synchronous.
 * Read-only option: gmm_weights_ms (device time of the last k_gmm_weights; mvn_moments_ms is that of the moment
 * kernels that followed). */
int bhmm_gmm_emissions(bhmm_ctx *ctx, int M, const double *weights, const double *means, const double *covs,
                       int cov_type, int want_resp);
int bhmm_gmm_fetch_resp(bhmm_ctx *ctx, double *out);
int bhmm_gmm_moments(bhmm_ctx *ctx, const double *gamma_dev, const double *means, int cov_type, double *out);

/* The component of every step of a hidden path: what a Gibbs sweep of a mixture model needs
 * between the path and the parameter draws.  Both calls use the table, M, covariance type and means of the last
 * bhmm_gmm_emissions, which the context keeps (with or without want_resp: the responsibilities are neither read nor
 * needed), and return BHMM_ERR_INVALID when the last emissions on these observations were not a mixture's.
 *   bhmm_gmm_path_components: paths / path_u8 / paths_on_device as for bhmm_mvn_path_moments.  For every step, with
 *     i = s_t, the components c of state i in ascending order, those of weight zero skipped:
 *       a_c = log w_ic + l_tic, the running maximum a* and the rescaled sum s of bhmm_gmm_emissions' log-sum-exp
 *       (a new maximum: s = s exp(a* - a_c) + 1, e = 1; else e = exp(a_c - a*), s += e);
 *       the first component visited is the pick; a later one becomes the pick when u s < e,
 *       u = uniform(key, g M + c) in [0, 1) -- the counter-based generator of bhmm_sample_paths, key one mix of seed
 *       with a constant, g the position of the step in the random stream (its index, or with
 *       bhmm_ctx_set_stream_offsets the trajectory's offset plus the step).
 *     The pick is c with probability e_c / sum e = r_t(i, c) exactly: one pass, nothing stored per component.  A NaN
 *     observation keeps the first component.  labels (host, int32[total], may be NULL): s_t M + c_t.  moments (host):
 *     N * M blocks S0 | S1 | S2 of the labels about the means of those emissions, in the packed layout of
 *     bhmm_gmm_moments, by the kernels of bhmm_mvn_path_moments (the same guarantees: no floating-point atomics,
 *     the order of every sum a function of the labels alone).  A state outside [0, N) gives BHMM_ERR_INVALID (found
 *     before anything is indexed by it; nothing is delivered).  Labels and moments are a function of the
 *     observations, the path, the parameters, the seed and the stream offsets alone: bitwise the same from call to
 *     call, for a host and a device path, for bytes and int32.  Synchronous.
 *   bhmm_gmm_sample_paths: bhmm_sample_paths (par0 = par1 = emis = NULL) on the loaded mixture rows, then the draw
 *     and the moments above on the path where the draw left it on the device, with the same seed (the two streams
 *     are disjoint).  paths, counts and n0 are bitwise those of bhmm_sample_paths for the same arguments; paths and
 *     labels (both may be NULL) cross the link only when given.
 * Memory: 4 bytes per step for the labels; no buffer of total * N * M.  Read-only option: gmm_draw_ms (device time of
 * the last component draw; mvn_path_moments_ms is that of the moment kernels that followed). */
int bhmm_gmm_path_components(bhmm_ctx *ctx, const void *paths, int path_u8, int paths_on_device, uint64_t seed,
                             int32_t *labels, double *moments);
int bhmm_gmm_sample_paths(bhmm_ctx *ctx, const double *A, const double *pi, const double *u, uint64_t seed,
                          int32_t *paths, int32_t *labels, int64_t *counts, int64_t *n0, double *moments);

/* Poisson count emissions, on the observations of bhmm_ctx_set_observations_mvn (counts held
 * as doubles, D channels): state i has a rate lambda_id >= 0 per channel, log b_i(x_t) = sum_d [x_td log lambda_id -
 * lambda_id - log(x_td !)].  The recursions need nothing new: they run on explicit rows.
 *   bhmm_pois_emissions validates rates[N*D] (negative or not finite: BHMM_ERR_INVALID, nothing changes), forms
 *       l_ti = sum_d x_td log lambda_id - Lambda_i      (log lambda in long double, rounded once, log 0 = -inf;
 *                                                        Lambda_i = sum_d lambda_id in ascending d; one fma per
 *                                                        channel in ascending d)
 *     where a channel with x_td = 0 is skipped -- it contributes exactly 0 whatever the rate -- and a positive count
 *     under rate 0 gives -inf; m_t = max_i l_ti and the rows exp(l_ti - m_t) (every finite row has maximum exactly
 *     1.0); a step that every state gives probability zero: a row of zeros and m_t = 0, so that the recursions give
 *     -inf for that trajectory only.  c_t = -sum_d log(x_td !) does not depend on the state: the step scale kept is
 *     m_t + c_t, shift_k their sum per trajectory, so that bhmm_mvn_fetch_scale, the filter increments and every
 *     log-likelihood carry the complete density.  Rows, scales and shifts go into the buffers of bhmm_mvn_emissions
 *     and are loaded the same way; bhmm_mvn_fetch_scale and bhmm_mvn_fetch_rows deliver them, the read-only option
 *     mvn_rows_ms the device time.  A NaN count makes its row, scale and shift_k NaN.  A count that is negative or not
 *     an integer: BHMM_ERR_INVALID, no rows are loaded.
 * The moments of the M-step and of a hidden path are bhmm_mvn_moments / bhmm_mvn_path_moments with BHMM_COV_DIAG about
 * the rates (their second-moment block is not used). */
int bhmm_pois_emissions(bhmm_ctx *ctx, const double *rates);

/* Gibbs hidden-path step (bayesian_sampling.py:283-331): forward pass + backward sampling
 * of every trajectory.  Uniforms come either from u (host, concatenated like obs; u[t]
 * used at step t) or, when u == NULL, from a counter-based generator seeded with `seed`.
 * Outputs (any may be NULL): paths (host, int32, concatenated), and the hidden-path
 * statistics the sweep needs (generic_hmm.py:297-334,398-431):
 *   counts[N*N] int64 transition counts, n0[N] int64 first-state counts,
 *   emis: gaussian -> 3N doubles: n_i, sum (o - mu_i), sum (o - mu_i)^2 over the steps
 *         assigned to state i (mu = par0, the current means); discrete -> N*M counts. */
int bhmm_sample_paths(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0,
                      const double *par1, const double *u, uint64_t seed, int32_t *paths,
                      int64_t *counts, int64_t *n0, double *emis);

/* The same Gibbs step with the hidden-path statistics left ON THE DEVICE as one packed fp64
 * vector of bhmm_ctx_path_stats_size() doubles,
 *   [ counts N*N | n0 N | emission block (gaussian 3N: n_i, sum d, sum d^2; discrete N*M) ],
 * so that several ranks reduce them with ONE all-reduce (RCCL) and ONE device-to-host copy -- the
 * distributed form of generic_hmm.py:297-334,398-431.  The integer counts are < 2^53, so their
 * fp64 sums are exact whatever the order.  paths (host int32, concatenated) may be NULL. */
int bhmm_ctx_path_stats_size(const bhmm_ctx *ctx);
/* Position of each loaded trajectory in the device random stream used when u == NULL: step t of
 * trajectory k draws uniform(seed, soff[k] + t).  Default (soff == NULL, and after every
 * bhmm_ctx_set_observations): the trajectory's offset in this context.  A caller that shards
 * trajectories over several contexts / GPUs passes their offsets in the UNSHARDED concatenation,
 * so that the sampled paths do not depend on the partition.  soff: host, K entries. */
int bhmm_ctx_set_stream_offsets(bhmm_ctx *ctx, const int64_t *soff);
int bhmm_sample_paths_dev(bhmm_ctx *ctx, const double *A, const double *pi, const double *par0,
                          const double *par1, const double *u, uint64_t seed, int32_t *paths,
                          double *stats_dev);

/* Tuning / introspection knobs by name (returns BHMM_ERR_INVALID for an unknown name):
 *   "spec_enabled"  1/0  use speculative, verified chunk boundaries in bhmm_estep (default 1;
 *                        switched off automatically when verification keeps failing)
 *   "spec_W"        warm-up length in time steps.  By default it is read off the forgetting
 *                   curve that the first E-step on new observations measures for the model at
 *                   hand (two differently started chains on 256 sampled stretches, both
 *                   directions; +15 %, 9..64 states: +50 %); a failed check re-measures and
 *                   lengthens it.  Setting it (or BHMM_AMD_SPEC_W) fixes it
 *   "wide_segments" 1/0  (9..64 states) cut trajectories into time segments with the same
 *                        verified warm-up boundaries; reading it returns the segment count in use
 *   "wide_segment_len"   segment length for the next bhmm_ctx_set_observations (0 = automatic)
 *   "carry"         1/0  (N <= 8) in a sequence of E-steps on slowly changing models (EM) start the
 *                        warm-ups from the PREVIOUS E-step's boundary vectors, a shorter distance
 *                        out, sized from the model change and the measured sensitivity; verified
 *                        like every warm-up, repeated with full warm-ups if the check fails.  Not
 *                        used when the model is identical to the previous call's (default 1;
 *                        BHMM_AMD_CARRY=0)
 *   "carry_W", "carry_ok", "carry_fail"  (read-only) warm-up steps of the last E-step's carried
 *                        starts (0: full warm-ups), E-steps that verified on carried starts /
 *                        had to be repeated
 *   "carry_cap"          (read-only) local step at which the last E-step's backward sweep was split
 *                        to capture beta for the next one (0: one stretch, nothing captured)
 *   "obs16"         1/0  (N <= 8, discrete, tables in LDS, nsymbols * N * 8 <= 65536 with N the padded state
 *                        count) the main loops of the two-launch E-step read a second copy of the observations,
 *                        2 bytes per step, packed by bhmm_ctx_set_observations (default 1).  0 keeps them on the
 *                        int32 copy -- same statistics, bit for bit -- from the next E-step on; setting it back
 *                        to 1 takes effect for observations loaded afterwards
 *   "obs16_used"         (read-only) 1 if the sweeps of the last E-step read that copy
 *   "spec_ok", "spec_fail"  (read-only) E-steps whose boundaries verified / fell back
 *   "spec_last_dev" (read-only) largest relative boundary deviation of the last check
 *   "f32_used"      (read-only) 1 if the last E-step ran in fp32 end to end (BHMM_FLAG_SINGLE)
 *   "f32_fallbacks" (read-only) E-steps that asked for fp32 (BHMM_FLAG_SINGLE) and ran the fp64 path
 *   "f32_tol"       relative tolerance of the fp32 E-step's boundary check (default 1e-5); its
 *                   warm-up is read off the measured forgetting curve at a thousandth of it, +50 %
 *   "f32_W"         fixes the fp32 warm-up length in time steps (0: measured, the default; a
 *                   failed check doubles a measured one for the next call)
 *   "f32_last_dev"  (read-only) largest relative boundary deviation of the last fp32 check
 *   "careful"       (read-only) 1 after an E-step met an all-zero emission row (gaussian
 *                   outlier rule, outputmodel.py:126-130) and switched to the kernel that
 *                   applies the rule per step; 9..64 states: 1 after a lazily scaled vector
 *                   left its range and the E-step was repeated with per-step normalisation
 *   "viterbi_chunked" (read-only) 1 if the last bhmm_viterbi_batch ran parallel over time
 *                   chunks (boundaries verified, no close decision), 0 if it ran serially
 *   "viterbi_margin" 1/0/2  (9..256 states) accept a segment-parallel first pass whose boundaries equal their
 *                   predecessors' vectors to 1e-12 by the margins of the decisions on its path (2: up to 64 states
 *                   from the next call on, not only after a call that needed rounds); "viterbi_mend" 1/0  (9..64
 *                   states) segments further than 1e-12 from their predecessor run again alone up to a kept
 *                   vector of the first pass;  read-only: "viterbi_segments", "viterbi_W", "viterbi_mismatch",
 *                   "viterbi_far", "viterbi_mended", "viterbi_rounds", "viterbi_margin_used",
 *                   "viterbi_margin_close"
 *   "draw_watch"    1/0  (bhmm_sample_paths*) draws whose cumulative sums lie within 64 x the deviation the
 *                   forward pass's boundary check measured are decided again on the serial recursion over a
 *                   long window (csrc/draw_verify.hpp); if one does not stand the call is repeated on exact
 *                   alpha rows (default 1).  read-only: "draw_events", "draw_checked", "draw_redone",
 *                   "draw_alpha_dev";  tests: "draw_watch_tol" (watch tolerance), "draw_test_redo" */
int bhmm_ctx_set_option(bhmm_ctx *ctx, const char *name, double value);
int bhmm_ctx_get_option(bhmm_ctx *ctx, const char *name, double *value);

/* introspection (used by bench.py / tests) */
int64_t bhmm_ctx_total_steps(const bhmm_ctx *ctx);
int bhmm_ctx_num_chunks(const bhmm_ctx *ctx);
int bhmm_ctx_chunk_len(const bhmm_ctx *ctx);
/* time in milliseconds spent in the named kernel during the last bhmm_estep, measured with
 * HIP events on the context's stream.  which: 0 prescan, 1 stitch, 2 forward-backward,
 * 3 finalize, 4 whole E-step. Valid after bhmm_estep_fetch (or a stream sync). */
double bhmm_ctx_last_kernel_ms(bhmm_ctx *ctx, int which);
/* all five at once: out[5] (one call inside a timed loop instead of five) */
int bhmm_ctx_last_kernel_ms_all(bhmm_ctx *ctx, double *out);
void *bhmm_ctx_stream(bhmm_ctx *ctx);
int bhmm_ctx_sync(bhmm_ctx *ctx);
/* ------------------------------------------------------------------------------------
 * (2b) more than one GPU: one process (or thread) per device, trajectories sharded over the
 *      ranks (they are independent given the model: maximum_likelihood.py:383-385,
 *      bayesian_sampling.py:288-290), ONE all-reduce of the packed sufficient statistics per EM
 *      iteration / Gibbs sweep -- the distributed form of the host sums at
 *      bhmm/estimators/maximum_likelihood.py:271-282.  RCCL over xGMI, loaded on first use
 *      (librccl.so; BHMM_ERR_INVALID with a message if it is not there -- the rest of the
 *      library does not need it).  The Python estimators use torch.distributed for the same sum
 *      (bhmm_amd/sharding.py); these entry points give a non-Python binder the same thing.
 *
 *   bhmm_comm_unique_id : rank 0 fills 128 bytes and hands them to the other ranks out of band
 *   bhmm_comm_init_rank : collective over the nranks callers; `device` is this rank's GPU
 *   bhmm_ctx_allreduce_stats : in-place sum over the ranks of count doubles in a DEVICE buffer --
 *                          what bhmm_estep(..., stats_dev) / bhmm_sample_paths_dev left there --
 *                          enqueued on the context's stream (no host synchronisation: follow it
 *                          with the copy to the host on the same stream, or bhmm_ctx_sync)
 * ---------------------------------------------------------------------------------- */
typedef struct bhmm_comm bhmm_comm;
#define BHMM_COMM_ID_BYTES 128
int bhmm_comm_unique_id(void *id);
int bhmm_comm_init_rank(bhmm_comm **out, int device, int nranks, int rank, const void *id);
int bhmm_comm_destroy(bhmm_comm *comm);
int bhmm_comm_size(const bhmm_comm *comm, int *nranks, int *rank);
int bhmm_ctx_allreduce_stats(bhmm_ctx *ctx, bhmm_comm *comm, double *stats_dev, int64_t count);

/* Measurement / test support: K synthetic trajectories of T steps each, drawn ON
 * THE DEVICE from the HMM (A, pi, emission) -- hidden path by inverse CDF of pi / the rows of A,
 * one emission per step (recipe of bhmm/hmm/generic_hmm.py:435-507) -- with the counter-based
 * stream of bhmm_sample_paths: step t of trajectory k uses uniform(seed, 2*(k*T+t)) for the state
 * and uniform(seed, 2*(k*T+t)+1) for the emission, so the result does not depend on launch
 * geometry and a host restatement reproduces discrete trajectories bit for bit.
 *   obs_dev    : device buffer, K*T elements, trajectory-concatenated (double | int32 per kind)
 *   states_dev : optional device buffer of K*T bytes receiving the hidden path (may be NULL)
 *   stream     : hipStream_t or NULL;  par0/par1 as for the emission kinds above. */
int bhmm_synth_observations(void *obs_dev, uint8_t *states_dev, int device, void *stream, int kind,
                            const double *A, const double *pi, const double *par0,
                            const double *par1, int N, int M, int K, int64_t T, uint64_t seed);

/* The same for a SLICE of a larger set: this call's trajectory k is trajectory first_traj + k of
 * the set (stream positions 2 * ((first_traj + k) * T + t)), so ranks that each draw their own shard
 * hold exactly the trajectories one process would draw for the whole set. */
int bhmm_synth_observations_at(void *obs_dev, uint8_t *states_dev, int device, void *stream, int kind,
                               const double *A, const double *pi, const double *par0,
                               const double *par1, int N, int M, int K, int64_t T, uint64_t seed,
                               int64_t first_traj);

/* Host-side M-step helper (no device work): the reversible maximum-likelihood transition matrix
 * of a strongly connected count matrix C[n*n] -- the estimator bhmm takes from msmtools
 * (bhmm/estimators/_tmatrix_disconnected.py:94-105, maximum_likelihood.py:306-320) -- by the
 * fixed point x_ij <- (c_ij + c_ji) / (c_i / x_i + c_j / x_j), P_ij = x_ij / x_i, iterated until the
 * row sums of x move by less than maxerr (or maxiter).  P[n*n] row-major; *iterations (optional)
 * receives the number of iterations.  In numpy this loop costs tens of milliseconds per EM
 * iteration next to a 1 ms E-step. */
int bhmm_mle_reversible(double *P, int64_t *iterations, const double *C, int n, int64_t maxiter,
                        double maxerr);

/* ------------------------------------------------------------------------------------
 * (3) host-side model updates between two passes over the trajectories (no device work).
 *     The reference does these in Python / numpy / msmtools; next to a 0.9 ms E-step or Gibbs path
 *     step they must not cost milliseconds, so each is ONE call.
 * ---------------------------------------------------------------------------------- */

/* The whole M-step of one EM iteration (maximum_likelihood.py:284-330) from the packed statistics
 * vector of bhmm_estep (layout: bhmm_ctx_stats_size):
 *   transition matrix  estimate_P (_tmatrix_disconnected.py:68-123: strongly / weakly connected
 *                      sets, reversible fixed point, partially reversible iteration :126-190,
 *                      row normalisation, estimator with a fixed stationary vector),
 *   initial / stationary distribution (maximum_likelihood.py:310-320, _tmatrix_disconnected.py:229-251),
 *   emission parameters (gaussian.py:214-272 from moments about the old means; discrete.py:202-215).
 *   reversible : 1 / 0, or -1 = "reversible iff T_old is" (the reference passes
 *                self._hmm.is_reversible, _tmatrix_disconnected.py:213-226)
 *   stationary : pi_new = stationary distribution of T_new (else normalised sum_k gamma_k[0])
 *   fixed_pi   : NULL, or the fixed stationary (stationary != 0) / initial (stationary == 0) vector
 *   par0_old / par1_old : current emission parameters (gaussian: means, sigmas; else may be NULL)
 *   outputs    : T_new[n*n], pi_new[n], par0_new (means[n] | B[n*M]), par1_new (sigmas[n] | unused)
 *   info       : optional int32[2]: reversible branch taken, fixed-point iterations
 *   warm_state : optional, 1 + n doubles owned by the caller, zero-initialised and handed to every
 *                call of one EM run: the reversible fixed point then starts from the previous
 *                iteration's solution (same fixed point, same stopping rule, far fewer iterations;
 *                only while all states form one closed connected set).  NULL: cold start.
 * Returns BHMM_ERR_SIGMA if a sigma falls below machine epsilon. */
int bhmm_mstep(int kind, int n, int M, const double *stats, const double *T_old,
               const double *par0_old, const double *par1_old, int reversible, int stationary,
               const double *fixed_pi, int64_t maxiter, double maxerr, double mincount,
               double *T_new, double *pi_new, double *par0_new, double *par1_new, int32_t *info,
               double *warm_state);

/* The parameter draws of one Gibbs sweep (bayesian_sampling.py:333-373) from the packed path
 * statistics of bhmm_sample_paths_dev (layout: bhmm_ctx_path_stats_size), in the reference's order:
 *   emission parameters (gaussian.py:303-318 | discrete.py:243-251; par0 / par1 in and out),
 *   transition matrix   reversible: start at the reversible MLE of C = counts + prior_C, zero
 *                       pattern made consistent (:352-357), then `nsteps` FULL sweeps of the
 *                       element-wise Gibbs sampler of Trendelkamp-Schroer et al. 2015 (what
 *                       msmtools.estimation.sample_tmatrix(nsteps=...) counts); else independent
 *                       Dirichlet rows,
 *   initial distribution Dirichlet(n0 + prior_n0) over the positive entries, or (stationary != 0)
 *                       the stationary distribution of the new matrix.
 * Random numbers come from a counter-based generator: the result is a function of (seed, sweep)
 * and the inputs alone, so every rank of a sharded run draws the SAME parameters from the
 * all-reduced statistics without a broadcast.  prior_* may be NULL (zero).  info: optional
 * int32[1], number of 64-bit draws consumed.  Returns BHMM_ERR_DISCONNECTED for reversible
 * sampling of a count matrix that is not strongly connected. */
int bhmm_gibbs_parameters(int kind, int n, int M, const double *path_stats, const double *prior_C,
                          const double *prior_n0, const double *prior_B, int reversible,
                          int stationary, int64_t nsteps, uint64_t seed, uint64_t sweep, double *T,
                          double *p0, double *par0, double *par1, int32_t *info);

/* Multivariate gaussian emissions, host side.  bhmm_host_mvn_prepare: what
 * bhmm_mvn_emissions hands its kernel -- chol: the Cholesky factors L_i ([N*D*D] lower triangular, zeros above, or
 * [N*D] standard deviations), winv: their inverses as packed for the kernel ([N*D(D+1)/2] lower triangle row-major,
 * or [N*D]), cst[N]: -sum_d log L_i[d,d] - D log(2 pi) / 2; formed in long double, rounded once; any output may be
 * NULL.  BHMM_ERR_INVALID for a non-finite or asymmetric covariance, BHMM_ERR_SIGMA for one that is not positive
 * definite.  bhmm_host_mvn_mstep: from the moments of bhmm_mvn_moments about means_old, mu' = mu + S1 / S0 and
 * Sigma' = S2 / S0 - delta delta^T + min_covar I (covs_new in the layout of cov_type); BHMM_ERR_SIGMA if a result is
 * not positive definite. */
int bhmm_host_mvn_prepare(int N, int D, int cov_type, const double *covs, double *chol, double *winv, double *cst);
int bhmm_host_mvn_mstep(int N, int D, int cov_type, const double *moments, const double *means_old,
                        double min_covar, double *means_new, double *covs_new);

/* Poisson count emissions, host side: from the moments of bhmm_mvn_moments with BHMM_COV_DIAG
 * about rates_old[N*D] (N * (1 + 2 D) doubles, the second-moment block is not read), lambda' = max(0, lambda +
 * S1 / S0) into rates_new[N*D]; a state with S0 = 0 keeps its rates. */
int bhmm_host_pois_mstep(int N, int D, const double *moments, const double *rates_old, double *rates_new);

/* The parameter draws of one Gibbs sweep for multivariate gaussian emissions: as
 * bhmm_gibbs_parameters, with path_stats = [C n*n | n0 n | packed moments of bhmm_mvn_path_moments about `means`],
 * means[n*D] and covs ([n*D*D] or [n*D]) in (current) and out (new).  Per state i in ascending order, before the
 * transition matrix, with n_i = S0_i:
 *   n_i = 0: nothing is drawn, nothing changes;
 *   mean: xbar = mu + S1 / n_i, mu' = xbar + L z / sqrt(n_i), z: D standard normals in order, L the Cholesky factor of
 *     the current covariance (diag: the square roots of the variances);
 *   scatter about the new mean: S = S2 - delta S1^T - S1 delta^T + n_i delta delta^T, delta = mu' - mu;
 *   full, when n_i - 1 >= D and S has a Cholesky factor L_S: a Bartlett factor B (lower triangular; first
 *     B_dd = sqrt(chi2(n_i - 1 - d)) for d = 0 .. D-1, then the entries below the diagonal as standard normals,
 *     row-major), Sigma' = (L_S B^-T)(L_S B^-T)^T: inverse Wishart with n_i - 1 degrees of freedom and scale S, always
 *     symmetric positive definite.  Otherwise the covariance stays and info[1] counts the state;
 *   diag, when n_i > 1: sigma2_d = S_dd / chi2(n_i - 1), one chi-square per dimension in order.
 * At D = 1 both types consume the variates of the gaussian kind (gaussian.py:303-318) in its order.  info: optional
 * int32[2]: 64-bit draws consumed, states whose full covariance was kept.  BHMM_ERR_INVALID: bad shapes, cov_type or
 * NULL; BHMM_ERR_SIGMA: a current covariance is not positive definite. */
int bhmm_gibbs_parameters_mvn(int n, int D, int cov_type, const double *path_stats, const double *prior_C,
                              const double *prior_n0, int reversible, int stationary, int64_t nsteps, uint64_t seed,
                              uint64_t sweep, double *T, double *p0, double *means, double *covs, int32_t *info);

/* The parameter draws of one Gibbs sweep for gaussian-mixture emissions per state, host only:
 * path_stats = [C n*n | n0 n | the n * M packed blocks of bhmm_gmm_path_components], weights[n*M], means[n*M*D] and covs
 * ([n*M*D*D] or [n*M*D]) in (current) and out (new); prior_w[n*M] >= 0 (NULL: zeros) the Dirichlet prior of the weights.
 *   On the generator of (seed, sweep): the rule of bhmm_gibbs_parameters_mvn, unchanged, over the n * M components in
 *   ascending order (an empty component keeps its mean and covariance), then the transition matrix and p0 over the n
 *   states as in bhmm_gibbs_parameters.  At M = 1 T, p0, means and covs are bitwise those of
 *   bhmm_gibbs_parameters_mvn on the same statistics.
 *   On a generator of their own, (seed', sweep) with seed' one mix of seed with a constant: per state i in ascending
 *   order w_i ~ Dirichlet(alpha_i), alpha_ic = prior_w[i,c] + S0_ic.  A component with alpha_ic = 0 takes weight exactly
 *   0; a state whose alpha are all 0 keeps its weights; M = 1 consumes nothing.
 * info: optional int32[3]: 64-bit draws consumed by the first generator, components whose covariance was kept (as
 * info[1] of bhmm_gibbs_parameters_mvn), components of weight 0 after the call. */
int bhmm_gibbs_parameters_gmm(int n, int M, int D, int cov_type, const double *path_stats, const double *prior_C,
                              const double *prior_n0, const double *prior_w, int reversible, int stationary,
                              int64_t nsteps, uint64_t seed, uint64_t sweep, double *T, double *p0, double *weights,
                              double *means, double *covs, int32_t *info);

/* building blocks of the two calls above, exported for the parity / property tests:
 * component label per state (sets numbered by decreasing size, _tmatrix_disconnected.py:28-43) */
int bhmm_host_connected_sets(int32_t *label, const double *C, int n, double mincount, int strong);
int bhmm_host_stationary_vector(double *pi, const double *P, int n);
int bhmm_host_estimate_tmatrix(double *P, const double *C, int n, int reversible, const double *fixed_pi,
                         int64_t maxiter, double maxerr, double mincount, int64_t *iterations);
int bhmm_host_is_reversible(const double *P, int n); /* 1 / 0 (-1: bad argument) */
/* `nsweeps` full sweeps of the reversible transition-matrix posterior sampler (the draw of
 * bayesian_sampling.py:341-360 inside bhmm_gibbs_parameters) on the symmetric flux matrix X (n x n, in/out)
 * for the count matrix C.  base keys the per-update random streams; lanes: 0 = the widest instantiation the
 * CPU runs, 1 = one lane, 4 = AVX2 -- the result does not depend on it (that is what the tests check).
 * Returns the number of lanes used, negative on a bad argument. */
int bhmm_host_sample_reversible(double *X, const double *C, int n, int64_t nsweeps, uint64_t base, int lanes);
/* _tmatrix_disconnected.py:126-190: rows in_set != 0 of P (n x n, in/out) */
int bhmm_host_partial_rev(double *P, const double *C, int n, const int32_t *in_set, int64_t maxiter,
                          double maxerr);
/* `count` draws of the counter-based generator: what = 0 uniform [0,1), 1 standard normal,
 * 2 gamma(param), 3 uniform (0,1) */
int bhmm_host_rng_draws(double *out, int64_t count, int what, double param, uint64_t seed,
                        uint64_t stream);

/* diagnostics: y[i] = the E-step kernels' exp() for non-positive arguments (the exponential
 * of the gaussian density, _gaussian.c:18), so that tests can bound its error in ulps */
int bhmm_diag_exp_nonpos(double *y, const double *x, int64_t n);
/* y[i] = the E-step kernels' gaussian density of observation o[i] for one state (mu, sigma)
 * (_gaussian.c:18-20); nansafe = the variant of the per-step-checked kernels */
int bhmm_diag_gauss_pdf(double *y, const double *o, int64_t n, double mu, double sigma,
                        int nansafe);

#ifdef __cplusplus
}
#endif
#endif /* BHMM_AMD_H_ */
