/*
 * tamcmc_sampler.h -- C ABI of the sampler that calls the hot path (host-side mirror of the reference's
 * MALA + Model_def classes, tamcmc/sources/MALA.cpp, tamcmc/sources/model_def.cpp).
 *
 * The reference drives the hot path from MALA::execute (MALA.cpp:555-747): per iteration, for every tempered chain,
 * propose -> Model_def::generate_model -> accept; then Robbins-Monro adaptation and a parallel-tempering swap.
 * tamcmc_sampler_run() is that loop with the chains batched into one device call per iteration.
 * The configuration struct carries what Config::setup (config.cpp:167-396) would have produced from the
 * .cfg/.model/.data files: Input_Data{inputs, relax, priors, plength, extra_priors} and the !MALA section.
 */
#ifndef TAMCMC_SAMPLER_H
#define TAMCMC_SAMPLER_H

#include <stdint.h>

#include "tamcmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamcmc_sampler tamcmc_sampler;

typedef struct tamcmc_sampler_config {
    /* modeling (config_default.cfg !Modeling; ids from Config/default/{models,priors,likelihoods}_ctrl.list) */
    int32_t model_id;        /* model_fct_name_switch: 0, 1, 3, 11, 23, 25, 27 */
    int32_t prior_class;     /* prior_fct_name_switch: 0 = priors_Kallinger2014_Gaussian, 1 = priors_Harvey_Gaussian, 2 = io_MS_Global,
                                3 = io_local, 4 = io_asymptotic */
    int32_t likelihood_id;   /* 0 = chi(2,2p) */
    int32_t use_drift;       /* 0 = adaptive random-walk MH (the reference), 1 = Langevin drift with FD gradient */
    double likelihood_params;/* p */
    int64_t Nparams;
    const double *inputs;          /* [Nparams] initial parameter vector */
    const int32_t *relax;          /* [Nparams] 1 = free */
    const int32_t *plength;        /* [11], summing to Nparams (ids 0 and 1: {Nparams, 0, ...}, see tamcmc_io_load_model_simple) */
    const double *priors;          /* [4 x Nparams] row-major */
    const int32_t *priors_switch;  /* [Nparams] primitive prior ids (primepriors_ctrl.list) */
    const double *extra_priors;    /* [n_extra] */
    int32_t n_extra;
    /* !MALA section */
    int32_t Nchains;
    double lambda_temp, target_acceptance, c0, epsilon1, epsilon2, A1, delta, delta_x;
    const int64_t *Nt_learn;       /* [n_Nt_learn] */
    const int64_t *periods_learn;  /* [n_Nt_learn-1] */
    int32_t n_Nt_learn;
    int32_t engine;                /* 0 = host-driven loop (one batched device call per iteration),
                                      1 = device-resident iteration (proposal, priors, unpack, accept, swap, adaptation on the GPU;
                                          use_drift = 1: the Langevin step with the gradient batch on the device -- see the limits
                                          table below for the red-giant and the Gaussian-envelope models) */
    int64_t dN_mixing;
    const double *init_errors;     /* [Nvars] initial proposal standard deviations (errors_default.cfg), NULL -> 1 */
    /* additions of this build */
    uint64_t seed;                 /* counter-based RNG seed (the reference seeds libc rand() with time(NULL)) */
    double fd_step_rel;            /* forward-difference step = fd_step_rel * max(|theta_k|, 1e-3); 0 -> 1e-7 */
    int32_t chain_groups;          /* device engine, lockstep scheme (iterations with adaptation): the chains run as this many groups
                                      on separate HIP streams (one group's proposal kernel overlaps another's likelihood kernel).
                                      0 = default (2 from 8 chains on); use 1 when several stars share a GPU
                                      (tamcmc_sampler_run_packed): the co-resident stars already fill each other's gaps */
    int32_t swap_rule;             /* what chain B = A+1 stores as logPosterior after an accepted parallel-tempering swap:
                                      0 = logL_A(T_B) + logPrior_A, the posterior of the position it receives (default);
                                      1 = the reference as executed: MALA.cpp:433 overwrites logPrior[A] with B's before MALA.cpp:444
                                          reads it, so B stores logL_A(T_B) + its OWN OLD prior (that value enters B's next MH ratio,
                                          MALA.cpp:515, until B accepts a move) */
} tamcmc_sampler_config;

/* The context must already hold the spectrum (tamcmc_hip_set_spectrum). It is borrowed, not owned: the sampler uses its stream and
 * device buffers.  Destruction order is free: tamcmc_hip_destroy on a context that still has samplers defers the release to the
 * last tamcmc_sampler_destroy. */
int tamcmc_sampler_create(tamcmc_sampler **s, tamcmc_hip_ctx *ctx, const tamcmc_sampler_config *cfg);
void tamcmc_sampler_destroy(tamcmc_sampler *s);
int64_t tamcmc_sampler_nvars(const tamcmc_sampler *s);

/* ---- size limits of the sampler (the reference factors any size with Eigen's LLT, MALA.cpp:339-369, and caps Nchains at 24, :580-587) ----
 *   quantity                       limit                 beyond it
 *   Nchains                        <= 64                 tamcmc_sampler_create returns TAMCMC_ERR_BAD_ARG
 *   Harvey terms                   <= TAMCMC_MAX_HARVEY  TAMCMC_ERR_BAD_ARG
 *   Nvars, device engine:          none                  the adaptation's work matrix (Nvars^2 + Nvars doubles: covariance update, Cholesky
 *     adaptation workspace in LDS  while (Nvars^2 + Nvars) 8 B + (Nparams + 2 Nvars) 8 B + 4.3 KB <= 150 KB, i.e. Nvars <~ 135
 *                                                        factor) moves from LDS to a per-chain block of device memory -- same operations
 *                                                        in the same order, same factor bit for bit, several times slower per learning
 *                                                        iteration (TAMCMC_INFO_ADAPT_IN_LDS = 0); the Langevin engine's test kernel: Nvars <~ 139
 *   Nparams + 2 Nvars, device      <= 971                the fused one-launch iteration borrows the likelihood tile's 12 KB of LDS for its
 *     engine, fused step                                 candidate roles; longer vectors run every iteration on the lockstep kernels
 *                                                        (TAMCMC_INFO_FUSED_AVAILABLE = 0) -- same chains bit for bit
 *   red-giant models (ids 25/27)   device engine: lockstep kernels only.  Its Langevin step (engine = 1 with use_drift = 1) is opt-in:
 *                                  TAMCMC_ERR_BAD_MODEL at tamcmc_sampler_create unless the context has TAMCMC_OPT_RGB_DEVICE_LANGEVIN = 1
 *                                  at that moment.  Such a sampler runs under FAST / FAST_DIRECT arithmetic and TAMCMC_GRADIENT_FD:
 *                                  tamcmc_sampler_run on a STRICT context returns TAMCMC_ERR_BAD_ARG (the long-double unpack STRICT
 *                                  promises is the host's, and the proposals never leave the device), under TAMCMC_GRADIENT_ADJOINT
 *                                  TAMCMC_ERR_BAD_MODEL; either way the chains stay where they were and a later call continues them.
 *                                  With TAMCMC_OPT_RGB_ADJOINT = 1 (read at every call) TAMCMC_GRADIENT_ADJOINT is accepted by both
 *                                  engines: the hybrid batch of tamcmc_hip.h (tamcmc_hip_adjoint_table) -- the table-space adjoint for
 *                                  the perturbed vectors whose rows correspond one to one with the base table's (same count, same l,
 *                                  every l=1 row within half the distance to its nearest l=1 neighbour), the windowed finite difference
 *                                  for the others; tolerances there.  A sampler whose options change between two calls continues its
 *                                  chain from a gradient taken on the new route.
 *                                  Nchains (Nvars + 1) <= 65535.  Host-driven engine: random walk or Langevin, any arithmetic mode
 *                                  (tamcmc_hip_fd_gradient_posterior; the adjoint routes: FAST / FAST_DIRECT)
 *   Gaussian-envelope models       host-driven engine: random walk or Langevin.  Device engine (engine = 1): opt-in, one option per
 *     (ids 0/1)                    step -- TAMCMC_ERR_BAD_MODEL at tamcmc_sampler_create unless the context has, at that moment,
 *                                  TAMCMC_OPT_ENVELOPE_DEVICE_ENGINE = 1 for use_drift = 0 or TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN = 1 for
 *                                  use_drift = 1; neither option implies the other.  prior_class must equal model_id.
 *                                  Langevin step (use_drift = 1): lockstep kernels only (TAMCMC_INFO_ITER_LOCKSTEP), nothing crosses
 *                                  PCIe inside an iteration.  One gradient route, the analytic gradient of tamcmc_hip.h
 *                                  (tamcmc_hip_envelope_gradient_sums) with its chain rule on the device in double;
 *                                  TAMCMC_OPT_ENVELOPE_GRADIENT is not read.  Under TAMCMC_GRADIENT_ADJOINT tamcmc_sampler_run returns
 *                                  TAMCMC_ERR_BAD_MODEL before anything is enqueued: the chains, the counters and the held gradients
 *                                  stay where they were and a later call continues them.  tamcmc_sampler_get_gradient and
 *                                  _get_last_test as for the other device Langevin samplers; tamcmc_sampler_get_envelope_rows gives
 *                                  the rows of the last proposals.  The rest of this entry is the random walk's (use_drift = 0):
 *                                  Runs of three or more iterations without adaptation take ONE launch per iteration (k_env_step: every 1024-bin tile of a chain
 *                                  settles the previous test, proposes and evaluates; counted by TAMCMC_INFO_ITER_FUSED /
 *                                  _FUSED_STRETCHES) while Nx <= 32768 (id 1) or 6144 (id 0, whose step repeats the xi pass over the whole
 *                                  spectrum in every tile: the measured crossover) and TAMCMC_OPT_STEP_SCHEME != 1; everything else on the lockstep
 *                                  kernels (k_iterate -> k_env_ksi / k_env_eval).  Same chains bit for bit either way; a chain's stored
 *                                  logL is what tamcmc_hip_loglike_params_batch returns for the same EnvRow bits, i.e. within 1e-12 |logL|
 *                                  of the reference.  TAMCMC_OPT_WORKGROUP / _BINS_PER_THREAD / _PRECISION do not apply.  No tables:
 *                                  tamcmc_sampler_get_tables -> TAMCMC_ERR_BAD_MODEL; see tamcmc_sampler_get_envelope_rows
 *   tamcmc_sampler_seed_proposal   models 3, 11, 12, 13, 14, 23, and with TAMCMC_OPT_RGB_FISHER = 1 the red giants 25, 27, on a FAST or
 *     _fisher                      FAST_DIRECT context, both engines (tamcmc_hip_fisher's refusals: ids 0, 1, and 25, 27 with the option
 *                                  at 0 -> TAMCMC_ERR_BAD_MODEL, STRICT -> TAMCMC_ERR_BAD_ARG); Nvars <= 16384
 * The host-driven engine has no size-dependent branches (host memory, column Cholesky).
 * tamcmc_sampler_get_info reports which side of each limit a sampler is on and how many iterations each scheme has run. */
#define TAMCMC_INFO_ENGINE 0          /* 0 host-driven, 1 device-resident */
#define TAMCMC_INFO_NVARS 1
#define TAMCMC_INFO_NPARAMS 2
#define TAMCMC_INFO_NCHAINS 3
#define TAMCMC_INFO_ADAPT_IN_LDS 4    /* device engine: 1 = adaptation workspace in LDS, 0 = in device memory; -1 host engine */
#define TAMCMC_INFO_FUSED_AVAILABLE 5 /* device engine: the fused one-launch iteration can be used for this star */
#define TAMCMC_INFO_CHAIN_GROUPS 6
#define TAMCMC_INFO_ITER_FUSED 7      /* iterations run as fused launches since creation */
#define TAMCMC_INFO_ITER_LOCKSTEP 8   /* iterations run by the lockstep kernels (adaptation, long vectors, red giants, Langevin) */
#define TAMCMC_INFO_FUSED_STRETCHES 9  /* fused stretches since creation; the first launch of a stretch starts from settled chains, so
                                          the likelihood tiles have decided Nchains * (ITER_FUSED - FUSED_STRETCHES) tests */
#define TAMCMC_INFO_QUICK_FALLBACKS 10 /* of those, the tests for which the tiles' decision shortcut answered "undecided" and the exact
                                          evaluation ran instead (counted by the chain's first tile) */
#define TAMCMC_INFO_QUICK_SURE 11      /* of those, the tests of chains outside the swap pair whose record said "cannot be accepted"
                                          (proposal outside a prior's support): decided without sums, also under
                                          TAMCMC_OPT_QUICK_DECIDE = 1, where FALLBACKS + SURE = the number of tile tests */
#define TAMCMC_INFO_ITER_JOINT 12      /* of ITER_FUSED with two chain groups: iterations run as ONE launch over all chains (a swap pair
                                          on the moved boundary of a window) */
#define TAMCMC_INFO_ITER_WINDOW 13     /* ... and iterations run as two launches with the boundary between the groups moved by one chain
                                          (the iteration of a swap pair that straddles the groups, and the next) */
#define TAMCMC_INFO_QUICK_MISMATCH 14  /* tests that the decision shortcut decided OTHERWISE than the exact evaluation: every commit
                                          workgroup asks both.  0 -- anything else is a defect of the shortcut */
#define TAMCMC_INFO_FACTOR_UPDATES 15   /* rank-one steps of the proposal factor taken since creation, summed over the chains
                                          (TAMCMC_OPT_FACTOR_REFRESH >= 2; always 0 otherwise) */
#define TAMCMC_INFO_FACTOR_REFRESHES 16 /* full factorisations of adapting iterations that were SCHEDULED, summed over the chains: every
                                          adapting iteration with R < 2, every R-th otherwise */
#define TAMCMC_INFO_FACTOR_FORCED 17    /* full factorisations in an adapting iteration scheduled as a rank-one step, forced by the rule
                                          below (gain, rescaled covariance, a factor not marked valid), summed over the chains */
#define TAMCMC_SAMPLER_INFO_N 18
int tamcmc_sampler_get_info(const tamcmc_sampler *s, int64_t *info, int32_t n);

/* Advances all chains by n_iter iterations.  Optional outputs, one record per iteration after the swap step
 * (what update_buffer_params / update_buffer_stat_criteria record, MALA.cpp:708-710):
 *   samples : [n_iter x Nchains x Nvars]      stats : [n_iter x Nchains x 3] = logL (tempered), logPrior, logPosterior */
int tamcmc_sampler_run(tamcmc_sampler *s, int64_t n_iter, double *samples, double *stats);
/* S independent stars at once: tamcmc_sampler_run on every sampler, one host thread each (each sampler on its OWN context; the
 * contexts may share a GPU).  One star's MCMC iteration is two short dependent kernels and leaves most of an MI355X idle, so
 * co-resident stars raise the GPU's aggregate samples/s (~2x at 4 stars of the C3 size); each star's samples are bit-identical to a
 * run on its own (no shared state, random numbers addressed by (seed, chain, iteration)).  samples / stats: S pointers (or NULL
 * arrays / NULL entries).  Returns the first non-zero status. */
int tamcmc_sampler_run_packed(tamcmc_sampler *const *s, int32_t S, int64_t n_iter, double *const *samples, double *const *stats);

/* The random numbers iteration `iteration` consumes -- the counter-based streams (csrc/rng.h) that replace the reference's
 * rand() (MALA.cpp:62-63, random_JB.cpp:99-105,255), pure functions of (seed, chain, iteration): z [Nchains x Nvars] = the normals of
 * new_prop_values (MALA.cpp:352), u_accept [Nchains] = the comparators of update_position_MH (MALA.cpp:467,536), *u_swap / *ind_A = the
 * comparator and first chain of parallel_tempering (MALA.cpp:400,406).  Lets a caller replay or audit any step. Pointers may be NULL. */
int tamcmc_sampler_draws(const tamcmc_sampler *s, int64_t iteration, double *z, double *u_accept, double *u_swap, int32_t *ind_A);

/* Current state. Any pointer may be NULL.
 *   vars [Nchains x Nvars], logL/logPrior/logPost/Pmove/sigma [Nchains], counters [4] = iteration, accepted moves
 *   of chain 0, swap attempts, swaps accepted */
int tamcmc_sampler_get_state(const tamcmc_sampler *s, double *vars, double *logL, double *logPrior, double *logPost,
                             double *Pmove, double *sigma, int64_t *counters);
/* use_drift = 1: the gradient of the tempered log-posterior the sampler HOLDS for each chain's current position -- computed when that
 * position was proposed, carried through the accept step and, after a parallel-tempering swap, moved to the partner with its likelihood
 * share re-tempered (grad_prior = the prior's share).  grad / grad_prior [Nchains x Nvars], valid [Nchains] (0: will be recomputed before
 * its next use: start of a run, positions set from outside); any pointer may be NULL.  An audit entry like tamcmc_sampler_draws. */
int tamcmc_sampler_get_gradient(const tamcmc_sampler *s, double *grad, double *grad_prior, int32_t *valid);
/* What the LAST iteration tested -- the proposals vars_prop [Nchains x Nvars], their logL (tempered) / logPrior / logPosterior
 * stats_prop [Nchains x 3] and, with use_drift = 1, lq [Nchains x 2] = log q(x'|x), log q(x|x') without the constant the two share,
 * and grad_prop [Nchains x Nvars] = the gradient at the proposals.  Audit entry (tests replay an iteration piece by piece); any
 * pointer may be NULL.  Host-driven engine: everything.  Device-resident engine: use_drift = 1 only (else TAMCMC_ERR_BAD_ARG),
 * vars_prop and grad_prop; stats_prop and lq come back as NaN (those scalars are not kept). */
int tamcmc_sampler_get_last_test(const tamcmc_sampler *s, double *vars_prop, double *stats_prop, double *lq, double *grad_prop);
/* Audit entry of the device-resident random-walk engine (models 3, 11, 12, 13, 14, 23, and the red giants 25, 27: always scheme 1, rows
 * per slot = Nfl0 + Nfl2 + Nfl3 + 400, the rows k_rgb_finish left; host-driven engine, Langevin step,
 * Gaussian-envelope ids 0 / 1 -- they have no table --: TAMCMC_ERR_BAD_MODEL): the multiplet tables the last stretch of the last tamcmc_sampler_run left in the likelihood kernel's input
 * block, and the parameter vector each was built from -- both read from the engine's own buffers, nothing is replayed.
 *   shape[4] = scheme, slots, rows per slot, noise stride (always returned; call with every other pointer NULL for the sizes)
 *   scheme 0  no stretch has run yet (slots = 0)
 *   scheme 1  lockstep: slots = Nchains; slot m is the table of chain m's proposal of the last iteration and params[m] is that proposal
 *             (the engine's params_prop of that iteration's parity); status and logprior are the proposal's.  A proposal whose log-prior
 *             is not finite is not unpacked, a table that fails is discarded: either way the slot holds the placeholder (no rows,
 *             nnoise = 1, noise[0] = 1, nharvey = 0)
 *   scheme 2  fused: slots = 3 (2 Nchains + 8): slot e (2 Nchains + 8) + s is candidate slot s of candidate set e (the candidates of the
 *             iterations = e mod 3) and params[slot] is the candidate vector the same launch stored for that slot (cand_params); status is
 *             the status of the slot's table, logprior the candidate's log-prior.  A table that fails leaves an EMPTY slot (no rows,
 *             nnoise = 0); the table is built whatever the prior says.  written[slot] = 0: no launch has written the slot yet.
 * Out (any may be NULL): rows [slots x rows per slot] (a slot's first nrows[slot] rows are its table), nrows, nharvey, nnoise, status,
 * written [slots], noise [slots x stride], logprior [slots], params [slots x Nparams]. */
int tamcmc_sampler_get_tables(const tamcmc_sampler *s, int32_t *shape, void *rows, int32_t *nrows, double *noise, int32_t *nharvey,
                              int32_t *nnoise, int32_t *status, int32_t *written, double *logprior, double *params);
/* Audit entry of the device-resident engine for the Gaussian-envelope models (ids 0 / 1; anything else: TAMCMC_ERR_BAD_MODEL; before the
 * first tamcmc_sampler_run: TAMCMC_ERR_BAD_ARG): for every chain the scalars the LAST iteration's proposal was evaluated from, the
 * parameter vector they were built from, its log-prior and status -- read from the engine's own buffers, nothing is replayed.
 *   rows [Nchains x TAMCMC_ENVELOPE_ROW_N], the fields of the engine's row as doubles:
 *     [0] amp  [1] numax  [2] sigma^2  [3] N0                                   (Gaussian and white noise, both ids)
 *     [4..5] H_k  [6..7] ln(1e-3 tc_k)  [8..9] p_k                              (id 1: Harvey terms k = 0, 1)
 *     [10..12] b_k  [13..15] ln b_k  [16..18] c_k  [19..21] a_k^2               (id 0: super-Lorentzians k = 0, 1, 2)
 *     [22..23] 1.0 where Harvey term k is active (tc_k != 0), else 0.0          (id 1)
 *     (the fields of the other id are 0)
 *   params [Nchains x Nparams], logprior [Nchains], status [Nchains].  Any pointer may be NULL.
 * A proposal whose log-prior is -inf or NaN, or whose status is not TAMCMC_OK, is rejected whatever its row holds. */
#define TAMCMC_ENVELOPE_ROW_N 24
int tamcmc_sampler_get_envelope_rows(const tamcmc_sampler *s, double *rows, double *params, double *logprior, int32_t *status);

/* Audit entry of the device-resident engine's Langevin step for the Gaussian-envelope models (ids 0 / 1 created with
 * TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN; anything else: TAMCMC_ERR_BAD_MODEL; before the first tamcmc_sampler_run: TAMCMC_ERR_BAD_ARG): the
 * sums the analytic gradient's kernels folded for the LAST iteration's proposals, as the device's chain rule read them -- S [Nchains]
 * (logL = -p S / T), the tile sums [Nchains x 16] and the xi sums [Nchains x 12] in the kernels' own layout -- read
 * from the engine's buffers.  With the rows of tamcmc_sampler_get_envelope_rows they are everything the chain rule starts from: a
 * replay in another arithmetic needs nothing else.  Any pointer may be NULL. */
int tamcmc_sampler_get_envelope_gradient_sums(const tamcmc_sampler *s, double *S, double *tile_sums, double *xi_sums);
/* moves [Nchains]: for every chain the number of iterations since creation whose record carries moved = 1 -- the flag the reference
 * stores per iteration and chain (MALA.cpp:543-545; a swap exchanges the pair's flags, :436, :446) and its acceptance diagnostic counts
 * per buffer (Outputs::reject_rate / count_accepted_vals, outputs.cpp:1824-1858).  Differences between two calls / the iterations in
 * between = the acceptance rates of that buffer (tamcmc_outputs_write_acceptance). */
int tamcmc_sampler_get_move_counts(const tamcmc_sampler *s, int64_t *moves);
/* proposal law of chain m: mu [Nvars], covarmat [Nvars x Nvars] (restore file content, outputs.cpp:863-1025) */
int tamcmc_sampler_get_proposal(const tamcmc_sampler *s, int32_t m, double *mu, double *covarmat);
int tamcmc_sampler_set_proposal(tamcmc_sampler *s, int32_t m, const double *mu, const double *covarmat, double sigma);
/* The factor IN FORCE for chain m -- what the next proposal is drawn with (and, with use_drift = 1, what its two densities are taken with):
 * L [Nvars x Nvars], lower triangle, row-major, zeros above.  Both engines, any TAMCMC_OPT_FACTOR_REFRESH.  An audit entry like
 * tamcmc_sampler_draws.
 *
 * TAMCMC_OPT_FACTOR_REFRESH = R >= 2 (opt-in, read at creation): the proposal law of the learning phase.  mu, Sigma and sigma are
 * updated exactly as with R = 0 -- the same bits, clips included.  With g = c0 / (1 + i), sigma / sigma' the scale before / after its
 * update and d = x - mu', an adapting iteration is a RANK-ONE STEP iff it is not a scheduled full step (the k-th adapting iteration of
 * the sampler, k counted from 0, is full when k % R == 0), 0 < g < 1, the covariance was not rescaled to norm A1, and the chain's factor
 * is marked valid.  It replaces L in place by the Cholesky factor of
 *     beta^2 L L^T + w w^T,     beta^2 = (1 - g) sigma' / sigma,     w = sqrt(g sigma') d,
 * in O(Nvars^2).  Otherwise the step is FULL: L = chol((Sigma + eps2 I) sigma) as with R = 0, and the factor is marked valid iff that
 * matrix was positive definite (if not, the old factor stays in force, as with R = 0, and the next adapting iteration is full again).
 * A rank-one step whose pivots are not all finite and positive leaves the old factor in force and clears the mark.
 * The law: in exact arithmetic the factor in force satisfies  L L^T = sigma (Sigma + eps2 rho I),  rho = prod (1 - g_j) over the rank-one
 * steps since the last full step -- Sigma is exactly the default's, the regulariser decays until the next refresh.  It is a valid
 * adaptive law: the random walk is symmetric for any L, the Langevin densities are taken with the L that draws, and the drift stays the
 * deterministic function (1/2) sigma (Sigma + eps2 I) grad it is with R = 0.
 * Laws from outside: tamcmc_sampler_set_proposal (and through it tamcmc_sampler_read_restore with restore_proposal and
 * tamcmc_sampler_seed_proposal_fisher) clears the mark: the next adapting iteration is a full step.  A restored run therefore starts with a
 * full step and does NOT continue a rank-one run bit for bit (the restore file holds Sigma, not the factor with its decayed regulariser). */
int tamcmc_sampler_get_factor(const tamcmc_sampler *s, int32_t m, double *L);
/* The rank-one step alone, on the host (no device): L [Nvars x Nvars] lower triangular, row-major, replaced in place by the Cholesky
 * factor of beta2 L L^T + w w^T (zeros above the diagonal); the arithmetic of both engines (csrc/factor_update.h).  TAMCMC_ERR_BAD_ARG
 * (L untouched) for a non-finite input, beta2 <= 0 or a pivot that is not finite and positive. */
int tamcmc_factor_rank_one_update(int32_t Nvars, double *L /* lower, row-major, in place */, const double *w, double beta2);
/* Seeds every chain's proposal covariance from the curvature of the likelihood at the chain's CURRENT position (tamcmc_hip_fisher, one call
 * per chain with the steps h_k = hstep_rel max(|theta_k|, 1e-2); hstep_rel = 0 means 1e-6): with F_m the expected information at the chain's
 * temperature T_m and E = diag(init_errors),
 *   Sigma_m = E (I + E F_m E)^-1 E      ( = (F_m + E^-2)^-1, written so that a zero initial error or a variable without information is harmless:
 *                                         every eigenvalue of I + E F E is >= 1, and diag Sigma <= e^2 -- never wider than the default law).
 * The inverse is taken on the host from a Cholesky factor in long double; Sigma_m goes through tamcmc_sampler_set_proposal, so both
 * engines get it; mu and sigma are not touched.  F (may be NULL) receives the F_m, [Nchains x Nvars x Nvars].  Never called implicitly:
 * without it nothing changes.  Any failure (a refusal of tamcmc_hip_fisher, a table that fails at a perturbed point, a non-finite F)
 * returns the status and leaves every proposal law as it was.  Red giants (ids 25, 27): set TAMCMC_OPT_RGB_FISHER = 1 on the context
 * first (read at every call; with it at 0 this returns TAMCMC_ERR_BAD_MODEL); a variable whose step reaches across a change of the set
 * of mixed modes then takes the one-sided or the unfrozen form of the derivative (tamcmc_hip_fisher). */
int tamcmc_sampler_seed_proposal_fisher(tamcmc_sampler *s, double hstep_rel, double *F /* may be NULL, [Nchains x Nv x Nv] */);
/* The rule alone, on the host (no device): cov [Nvars x Nvars] = E (I + E F E)^-1 E for a symmetric F and E = diag(errors); symmetric bit
 * for bit.  TAMCMC_ERR_BAD_ARG for a non-finite entry or an F so far from positive semi-definite that I + E F E has no Cholesky factor. */
int tamcmc_fisher_seed_covariance(int32_t Nvars, const double *F, const double *errors, double *cov);
/* Chain positions vars [Nchains x Nvars] from outside (restart): priors and likelihoods are re-evaluated on the device;
 * iteration >= 0 also sets the iteration counter (the learning schedule and gamma = c0/(1+i) depend on it). */
int tamcmc_sampler_set_state(tamcmc_sampler *s, const double *vars, int64_t iteration);

/* ---- checkpoint / resume: the reference's restore files <root>1.dat (positions), <root>2.dat (sigmas, mus), <root>3.dat
 * (covariance matrices) -- Outputs::write_buffer_restore outputs.cpp:863-1025, Config::read_restore_files config.cpp:1734-1990.
 * Written with 17 significant digits (the reference: 6); the *_mean blocks repeat the last values. */
int tamcmc_outputs_write_restore(const char *root, int32_t Nchains, int32_t Nvars, int64_t iteration, const char *const *names,
                                 const double *vars, const double *sigmas, const double *mus, const double *covarmats);
/* sizes always; arrays (may be NULL): vars [Nchains x Nvars], sigmas [Nchains], mus [Nchains x Nvars], covarmats [Nchains x Nvars^2] */
int tamcmc_outputs_read_restore(const char *root, int32_t *Nchains, int32_t *Nvars, int64_t *iteration, double *vars, double *sigmas,
                                double *mus, double *covarmats);
int tamcmc_sampler_write_restore(const tamcmc_sampler *s, const char *root, const char *const *var_names);
/* the three switches of the reference's !Outputs section: do_restore_variables, do_restore_proposal, do_restore_last_index */
int tamcmc_sampler_read_restore(tamcmc_sampler *s, const char *root, int32_t restore_variables, int32_t restore_proposal,
                                int32_t restore_last_index);

/* ---- the reference's on-disk sample formats (outputs.cpp:1231-1333, :1472-1550) and summary statistics ---- */
/* <root>params.hdr + <root>params_chain-<m>.bin: raw little-endian doubles [sample][var]; samples = [n x Nchains x Nvars]
 * exactly as tamcmc_sampler_run returns them.  names (may be NULL) = Nparams parameter names for the header; plength has n_plength
 * entries (11 for the spectrum models of this build, 10 for the reference's Gaussian-envelope models).
 * append != 0: a later buffer of the same run -- the .bin files grow and, as in the reference (outputs.cpp:1268), the header is
 * rewritten with the cumulative `! Nsamples_done` (rows already on disk + n). */
int tamcmc_outputs_write_params(const char *root, const double *samples, int64_t n, int32_t Nchains, int32_t Nvars,
                                int64_t Nsamples_total, const int32_t *relax, const int32_t *plength, int32_t n_plength, int64_t Nparams,
                                const double *inputs, const char *const *names, int32_t append);
/* <root>stat_criteria.hdr/.bin: per sample logLikelihood[0:Nchains], logPrior[0:Nchains], logPosterior[0:Nchains];
 * stats = [n x Nchains x 3] as tamcmc_sampler_run returns them; append as above (outputs.cpp:1502). */
int tamcmc_outputs_write_stat_criteria(const char *root, const double *stats, int64_t n, int32_t Nchains, int32_t append);
/* <file>: the acceptance diagnostic the reference appends one line to per buffer (Outputs::write_txt_acceptance, outputs.cpp:747-790):
 * x = (Ncopy + 0.5) Nbuffer + Nsamples_init (the buffer's average sample index, outputs.cpp:1838) followed by acceptance_rate[0:Nchains-1]
 * streamed as an Eigen row (6 significant digits, columns padded to the widest entry).  first != 0 starts the file with its header. */
int tamcmc_outputs_write_acceptance(const char *file, double xaxis, const double *rates, int32_t Nchains, int32_t first);
/* reads it back: *Nchains from the header, then up to max_rows lines into xaxis [max_rows] and rates [max_rows x Nchains] (either may be
 * NULL to query *n_rows) */
int tamcmc_outputs_read_acceptance(const char *file, int32_t *Nchains, int64_t max_rows, int64_t *n_rows, double *xaxis, double *rates);
/* reads back one chain (what tools/bin2txt_params.cpp does): the header's Nsamples_done rows; samples may be NULL to query the count */
int tamcmc_outputs_read_params(const char *root, int32_t chain, double *samples, int64_t max_samples, int64_t *n_read,
                               int32_t *Nchains, int32_t *Nvars);
/* mean, median, population standard deviation per variable (tools/quick_samples_stats.cpp:4-35 via bin2txt_params.cpp:165-168);
 * samples rows are row_stride doubles apart */
int tamcmc_params_summary(const double *samples, int64_t n, int32_t Nvars, int64_t row_stride, double *mean, double *median,
                          double *stddev);

/* Evidence diagnostic of the tempered ladder (Diagnostics::evidence_calc, diagnostics.cpp:980-1019; quad_interpol, interpol.cpp:46-101):
 * beta = 1/Tcoefs, L_beta[m] = mean recorded log-likelihood of chain m, both resampled to interp_factor*Nchains points, evidence =
 * average of the resampled L_beta.  logL[i*row_stride + m*col_stride]: for tamcmc_sampler_run's stats block pass row_stride =
 * 3*Nchains, col_stride = 3.  beta_interp / L_beta_interp ([interp_factor*Nchains]) may be NULL. */
int tamcmc_evidence_calc(const double *Tcoefs, int32_t Nchains, const double *logL, int64_t n, int64_t row_stride, int64_t col_stride,
                         int32_t interp_factor, double *beta, double *L_beta, double *beta_interp, double *L_beta_interp, double *evidence);
/* appends one line (sample count, L_beta, evidence) to the text file the reference's diagnostics keep (diagnostics.cpp:1021-1066) */
int tamcmc_outputs_write_evidence(const char *file, int64_t n_samples, int32_t Nchains, const double *beta, const double *L_beta,
                                  int32_t interp_factor, double evidence, int32_t first);

/* Host log-prior of one parameter vector = Model_def::call_prior (model_def.cpp:421-464) for the model classes
 * io_MS_Global (2), io_local (3), io_asymptotic (4), priors_Kallinger2014_Gaussian (0) and priors_Harvey_Gaussian (1; classes 0 and 1
 * read neither plength nor extra_priors, which may be NULL): long double arithmetic, the reference's term order.  *status (may be NULL) receives
 * TAMCMC_ERR_BAD_MODEL for prior ids / model families this build does not carry. */
double tamcmc_log_prior(int prior_class, const double *params, int64_t Nparams, const int32_t *plength, const double *priors,
                        const int32_t *priors_switch, const double *extra_priors, int32_t n_extra, int32_t *status);

#ifdef __cplusplus
}
#endif
#endif
