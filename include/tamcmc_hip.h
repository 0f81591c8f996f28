/*
 * tamcmc_hip.h -- C ABI of the MI355X (gfx950) hot path of TAMCMC:
 *   per-chain Lorentzian-sum model over the power-spectrum bins
 *   -> chi^2(2 d.o.f.) log-likelihood reduction
 *   -> finite-difference gradient for the Langevin proposal.
 *
 * Plain C: opaque context, plain pointers and sizes, int status codes
 * (never exit()).  All pointers are HOST pointers unless a name ends in _dev.
 * One context per host thread / GPU; a context is not thread-safe.
 *
 * The reference (OthmanB/TAMCMC-C, paths relative to its root) has no FFI:
 * its boundary is the in-process call
 *     Model_def::generate_model(Data*, m, Tcoefs)      tamcmc/sources/model_def.cpp:466-482
 * made once per chain per iteration from
 *     MALA::update_position_MH                         tamcmc/sources/MALA.cpp:486-488
 * inside `#pragma omp parallel for` over chains        tamcmc/sources/MALA.cpp:648-668.
 * Each entry point below names the reference interface it replaces.
 * INTEGRATION.md shows the reference-side binding.
 */
#ifndef TAMCMC_HIP_H
#define TAMCMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- status codes ---------------- */
#define TAMCMC_OK 0
#define TAMCMC_ERR_HIP (-1)          /* a HIP runtime call failed (tamcmc_hip_last_error has the text) */
#define TAMCMC_ERR_EMPTY_WINDOW (-2) /* set_imin_imax: imax-imin<=0 (reference exits, build_lorentzian.cpp:650-665) */
#define TAMCMC_ERR_NAN_WINDOW (-3)   /* NaN width/splitting: no window regime applies (build_lorentzian.cpp:597-634) */
#define TAMCMC_ERR_BAD_MODEL (-4)    /* model id without a device table builder (model_def.cpp:352-385) */
#define TAMCMC_ERR_BAD_ARG (-5)
#define TAMCMC_ERR_NO_SPECTRUM (-6)
#define TAMCMC_ERR_NO_DEVICE (-7)    /* no HIP device: the product path has NO CPU fallback */

/* ---------------- model ids (Config/default/models_ctrl.list) ---------------- */
/* Gaussian-envelope background fits (ids 0, 1): the first fit of a star, over the whole spectrum -- background + Gaussian envelope of the
 * modes, no mode table.  Only through tamcmc_hip_loglike_params_batch and the tamcmc_hip_fd_gradient* entry points (plength is not read
 * and may be NULL); tamcmc_build_mode_table returns TAMCMC_ERR_BAD_MODEL.  Kernels: csrc/envelope.hip.
 *   id 0 params: [k_Agran, s_Agran, k_taugran, s_taugran, c_gran, a1, a2, k1, s1, c1, k2, s2, c2, N0, Amax, numax, sigma, mu_numax,
 *                 omega_numax] (19; omega_numax is read by the prior only)
 *   id 1 params: [H1, tc1, p1, H2, tc2, p2, B0, Amax, numax, Gauss_sigma] (10)
 * Known deviation from Kallinger et al. (2014), kept from the reference: the sinc^2 leakage filter eta^2 multiplies the Gaussian only.
 * The reference's `Power.cwiseProduct(eta_squared);` (noise_models.cpp:150) discards its result, so the noise terms are not filtered.
 * One arithmetic mode for both (TAMCMC_OPT_PRECISION does not apply): double per bin, power laws as exp(c (ln x - ln b)) on the resident
 * ln x, the three normalisation integrals of id 0 as fixed-order tree sums.  Stated tolerance against a long-double restatement of the
 * reference: |dM|/M <= 1e-12 per bin, |dlogL|/|logL| <= 1e-12 (tests/test_gpu_envelope.py).  A vector's logL is bit-identical in any
 * batch at any position. */
#define TAMCMC_MODEL_KALLINGER2014_GAUSSIAN 0 /* model_Kallinger2014_Gaussian, models.cpp (after model_Harvey_Gaussian); prior class 0 */
#define TAMCMC_MODEL_HARVEY_GAUSSIAN 1        /* model_Harvey_Gaussian, models.cpp:5674; prior class 1 */
#define TAMCMC_MODEL_MS_GLOBAL_A1ETAA3_CLASSIC 3 /* model_MS_Global_a1etaa3_HarveyLike_Classic, models.cpp:1943 */
#define TAMCMC_MODEL_MS_LOCAL_BASIC 11           /* model_MS_local_basic, models.cpp:3012 */
/* Height-per-m models (ids 12, 13, 14): no stellar inclination; the heights of the 2l+1 components are read from the parameter
 * vector, mirrored around m = 0.  Frequencies, widths and windows are those of id 3 (ids 12, 13) / of id 11 with a1 = |p[o_split]|
 * and no sqrt(a1) cos/sin form (id 14).  With o_inc = the first index of the "inclination" block (after the noise block):
 *   id 12  Ninc = 9 ratios shared by all orders: hv = H_l * |p[o_inc + {1,0,1}]|, |p[o_inc + {4,3,2,3,4}]|, |p[o_inc + {8,7,6,5,6,7,8}]|
 *          for l = 1, 2, 3 with H_l exactly as in id 3 (visibilities included) -- with ratios = amplitude_ratio(l, i) the rows are
 *          bit-identical to id 3's.  Prior: io_MS_Global with extra_priors[8] = 1 (the three sums of ratios in [0, 1 + 1e-10]).
 *   id 13  one height per (n, l, |m|), no visibilities: hv = |p[o_inc + (l+1) n + |m|] / (pi W)| (|p[..]| without do_amp).
 *   id 14  local: heights of l = 0 at p[n], of l >= 1 at p[off_l + (l+1) n + |m|] with off_l = Nfl0 + .. + Nfl(l-1);
 *          plength[0] = Nfl0 + 2 Nfl1 + 3 Nfl2 + 4 Nfl3, Nharvey = 0.  Prior: io_local unchanged (no normalisation: the block of
 *          priors_local that would apply one is commented out in the reference, priors_calc.cpp:575-613).
 * Known quirk, kept from the reference (ids 13 and 14): the loaders lay the l >= 1 heights out l-major -- degree l starts after
 * the 2 Nfl1 (+ 3 Nfl2) entries of the lower degrees -- but the model functions count every degree's offset (l+1) n from the START of
 * the block (id 13, models.cpp:2427-2477) or from Nfl0 + Nfl1 (+ Nfl2) (id 14, models.cpp:3261-3316), so for l >= 2 they read inside the
 * l = 1 heights.  The table builders read what the reference's model functions read; a star with l <= 1 is unaffected.
 * For l >= 1 the amplitude conversion divides in double by the double-rounded product pi W (an Eigen vector divided by a scalar),
 * where l = 0 and ids 3, 11 divide in long double.
 * The reference's `params.model` side output (outparams = true) does not exist for these three: it exits there.  The row-writing
 * entries are unaffected.  Id 13 has no prior the reference can run (its loader sets extra_priors[8] = 2, where priors_MS_Global
 * exits): it is served at the model level only -- tables, likelihood, gradient -- and has no loader or sampler.
 * A layout whose height block is shorter than what the model function reads is refused with TAMCMC_ERR_BAD_MODEL. */
#define TAMCMC_MODEL_MS_GLOBAL_A1ETAA3_CLASSIC_V2 12 /* model_MS_Global_a1etaa3_HarveyLike_Classic_v2, models.cpp:2128 */
#define TAMCMC_MODEL_MS_GLOBAL_A1ETAA3_CLASSIC_V3 13 /* model_MS_Global_a1etaa3_HarveyLike_Classic_v3, models.cpp:2338 */
#define TAMCMC_MODEL_MS_LOCAL_HNLM 14                /* model_MS_local_Hnlm, models.cpp:3198 */
#define TAMCMC_MODEL_MS_GLOBAL_AJ 23             /* model_MS_Global_aj_HarveyLike, models.cpp:1195 */
#define TAMCMC_MODEL_RGB_ASYMPT_AJ_APPWIDTH_V4 25 /* model_RGB_asympt_aj_AppWidth_HarveyLike_v4, models.cpp:4684: through
                                                    tamcmc_hip_loglike_params_batch and the tamcmc_hip_fd_gradient* entry points
                                                    (its table needs the device pre-step: ARMM mixed-mode solver + zeta function,
                                                    csrc/rgb_prestep.hip; tamcmc_build_mode_table: TAMCMC_ERR_BAD_MODEL) */
#define TAMCMC_MODEL_RGB_ASYMPT_AJ_CTEWIDTH_V4 27 /* model_RGB_asympt_aj_CteWidth_HarveyLike_v4, models.cpp:4334: same path, one
                                                    constant width for the l=0,2,3 modes */

/* ---------------- arithmetic modes ---------------- */
/* STRICT: per-bin operation order of the reference (IEEE divides, no FMA contraction): the model row is
 *         bit-identical to the CPU restatement when the Harvey pow() terms are inactive.
 * FAST  : same function, re-associated (common-denominator multiplet sum, reciprocal+Newton, exp/log Harvey) and,
 *         for multiplets far from a tile, summed as ONE degree-15 polynomial per tile.  A multiplet is far when its window
 *         covers the tile and rho = beta / sqrt(A_m^2 + 1) <= 1/6 for every component (1/8 for a multiplet with asymmetry;
 *         beta = tile half-width x 2/gamma, A_m = (nu_m - tile centre) x 2/gamma).  Stated tolerance, per bin:
 *             FAST_DIRECT  |dM| <= 1e-12 M
 *             FAST         |dM| <= 1e-12 M + tau_far F(x) + tau_asym F_asym(x)
 *         with F (F_asym) the sum of the far components without (with) asymmetry at the bin.  tau_far = rho^16 (17 + 16 rho) at
 *         rho = 1/6 = 6.96e-12: in its wing a Lorentzian is a DOUBLE pole, hv / (A^2 (1 - rho s)^2), whose series loses
 *         rho^n (n + 1 + n rho) of the term after n coefficients (reached at the gate when the tile lies deep in the wing of one
 *         component; the simple-pole figure 6^-16 / (1 - 1/6) = 4e-13 quoted here before omitted the factor 17).  tau_asym =
 *         2.8e-12, four times the measured worst case (the asymmetry factor can come close to zero on a tile far from nu_c, and
 *         relative to the term the coefficients' rounding then counts; 3.6e-15 at the tile centre).  The background joins the
 *         polynomial on tiles where its series keeps 2.3e-13 of every Harvey term (csrc/bg_series.h), inside the 1e-12 M.
 *         |dlogL|/|logL| <= 1e-11 in both FAST modes.  Pinned by tests/test_tile_bounds.py (CPU, against a 50-digit reference)
 *         and tests/test_gpu_tile_reference.py. */
#define TAMCMC_PRECISION_STRICT 0
#define TAMCMC_PRECISION_FAST 1        /* far-field expansion per tile + direct near field */
#define TAMCMC_PRECISION_FAST_DIRECT 2 /* FAST arithmetic, every component evaluated per bin (no far field) */

#define TAMCMC_OPT_PRECISION 1   /* value: TAMCMC_PRECISION_* (default STRICT) */
#define TAMCMC_OPT_TIMING 2      /* value: 0/1 -- bracket the likelihood kernel with HIP events on the context stream */
#define TAMCMC_OPT_BINS_PER_THREAD 3 /* value: 1,2,4 (workgroup 256) or 4,8,16 (workgroup 64) -- tile = workgroup*value bins */
#define TAMCMC_OPT_FD_WINDOWED 5     /* value: 0/1 -- FAST modes: FD gradients from delta tables (only the multiplets a perturbation
                                        changes, on their windows, against the stored base model row); default 1 */
#define TAMCMC_OPT_WORKGROUP 4       /* value: 256 (four waves share a tile) or 64 (one wave per tile); resets bins per thread */
#define TAMCMC_OPT_STEP_SCHEME 6     /* device-resident sampler: 0 = automatic (fused launches wherever no adaptation separates two
                                        iterations -- one launch per iteration, or one per chain group on two streams once a launch no
                                        longer fits the GPU's resident waves -- lockstep kernels elsewhere), 1 = lockstep kernels only,
                                        2 = fused with one launch per iteration, 3 = fused with two chain groups whenever there are
                                        8 chains or more.  Same chains bit for bit in every case (tests/test_gpu_sampler.py); default 0 */
#define TAMCMC_OPT_QUICK_DECIDE 8    /* a test facility of the fused step.  Its likelihood tiles learn the outcome of the previous
                                        iteration's Metropolis test and swap from a threshold comparison with a 1e-11 safety margin and
                                        fall back to the exact evaluation when the comparison is too close (about once in 1e5 tests).
                                        0 = that (default); 1 = the margin is +inf: every margin test answers "undecided" and every
                                        test takes the fallback (records of proposals that cannot be accepted keep deciding without
                                        sums).  Same chains bit for bit, several times slower; tamcmc_sampler_get_info counts the
                                        fallbacks taken (TAMCMC_INFO_QUICK_FALLBACKS) */
#define TAMCMC_OPT_ARMM_DENSE_SCAN 7 /* red-giant pre-step: 1 = walk the solver's whole grid like the reference (solver_mm.cpp:340-377)
                                        instead of the pole-structured scan that finds the same cells; default 0 */

#define TAMCMC_OPT_GRADIENT 9        /* value: TAMCMC_GRADIENT_* -- how the gradient batches (tamcmc_hip_fd_gradient*, both samplers' Langevin
                                        step) obtain the likelihood's share; see tamcmc_hip_adjoint_table.  Default TAMCMC_GRADIENT_FD */
#define TAMCMC_GRADIENT_FD 0         /* finite differences: Nvars perturbed likelihoods per chain (windowed or brute force) */
#define TAMCMC_GRADIENT_ADJOINT 1    /* table-space adjoint with frozen windows: one pass over the bins per chain, whatever Nvars is */

#define TAMCMC_OPT_FISHER_WORKSPACE_MB 10 /* value: MiB (>= 1, default 2048) of model rows tamcmc_hip_fisher keeps on the device per pass: a chain
                                        takes 2 Nvars Nx 8 bytes, as many chains per pass as fit, a single chain above the budget still
                                        runs alone.  The result does not depend on it */
#define TAMCMC_OPT_RGB_DEVICE_LANGEVIN 11 /* value: 0/1 (default 0) -- 1: tamcmc_sampler_create builds the device-resident engine's Langevin
                                        sampler (engine = 1, use_drift = 1) for the red-giant models, ids 25 and 27; 0: it refuses them
                                        with TAMCMC_ERR_BAD_MODEL.  Read when the sampler is created: changing it afterwards does not
                                        affect an existing sampler.  FAST arithmetic; TAMCMC_GRADIENT_FD, or TAMCMC_GRADIENT_ADJOINT with
                                        TAMCMC_OPT_RGB_ADJOINT = 1 (tamcmc_sampler.h) */
#define TAMCMC_OPT_RGB_ADJOINT 12     /* value: 0/1 (default 0) -- 1: with TAMCMC_OPT_GRADIENT = TAMCMC_GRADIENT_ADJOINT the red-giant models, ids 25
                                        and 27, take the hybrid adjoint batch (see tamcmc_hip_adjoint_table) instead of being refused.  Read at
                                        every call, like TAMCMC_OPT_GRADIENT; nothing else changes with it.  Any other value: TAMCMC_ERR_BAD_ARG */
#define TAMCMC_OPT_ENVELOPE_DEVICE_ENGINE 13 /* value: 0/1 (default 0) -- 1: tamcmc_sampler_create builds the device-resident engine (engine = 1,
                                        use_drift = 0) for the Gaussian-envelope models, ids 0 and 1; 0: it refuses them with
                                        TAMCMC_ERR_BAD_MODEL.  Read when the sampler is created: changing it afterwards does not affect an
                                        existing sampler.  It admits use_drift = 0 only: the Langevin step of these ids on the device-resident
                                        engine has its own option, TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN, and neither implies the other; see
                                        tamcmc_sampler.h.  Any other value: TAMCMC_ERR_BAD_ARG */
#define TAMCMC_OPT_FACTOR_REFRESH 14 /* value R: 0 (default) or 1 -- every adapting iteration factors (Sigma + eps2 I) sigma from scratch; 2 ... 65536 --
                                        the factor follows the Robbins-Monro step by a rank-one update in O(Nvars^2), with a scheduled full
                                        factorisation every R-th adapting iteration (both engines, both samplers, every model; the law and
                                        the rule: tamcmc_sampler.h).  Read when the sampler is created: changing it afterwards does not
                                        affect an existing sampler.  Any other value: TAMCMC_ERR_BAD_ARG */
#define TAMCMC_OPT_ENVELOPE_GRADIENT 15 /* value: 0/1 (default 0) -- 1: for the Gaussian-envelope models, ids 0 and 1, tamcmc_hip_fd_gradient and
                                        tamcmc_hip_fd_gradient_posterior (and with them the host engine's Langevin step) take the
                                        likelihood's share from the analytic gradient, one pass over the bins per chain instead of
                                        Nvars + 1 (see tamcmc_hip_envelope_gradient_sums).  Read at every call.  hstep is still required: it
                                        sets the prior's forward and backward points and is not read by the likelihood's share.
                                        TAMCMC_GRADIENT_ADJOINT keeps refusing these ids.  The option concerns these host routes only: the
                                        device-resident engine's Langevin step (TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN) has one gradient route,
                                        the analytic one, and does not read it.  Any other value: TAMCMC_ERR_BAD_ARG */
#define TAMCMC_OPT_RGB_FISHER 16     /* value: 0/1 (default 0) -- 1: tamcmc_hip_fisher (and with it tamcmc_sampler_seed_proposal_fisher) accepts the
                                        red-giant models, ids 25 and 27, on a FAST or FAST_DIRECT context; 0: it refuses them with
                                        TAMCMC_ERR_BAD_MODEL, whatever TAMCMC_OPT_RGB_ADJOINT says.  Read at every call; nothing else
                                        changes with it.  Any other value: TAMCMC_ERR_BAD_ARG */
#define TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN 17 /* value: 0/1 (default 0) -- 1: tamcmc_sampler_create builds the device-resident engine's Langevin
                                        sampler (engine = 1, use_drift = 1) for the Gaussian-envelope models, ids 0 and 1; 0: it refuses
                                        them with TAMCMC_ERR_BAD_MODEL, whatever TAMCMC_OPT_ENVELOPE_DEVICE_ENGINE says.  Independent of that
                                        option: 13 admits use_drift = 0, 17 admits use_drift = 1.  Read when the sampler is created: changing
                                        it afterwards does not affect an existing sampler.  One gradient route, the analytic gradient with
                                        its chain rule on the device in double (tamcmc_sampler.h); TAMCMC_OPT_ENVELOPE_GRADIENT and
                                        TAMCMC_OPT_PRECISION are not read.  Any other value: TAMCMC_ERR_BAD_ARG */
#define TAMCMC_FISHER_SLAB 2048     /* bins per workgroup (and per partial matrix) of the Gram kernel of tamcmc_hip_fisher / _weighted_gram */

/* One (n,l) multiplet: <=7 Lorentzian m-components on its truncation window.
 * This is the flat "mode table" row every Lorentzian model of the dispatch table reduces to
 * (build_lorentzian.cpp:131-161, :208-246).  152 bytes, no padding. */
typedef struct tamcmc_multiplet {
    int32_t l;      /* degree 0..3 -> 2l+1 components */
    int32_t i0;     /* first bin of the window (set_imin_imax, build_lorentzian.cpp:645-649) */
    int32_t i1;     /* one past the last bin */
    int32_t flags;  /* reserved, 0 */
    double fc;      /* central frequency nu_c (asymmetry reference, build_lorentzian.cpp:240) */
    double gamma;   /* width */
    double asym;    /* asymmetry coefficient (0 = symmetric Lorentzian) */
    double nu[7];   /* nu_nlm for m=-l..l */
    double hv[7];   /* H_l * V_m */
} tamcmc_multiplet;

typedef struct tamcmc_hip_ctx tamcmc_hip_ctx;

/* ---------------- context ---------------- */
int tamcmc_hip_create(tamcmc_hip_ctx **ctx, int device);
void tamcmc_hip_destroy(tamcmc_hip_ctx *ctx);
const char *tamcmc_hip_last_error(const tamcmc_hip_ctx *ctx);
int tamcmc_hip_set_option(tamcmc_hip_ctx *ctx, int option, int64_t value);
const char *tamcmc_hip_version(void);

/* Page-locked host memory for buffers the library copies results into (recorded samples and statistics of tamcmc_sampler_run): any
 * host pointer works there, a pinned one is filled by an asynchronous DMA instead of a staged copy.  NULL on failure. */
void *tamcmc_hip_host_alloc(size_t bytes);
void tamcmc_hip_host_free(void *p);

/* Replaces the shared read-only `Data{x,y,Nx}` (tamcmc/headers/data.h:23-34) every chain reads:
 * uploads the spectrum once; it stays resident in HBM. x must be a regular grid (build_lorentzian.cpp:645). */
int tamcmc_hip_set_spectrum(tamcmc_hip_ctx *ctx, const double *x, const double *y, int64_t Nx);

/* Replaces, for B parameter vectors at once, the per-bin work of
 *   call_model  (model_def.cpp:220-388 -> optimum_lorentzian_calc_* + harvey_like, noise_models.cpp:15-39)
 *   call_likelihood (model_def.cpp:390-419 -> likelihood_chi22p, likelihoods.cpp:17-28).
 * mults[offsets[b] .. offsets[b+1]) are evaluation b's multiplets in the reference's accumulation order;
 * noise + b*noise_stride = the nnoise[b] values |noise params| = [H0,tau0,p0, H1,tau1,p1, ..., N0] of evaluation b:
 * nharvey[b] Harvey triples are applied (noise_models.cpp:29-36), the white noise N0 is the LAST of the nnoise[b] entries;
 * Tcoefs[b] = temperature (NULL -> 1); p = likelihood_params truncated to long.
 * Out: logL[b] = -p * sum_i(y_i/M_i + ln M_i) / Tcoefs[b]; model (may be NULL) = B x Nx rows.
 * A non-finite model gives a NaN/inf logL that the caller rejects (MALA.cpp:490,522-524). */
int tamcmc_hip_loglike_batch(tamcmc_hip_ctx *ctx, int B, const tamcmc_multiplet *mults, const int32_t *offsets,
                             const double *noise, int noise_stride, const int32_t *nharvey, const int32_t *nnoise,
                             const double *Tcoefs, double p, double *logL, double *model);

/* Table builders (Lorentzian models only; ids 0 and 1 have no multiplets: TAMCMC_ERR_BAD_MODEL): the host-side scalar part of the model functions
 *   VectorXd model_X(params, params_length, x, outparams)   tamcmc/headers/models.h:21-57
 * (parameter unpack, amplitude_ratio, lin_interpol, eta0, set_imin_imax) for ids 3, 11, 12, 13, 14, 23.
 * Writes at most max_mults rows; *n_mults = rows needed.  noise_abs receives |noise params| (plength[8] values). */
int tamcmc_build_mode_table(int model_id, const double *params, const int32_t *plength, const double *x, int64_t Nx,
                            tamcmc_multiplet *mults, int max_mults, int *n_mults, double *noise_abs,
                            int *nharvey, int *nnoise);

/* model id + params level: table build on the host for each of the B vectors, then one batched device call.
 * This is the batched body of Model_def::generate_model without the prior (model_def.cpp:473-474).
 * status (may be NULL) receives the per-vector table status; vectors with a failed table get logL = NaN.
 * Ids 0 and 1 are dispatched first, before plength is read: see the model ids above (at most 65535 vectors per call). */
int tamcmc_hip_loglike_params_batch(tamcmc_hip_ctx *ctx, int model_id, int B, const double *params, int64_t Nparams,
                                    const int32_t *plength, const double *Tcoefs, double p, double *logL,
                                    double *model, int32_t *status);

/* Red-giant tolerance (ids 25, 27; every arithmetic mode).  The reference evaluates the mixed-mode relation on its grids in double
 * (Eigen arrays, solver_mm.cpp:158-169, called at :356-358 and :382-383) and the intersection test in long double (:179-186, :389-404); the device pre-step uses double
 * throughout, the oracle long double throughout.  Stated: mixed-mode frequencies within 1e-10 muHz and zeta within 1e-9 of the oracle's,
 * model rows ||dM||_2 / ||M||_2 <= 1e-10, |dlogL| / |logL| <= 1e-11 (STRICT) / the FAST tolerance above (FAST).  Measured on MI355X
 * (tools/rgb_parity_probe.py, round 3): frequencies <= 3e-13 muHz (1.5e-11 at 2e5 bins with ~170 mixed modes), zeta <= 4e-13 (1.2e-10),
 * rows <= 2e-12 (1.1e-11), logL <= 1e-14.  A mixed mode is as narrow as 0.01 muHz, so a frequency error d nu moves single bins of its
 * profile by ~d nu / Gamma: the per-bin maximum is larger than the row norm (5e-12 typical, 5.5e-10 at the C5 size).
 * Against the DEFINITION (tests/rgb_reference.py: the same statements at 50 digits, every value with the scale a double evaluation's
 * rounding is proportional to): every mixed-mode frequency, zeta, h1_h0 and every row field of tamcmc_hip_rgb_mixed_modes and
 * tamcmc_hip_rgb_batch_tables (STRICT and FAST) lies within 4 x 2^-52 x scale -- ~1e-12 muHz for a frequency near 120 muHz -- and l, flags,
 * row count and order, nharvey, nnoise, status, i0 and i1 are the definition's.  The point count of the solver's local grid,
 * long(4 resol / (resol factor)), is an exact integer that a double evaluation rounds to itself or to one less: the definition carries
 * both results and a root must be one of the two.  Measured on the MI355X: worst ratio 0.6 of the permitted 4.
 *
 * Red-giant models (ids 25, 27): the l=1 mixed modes of ONE parameter vector as the device pre-step computes them for the table
 * (csrc/rgb_prestep.hip) -- what external/ARMM/do_solve.cpp:114-121 prints with the reference's solver:
 *   nu_m  = solve_mm_asymptotic_O2p / _O2from_l0 (solver_mm.cpp:470-760, chosen by the vector's model_type) + the spline bias,
 *   zeta  = ksi_fct2(nu_m, ..., "precise") (bump_DP.cpp:125-188),  h1_h0 = h_l_rgb(zeta, Hfactor) (bump_DP.cpp:235-254).
 * The solver's step is the spectrum's resolution x[2]-x[1] (models.cpp:4719).  Any of nu_m / zeta / h1_h0 ([max_modes]) may be NULL;
 * *n_modes = number of mixed modes found. */
int tamcmc_hip_rgb_mixed_modes(tamcmc_hip_ctx *ctx, int model_id, const double *params, int64_t Nparams, const int32_t *plength,
                               int max_modes, double *nu_m, double *zeta, double *h1_h0, int *n_modes);

/* Forward-difference gradient of the tempered logL (the drift MALA::D_MALA leaves as a stub, MALA.cpp:321-328):
 * for each of the C chains, Nvars+1 evaluations in ONE batched launch.
 * params: C x Nparams; index_to_relax: Nvars parameter indices (model_def.cpp:76-90); hstep: Nvars steps.
 * Out: logL0[C], grad[C x Nvars] = (logL(theta + h e_k) - logL(theta)) / h_applied.
 * Tolerance (FAST arithmetic, windowed differences: TAMCMC_OPT_FD_WINDOWED): the difference is formed term by term against the stored
 * base point -- per bin as the series in u = dM/M0 (five terms, closed form beyond |u| = 0.01), and on tiles where every changed
 * multiplet is in the far field from moments of the base point (first and second order in u; used where max|u| <= 1e-5, what is
 * omitted is below 1e-10 of the leading term).  Per slot, the un-tempered difference dS = grad h_applied T / (-p) is within
 * truncation (first omitted term of the series / of the moment form, per bin) + far-field truncation (tau(rho, n) of each far delta
 * row's own rho, TAU_ASYM with asymmetry, the background series' budget for a changed noise row) + 332 x 2^-53 sum_i w_i A_i (w_i =
 * |1 - y_i/M0_i| / M0_i, A_i = the absolute values summed into dM_i) + 1e-12 sum_i |f_i| of the exact difference of the two tables the batch
 * built (tests/delta_reference.py derives each part; tests/test_gpu_delta_reference.py).  Against the brute-force
 * difference of two full evaluations it agrees to that
 * difference's own cancellation noise (~5e-15 Nx / h) + 1e-6 of the gradient's scale (tests/test_gpu_parity.py).
 * Ids 0 and 1: every parameter moves every bin, so the batch is brute force -- C x (Nvars+1) full evaluations in one batched launch
 * (C x (Nvars+1) <= 65535), grad = (logL(theta + h e_k) - logL(theta)) / h_applied; plength is not read.
 * Ids 25 and 27 (red giants): each of the C x (Nvars+1) <= 65535 vectors goes through the device pre-step (scalar unpack beside the prior in
 * the batch's first kernel, then mixed-mode solver, zeta and rows), in chunks when their workspace (~28 KB per vector) would pass 256 MiB;
 * one likelihood launch over all tables (brute force: STRICT always, FAST with TAMCMC_OPT_FD_WINDOWED = 0) or the windowed pipeline above
 * (FAST, the default: at the C5 shape, 2e5 bins x 40 chains x 62 vectors, 8.2 ms against 10.4 ms brute force and 19.3 ms for the same vectors
 * through 62 tamcmc_hip_loglike_params_batch calls), where a perturbation that moves the mixed modes (period spacing, coupling, large separation, rotation, ...) is a
 * "full table" evaluation.  A perturbation may change the NUMBER of mixed modes; the tables are then compared row against absent row.
 * A vector the pre-step refuses (a negative large separation, more than 400 mixed modes, ...) makes the call return that status with
 * grad = NaN for this component (logL0 = NaN when it is the base point); the other components are unaffected.
 * Tolerance: the red-giant tolerance above carries into the differences -- each of the two log-likelihoods is within tol of the oracle's, so
 * |d grad| <= 2 tol |logL| / h with tol = 1e-11 (STRICT) / the FAST tolerance; windowed against brute force as for the other models.
 * STRICT: the scalar unpack of the vectors is the host's, in long double like the reference's, so logL0 and every difference are the very
 * bits of tamcmc_hip_loglike_params_batch on the same vectors.  FAST modes: the unpack runs on the device in double and agrees with that
 * entry to rounding (a few ulp of logL), not bit for bit (tests/test_gpu_rgb_gradient.py). */
int tamcmc_hip_fd_gradient(tamcmc_hip_ctx *ctx, int model_id, int C, const double *params, int64_t Nparams,
                           const int32_t *plength, const int32_t *index_to_relax, int Nvars, const double *hstep,
                           const double *Tcoefs, double p, double *logL0, double *grad);

/* Same batch, gradient of the tempered log-POSTERIOR: each of the C*(Nvars+1) workgroups also evaluates the log-prior of
 * its perturbed vector on the device (prior_class 2 = io_MS_Global, 3 = io_local, 4 = io_asymptotic with model ids 25 / 27 and only
 * with them -- generic terms one per lane, constraints and the ordered sum by one lane, in double --, 0 = priors_Kallinger2014_Gaussian
 * with model id 0, 1 = priors_Harvey_Gaussian with model id 1 -- these two on the device in double, one thread per point, extra_priors
 * not read; any other pairing: TAMCMC_ERR_BAD_MODEL;
 * priors = 4 x Nparams row-major table,
 * priors_switch = primitive ids, extra_priors[10]: Input_Data of tamcmc/headers/data.h:51-62).  Where the forward point
 * leaves a prior's support the backward difference of the prior is used, else that prior term is flat.
 * A prior that tamcmc_log_prior refuses -- a primitive id without an implementation (3, 9, 11, 12), impose_normHnlm = 2, model_index
 * 0..8 -- is refused here with the same status, TAMCMC_ERR_BAD_MODEL, for every prior class: the evaluation's slot fails like one whose
 * table failed and the call returns the status; it is never reported as TAMCMC_OK with a log-prior of -inf.
 * Out: logL0[C] (tempered), logPr0[C] (may be NULL), grad[C x Nvars], grad_prior[C x Nvars] (may be NULL: the prior's
 * share of grad, so that a caller can re-temper the likelihood share after a parallel-tempering swap). */
int tamcmc_hip_fd_gradient_posterior(tamcmc_hip_ctx *ctx, int model_id, int prior_class, int C, const double *params,
                                     int64_t Nparams, const int32_t *plength, const int32_t *index_to_relax, int Nvars,
                                     const double *hstep, const double *Tcoefs, double p, const double *priors,
                                     const int32_t *priors_switch, const double *extra_priors, double *logL0, double *logPr0,
                                     double *grad, double *grad_prior);

/* Adjoint gradient (TAMCMC_OPT_GRADIENT = TAMCMC_GRADIENT_ADJOINT).  Every parameter of a Lorentzian model reaches the sum
 * S = sum_i (y_i / M_i + ln M_i) only through the mode table and the noise row, so the likelihood's share of the gradient is
 *   dS/dtheta_k = sum_rows sum_f G[row][f] dT[row].f/dtheta_k + sum_j Gn[j] d|noise_j|/dtheta_k,   f in {nu[7], hv[7], gamma, asym, fc}.
 * G and Gn (the "table-space adjoint") are taken in ONE pass over the bins of the base point: G[row][f] = sum_i r_i dM_i/df over the row's
 * own window [i0, i1), Gn[j] = sum_i r_i dN_i/d|noise_j| over all bins, r_i = (1/M_i)(1 - y_i/M_i).  The table Jacobian is the forward
 * difference of the tables the batch's first kernel builds at theta + hstep[k] e_k anyway; hstep also still serves the prior's forward and
 * backward differences, which are untouched.  No perturbed likelihood is evaluated.
 * "Frozen window": the reference truncates each multiplet to a window of bins that depends on its frequency and width; a step that carries
 * a window edge across a bin makes a finite difference jump by that bin's whole term.  The adjoint differentiates with every window held at
 * the base point's [i0, i1) -- the windows of the perturbed tables are not read -- which is the exact derivative of the truncated model
 * wherever that derivative exists: no jumps, no cancellation noise.
 * With the option set, tamcmc_hip_fd_gradient, tamcmc_hip_fd_gradient_posterior, the host engine's Langevin step and the device engine's all
 * take this route (same signatures, same outputs; logL0 is the windowed route's bit for bit, the prior's share the finite-difference
 * route's bit for bit).  Models: the fixed-length table models, ids 3, 11, 12, 13, 14, 23; ids 0, 1 (no table) and 25, 27 (tables of
 * variable length) return TAMCMC_ERR_BAD_MODEL.  Arithmetic: FAST or FAST_DIRECT (the pass reads the planes 1/M0 and y/M0 that the FAST
 * base launch leaves), any workgroup geometry; STRICT returns TAMCMC_ERR_BAD_ARG.
 * Tolerance: each G[row][f] / Gn[j] within 1e-11 sum_i |r_i dM_i/df| of a long-double evaluation of the same sum (the FAST tolerance,
 * applied to this sum); the gradient within 3 R of the central difference with frozen windows, R that reference's own uncertainty
 * |g(h) - g(h/2)| (tests/test_gpu_adjoint.py).  The contraction itself is exact to rounding: with dT the differences of the batch's own
 * tables (tamcmc_hip_fd_batch_tables) and G, Gn the bits of the audit entry below, the dS of a component lies within
 *   D 2^-53 sum |G . dT| + 3 x 2^-53 |dS|,   D = 2 + 17 + ceil(rows / 64) + 6 + nnoise,
 * of the exact sum G . dT -- D the roundings one term can pass (difference, product, the row's running sum, the lane's row loop, the
 * wave's tree, the noise tail), the 3 those of the division by T and by h_applied (tests/test_gpu_adjoint_exact.py, which also holds G
 * and Gn to the 1e-11 above against a 50-digit evaluation that differentiates in field space).  Every sum has one fixed order: two calls
 * give the same bits, and a chain's gradient does not depend on the number of chains or on its place in the batch.
 * At a base point with asym = 0 the rows carry no asym and fc entries (the model takes its A = 1 branch there), so on this route the
 * likelihood's share of the asymmetry parameter's component is exactly 0, although dM/dasym = 2 u sum_m hv_m / q does not vanish at
 * asym = 0: the finite-difference route, which evaluates the model at asym = hstep, reports it.  The two routes differ in this component.
 *
 * The audit entry: G [C x *nrows x 17] and Gn [C x max(plength[8], 1)] of the C parameter vectors, for the UN-tempered S (Tcoefs and p are
 * accepted for symmetry and not read: logL = -p S / T).  *nrows = rows per table.  Runs under the adjoint route whatever the option says;
 * entries of rows a table does not have, of components m >= 2l+1 and, where asym = 0, of asym and fc are 0.  A vector whose table fails
 * makes the call return that status; its G and Gn are 0.  G, Gn, nrows may be NULL.
 *
 * Red giants (ids 25, 27) with TAMCMC_OPT_RGB_ADJOINT = 1: the HYBRID batch.  A red-giant table is the l=0 list, the l=1 mixed modes in
 * frequency order, then the l=2 and l=3 lists, and a perturbation may change the set of mixed modes: every later row then shifts and a
 * row-by-row contraction means nothing.  So every perturbed slot is classified on the device (csrc/adj_rgb_match.h).  It is LINEARISABLE
 * when its status and the base's are TAMCMC_OK, it has the base table's row count, every row has the base row's l, and every l=1 row's fc
 * lies within half the distance from the base row's fc to that row's nearest l=1 neighbour in the base table (a set that lost one mode and
 * gained another keeps its count and fails this).  A linearisable slot's difference is the contraction above; every other slot with two valid
 * tables is a FALLBACK slot and takes the windowed finite difference (tamcmc_hip_fd_gradient: delta table against the stored base point),
 * bit for bit what the windowed route gives for that component; a slot with a failed table gives NaN and the status, as there.  The base
 * launch is the windowed route's: logL0 is its bits, and the prior's share is the finite-difference route's bits.  Same determinism as
 * above.  FAST or FAST_DIRECT with a workgroup geometry that has the windowed route (256 x 4, 64 x 8, 64 x 4: others return
 * TAMCMC_ERR_BAD_ARG); STRICT returns TAMCMC_ERR_BAD_ARG; tamcmc_hip_fisher does not read this option (its own is
 * TAMCMC_OPT_RGB_FISHER).  With the option at 0 the ids are refused as before.
 * Tolerance of a linearisable component: G and Gn as above, within 1e-11 of their absolute sums A, An, carried through the contraction with
 * the batch's own tables (tamcmc_hip_rgb_batch_tables):
 *   |d grad_k| <= (p/T)/|h_applied| 1e-11 [sum_rows sum_f A[row][f] |dT[row].f| + sum_j An[j] |d noise_j|];
 * the tables themselves carry the red-giant tolerance above.  The forward table Jacobian adds the curvature of the mixed-mode frequencies
 * in the period spacing, the coupling and the large separation: against the frozen-window central difference the gradient lies within
 * 3 R + J, R that reference's |g(h) - g(h/2)| and J the distance between the adjoint with the forward and with the central table Jacobian
 * (tests/test_gpu_rgb_adjoint.py; sizes in DESIGN section 9).
 * This entry then accepts the ids: G [C x *nrows x 17] with *nrows = the rows RESERVED per table (Nfl0 + Nfl2 + Nfl3 + 400) and zeros
 * beyond a table's own rows. */
int tamcmc_hip_adjoint_table(tamcmc_hip_ctx *ctx, int model_id, int C, const double *params, int64_t Nparams, const int32_t *plength,
                             const double *Tcoefs, double p, double *G, double *Gn, int *nrows);

/* Analytic gradient of the Gaussian-envelope fits (ids 0, 1; TAMCMC_OPT_ENVELOPE_GRADIENT = 1).  Both models are closed forms in which
 * every parameter moves every bin, so with r_i = 1/M_i - y_i/M_i^2
 *   dS/dtheta_j = sum_i r_i dM_i/dtheta_j,   S = sum_i (y_i/M_i + ln M_i),   logL = -(long)p S / T.
 * The device sums r against the derivatives of M with respect to the ROW QUANTITIES (the scalars formed once per vector) in the pass that
 * forms M -- 1024-bin tiles, one partial per (vector, tile), folded in a fixed order, no atomics -- and the host applies the chain rule
 * from row quantities to parameters in long double.  With L = 1/(1 + e^u), D = L (1 - L), g = exp(-d^2/(2 sigma^2)), d = x - nu:
 *   id 1  M = A g + sum_q H_q L_q + N0, u_q = pw_q (lna_q + ln x):   dM/dA = g, dM/dnu = A g d/sigma^2, dM/dsigma^2 = A g d^2/(2 sigma^4),
 *         dM/dN0 = 1, dM/dH_q = L_q, dM/dlna_q = -H_q D_q pw_q, dM/dpw_q = -H_q D_q (lna_q + ln x); a term with tc = 0 is switched off and
 *         has 0 in its three places.  A = |p7|, nu = p8, sigma^2 = |p9|^2, N0 = |p6|, H = |p[3q]|, lna = ln(1e-3 |p[3q+1]|), pw = |p[3q+2]|.
 *   id 0  M = A eta^2 g + N0 + sum_k C_k L_k, u_k = c_k (ln x - ln b_k), C_k = a_k^2/(h I_k), I_k = sum_i w_i L_k(x_i) (the trapezoid sum
 *         of the normalisation, h = x(1) - x(0)):   g's derivatives as above times eta^2, dM/da_k^2 = L_k/(h I_k),
 *         dM/dln b_k = C_k (c_k D_k - L_k I_k^b/I_k), I_k^b = sum_i w_i c_k D_k,
 *         dM/dc_k = C_k (-D_k (ln x - ln b_k) - L_k I_k^c/I_k), I_k^c = -sum_i w_i D_k (ln x - ln b_k):
 *         the normalisation integral moves with b_k and c_k.  (c_k D_k - L_k I_k^b/I_k = c_k L_k (Lbar_k - L_k), Lbar_k = sum w L_k^2 / I_k:
 *         the sums are formed for both forms and the one whose terms are the smaller is used, so a spectrum whose bins all lie on one
 *         side of b_k keeps its digits.)  a_0^2 = (p0 nu^p1)^2, a_1 = p5, a_2 = p6,
 *         ln b_k = ln|p_i| + p_j ln|nu + mu| for (i, j) = (2, 3), (7, 8), (10, 11), c = |p4|, |p9|, |p12|, N0 = |p13|, A = |p14|,
 *         nu = |p15|, sigma = |p16|, mu = p17.  p18 does not reach the model: its likelihood share is exactly 0.
 * Conventions.  d|p|/dp = copysign(1, p).  A bin adds exactly 0 to the lna / pw / ln b / c sums when D = 0 (a saturated term, which
 * includes a first bin at x = 0) or when its ln x term is not finite.  With pw = 0 (or c = 0) the power law is 1 and L = 1/2, as the
 * evaluation has it.  A degenerate vector (b_k = 0, tc = 0: d lna/dtc = 1/tc) gives non-finite components; they are returned as they come
 * (both samplers map a non-finite component to 0).
 * logL0 is tamcmc_hip_loglike_params_batch's bit for bit (the two sums of S and I_k are formed by the evaluation's statements in its
 * orders); the prior's share and logPr0 are the default route's bits (same forward / backward points, same kernel).  A vector's sums do
 * not depend on the batch it sits in; two calls give the same bits.
 * Tolerance: M is stated to 1e-12 per bin, so component j lies within
 *   B_j = 1e-12 sum_i |dM_i/dtheta_j| (1/M_i + 2 y_i/M_i^2)   (summed over the chain-rule branches of theta_j)
 * of a 50-digit derivative of S itself (tests/test_gpu_envelope_gradient.py; measured ratios in DESIGN section 9).
 *
 * The audit entry: the row-space sums before the chain rule, whatever the option says.  S[C] (un-tempered); sums[C x TAMCMC_ENVELOPE_GRAD_N]
 * = dS/d(row quantity) in the order
 *   id 1  [A, nu, sigma^2, N0, H_0, H_1, lna_0, lna_1, pw_0, pw_1, 0, 0, 0]
 *   id 0  [A, nu (through the Gaussian only), sigma^2, N0, a_0^2, a_1^2, a_2^2, ln b_0, ln b_1, ln b_2, c_0, c_1, c_2];
 * ksi[C x TAMCMC_ENVELOPE_KSI_N] (id 0; may be NULL, not written for id 1) = [I_0, I_1, I_2, I_0^b, I_1^b, I_2^b, I_0^c, I_1^c, I_2^c].
 * Other model ids: TAMCMC_ERR_BAD_MODEL; no spectrum: TAMCMC_ERR_NO_SPECTRUM. */
#define TAMCMC_ENVELOPE_GRAD_N 13
#define TAMCMC_ENVELOPE_KSI_N 9
int tamcmc_hip_envelope_gradient_sums(tamcmc_hip_ctx *ctx, int model_id, int C, const double *params, int64_t Nparams, double *S, double *sums,
                                      double *ksi);

/* Audit entry of the red-giant gradient batches (ids 25, 27; others: TAMCMC_ERR_BAD_MODEL): the tables of the B = C x (Nvars + 1) vectors
 * of a batch -- slot c (Nvars + 1) is chain c's vector, slot c (Nvars + 1) + 1 + k the same with hstep[k] added to index_to_relax[k] --
 * after the batch's own table builder and nothing else: the very bits every route of tamcmc_hip_fd_gradient goes on from (the host cannot
 * build a red-giant table: tamcmc_build_mode_table refuses the ids).  Same params, index_to_relax and hstep as tamcmc_hip_fd_gradient; any
 * arithmetic mode (STRICT: the host's long-double unpack, as there).
 * Out (any may be NULL): *per = rows reserved per slot; rows [B x *per] (a slot's first nrows[slot] rows are its table); noise
 * [B x max(plength[8], 1)], nharvey [B], nnoise [B]; status [B].  Call with C = 0 for *per.  Returns the first status that is not TAMCMC_OK. */
int tamcmc_hip_rgb_batch_tables(tamcmc_hip_ctx *ctx, int model_id, int C, const double *params, int64_t Nparams, const int32_t *plength,
                                const int32_t *index_to_relax, int Nvars, const double *hstep, tamcmc_multiplet *rows, int32_t *nrows,
                                double *noise, int32_t *nharvey, int32_t *nnoise, int32_t *status, int *per);

/* The same audit entry for the main-sequence ids (3, 11, 12, 13, 14, 23; red giants and envelope fits: TAMCMC_ERR_BAD_MODEL): the tables
 * of the slots [0, C x (Nvars + 1)) of a gradient batch as its table kernel (k_fd_unpack -> wg_unpack) leaves them and nothing after it;
 * the base-table copies the windowed route keeps behind them are not part of it.  prior_class 0: the kernel prepares the unpack alone (the
 * tamcmc_hip_fd_gradient path; priors, priors_switch, extra_priors may be NULL); 2 or 3: the log-prior is evaluated first and its last
 * lane prepares the unpack (the tamcmc_hip_fd_gradient_posterior path) -- the table does not depend on what the prior says.  A slot whose
 * table failed holds the placeholder dev_unpack.h states: no rows, nnoise = 1, noise[0] = 1, nharvey = 0, and its status.
 * Out as tamcmc_hip_rgb_batch_tables (*per = the rows every table has). */
int tamcmc_hip_fd_batch_tables(tamcmc_hip_ctx *ctx, int model_id, int prior_class, int C, const double *params, int64_t Nparams,
                               const int32_t *plength, const int32_t *index_to_relax, int Nvars, const double *hstep, const double *priors,
                               const int32_t *priors_switch, const double *extra_priors, tamcmc_multiplet *rows, int32_t *nrows,
                               double *noise, int32_t *nharvey, int32_t *nnoise, int32_t *status, int *per);

/* Expected (Fisher) information of the chi^2(2p) likelihood at each of the C parameter vectors:
 *   F_jk = (p / T_c) sum_i (d_j M_i)(d_k M_i) / M0_i^2,   j, k over the Nvars free variables (index_to_relax), the sum over all bins,
 * M0 the model row at theta, T_c = Tcoefs[c] (NULL -> 1), p truncated to long as in the likelihood.  It is the expectation of the Hessian of
 * -logL at y = M0: a quick Laplace error bar of a fit ((F + prior curvature)^-1) and a data-driven start for the proposal law
 * (tamcmc_sampler_seed_proposal_fisher).  The derivative is the CENTRAL difference with FROZEN windows: the tables at theta +- hstep[k] e_k are
 * built on the device by the gradient batch's builder, every row of both takes the base table's window [i0, i1) (as the adjoint route: no
 * truncation edge crosses a bin between the two), both model rows are evaluated by the likelihood kernel, and
 *   U_k,i = (M+_k,i - M-_k,i) / (h_applied,k M0_i),   F = (p / T) U U^T,
 * h_applied,k = the difference of the two perturbed doubles as stored.  (With unfrozen windows F moves by up to 10 % of sqrt(F_jj F_kk) on a
 * global fit with asymmetry; a forward difference moves it by 2e-3; the central form agrees with itself at h and h / 2 to 4e-5.)
 * The rows stay on the device (TAMCMC_OPT_FISHER_WORKSPACE_MB); U U^T is accumulated per slab of TAMCMC_FISHER_SLAB bins in 16x16 blocks
 * with the fp64 matrix instruction, the slabs are added in slab order.  One fixed order everywhere: two calls give the same bits, F is
 * symmetric bit for bit, and a chain's F does not depend on the number of chains, its place in the batch or the number of passes.
 * Out: F [C x Nvars x Nvars].  hstep[k] != 0.
 * Models: the fixed-length table models, ids 3, 11, 12, 13, 14, 23, and with TAMCMC_OPT_RGB_FISHER = 1 the red giants, ids 25 and 27 (below);
 * ids 0, 1 (no table) return TAMCMC_ERR_BAD_MODEL, and so do 25 and 27 with the option at 0.  Arithmetic: FAST or FAST_DIRECT; STRICT returns TAMCMC_ERR_BAD_ARG, as for the adjoint route.  A perturbed
 * vector whose table fails makes the call return that status; row and column k of that chain's F are then NaN (all of it when the base
 * table fails), the other chains are unaffected.
 * Tolerance: the FAST tolerance of a model row (|dM|/M <= 1e-12 per bin) carried through the difference and the product: against the same
 * quantity from long-double model rows, |dF_jk| <= 2 (p/T) (eps_k ||U_j||_1 + eps_j ||U_k||_1 + Nx eps_j eps_k), eps_k = 2e-12 / |h_applied,k|
 * (tests/test_gpu_fisher.py; the factor 2 covers the device table builder's last-ulp differences in the frequencies).
 *
 * Red giants (ids 25, 27; TAMCMC_OPT_RGB_FISHER = 1).  A perturbation may change the SET of l=1 mixed modes; every later row then shifts and
 * "the base row's window" means nothing.  For each chain and variable BOTH perturbed tables are classified on the device against the
 * chain's base table with the rule of the hybrid adjoint (see tamcmc_hip_adjoint_table: LINEARISABLE / FALLBACK, csrc/adj_rgb_match.h),
 * and the form follows from the two classes (csrc/fisher_rgb_rule.h):
 *   both linearisable   the frozen central difference above;
 *   one linearisable    the frozen ONE-SIDED difference on that side, U_k,i = (M+ - M0) / ((x+ - x0) M0) or (M0 - M-) / ((x0 - x-) M0): the
 *                       other slot is overwritten with the base table, so that its model row is M0 bit for bit and it adds exactly zero;
 *   both fallback       the central difference of the two rows on their OWN windows (unfrozen): F then carries the window-edge error
 *                       quantified above, which is better than no information for a seed;
 *   a failed table      as above: NaN in row and column k (the whole chain when the base vector fails), the status returned.
 * The step is the difference of the doubles as stored for the form used.  tamcmc_hip_get_rgb_fisher_stats counts the three forms.
 * The one-sided form's truncation error, measured on the small test star at a point where both forms exist for the same variable (the
 * period spacing; numpy yardstick, tests/test_gpu_rgb_fisher.py): at most 4.0e-3 of sqrt(F_jj F_kk) (id 25;
 * 2.5e-3 for id 27) over all elements when EVERY variable is taken one-sided at steps of 1e-6 |theta| -- the largest element is the one
 * between the period spacing, in which the mixed-mode frequencies are curved, and a bias value of those frequencies -- against 4e-5 for the central form at h and h / 2.  Across the mode-count change
 * of that test the unfrozen central difference would give F_kk = 5.8e7 where the one-sided form gives 3.2e4.
 * The same tolerance, with h_applied the step of the form used; the same determinism: a chain's F does not depend on the number of chains,
 * its place in the batch or the number of passes (the chains of a pass are the smaller of the row budget's and what the red-giant
 * pre-step's workspace takes at 2 Nvars + 1 vectors a chain). */
int tamcmc_hip_fisher(tamcmc_hip_ctx *ctx, int model_id, int C, const double *params, int64_t Nparams, const int32_t *plength,
                      const int32_t *index_to_relax, int Nvars, const double *hstep, const double *Tcoefs, double p,
                      double *F /* [C x Nvars x Nvars] */);
/* The audit entry of the same Gram and fold kernels on caller data: G [N x N] = sum_k w_k A_jk A_lk for A [N x K] row-major, w [K] or NULL
 * (all ones).  With small integers every sum is exact in double, which checks the block layout and the lane map of the matrix instruction. */
int tamcmc_hip_weighted_gram(tamcmc_hip_ctx *ctx, int N, int64_t K, const double *A /* [N x K] */, const double *w /* [K] or NULL */,
                             double *G /* [N x N] */);
/* Split of the last tamcmc_hip_fisher call made with TAMCMC_OPT_TIMING on, from HIP events on the context's stream, summed over its
 * passes: table build (red giants: with the mixed-mode pre-step), window freeze + row launches, Gram + fold (milliseconds; any pointer
 * may be NULL). */
int tamcmc_hip_get_fisher_times(tamcmc_hip_ctx *ctx, double *tables_ms, double *rows_ms, double *gram_ms);
/* Red giants (TAMCMC_OPT_RGB_FISHER): the (chain, variable) pairs of the last tamcmc_hip_fisher call made with TAMCMC_OPT_TIMING on that
 * took the central, the one-sided and the unfrozen form, summed over its passes; pairs with a failed table are in none (any pointer may
 * be NULL). */
int tamcmc_hip_get_rgb_fisher_stats(tamcmc_hip_ctx *ctx, int64_t *central, int64_t *one_sided, int64_t *unfrozen);

/* Timing of the likelihood kernel measured with HIP events on the context's own stream
 * (enabled by TAMCMC_OPT_TIMING): totals since the last reset. */
int tamcmc_hip_get_kernel_stats(tamcmc_hip_ctx *ctx, double *kernel_ms_total, int64_t *launches,
                                int64_t *evaluations);
int tamcmc_hip_reset_kernel_stats(tamcmc_hip_ctx *ctx);
/* Windowed finite differences (TAMCMC_OPT_FD_WINDOWED, timing enabled): since the last reset, the bins inside the affected ranges of
 * the delta evaluations and the number of those evaluations -- the bytes such a launch really touches are 24 B per affected bin
 * (x, y, base model row), not 16 B x Nx per evaluation. */
int tamcmc_hip_get_fd_stats(tamcmc_hip_ctx *ctx, int64_t *affected_bins, int64_t *delta_evaluations);
/* ... and how many of those delta evaluations were "full tables": a perturbation that moves most multiplets (a splitting coefficient,
 * the asymmetry) is evaluated as the whole perturbed table minus the stored base model row instead of +new / -old row pairs
 * (FAST arithmetic only; same tolerance as the pair tables: the unchanged rows cancel exactly). */
int tamcmc_hip_get_fd_full_tables(tamcmc_hip_ctx *ctx, int64_t *full_table_evaluations);
/* Hybrid red-giant adjoint batches (TAMCMC_OPT_RGB_ADJOINT, timing enabled): since the last reset, the perturbed slots of the gradient
 * calls (host entries and both samplers' Langevin steps) that were contracted and that fell back to the windowed difference; slots with a
 * failed table are in neither. */
int tamcmc_hip_get_rgb_adjoint_stats(tamcmc_hip_ctx *ctx, int64_t *linearised_slots, int64_t *fallback_slots);
/* ... and the HIP-event split of the last such batch of a host entry, ms6 = table build (with the classification), base launch, row pass,
 * noise pass + folds, fallback delta launches (moments, far-only tiles, DELTA launch, its fold), contraction (milliseconds). */
int tamcmc_hip_get_rgb_adjoint_times(tamcmc_hip_ctx *ctx, double *ms6);

/* ---------------- posterior model spectrum ---------------- */
/* Per-bin statistics of the model M over a stream of parameter vectors (posterior draws), reduced over the SAMPLES axis on the device
 * (csrc/model_stats.hip): the mean model and its variance, the envelope, the posterior mean of y/M -- the residual checked against
 * chi^2 with 2 d.o.f. -- and the mean background.  It stands in for the models Diagnostics::gnuplt_model_diags (phases `buffer` and
 * `final`) and get_models of the reference evaluate one by one on the host (diagnostics.cpp); the plots themselves are not made here.
 * Seven planes of Nx doubles stay on the device; nothing proportional to (vectors x Nx) is stored or copied.
 *
 * The law.  A vector is ACCEPTED when its table status is TAMCMC_OK and its weight is > 0; the others are skipped and counted.  M is
 * evaluated with the STRICT per-bin operation order -- the windowed Lorentzian multiplets in table order, then harvey_like: the bits
 * tamcmc_hip_loglike_params_batch(model = ...) writes on a STRICT context -- whatever TAMCMC_OPT_PRECISION says.  Per bin i, over the
 * accepted vectors b in arrival order, every operation rounded on its own (no fused multiply-add):
 *     R_i  = M of the first accepted vector ever added (a reference plane, stored once)
 *     d    = M_b,i - R_i
 *     A1  += w_b d              A2 += w_b (d d)
 *     mn   = M < mn ? M : mn    mx  = M > mx ? M : mx          (from +inf / -inf)
 *     Q   += w_b (y_i / M)                                     (IEEE division)
 *     G   += w_b Bg_b,i         Bg = the Harvey terms in order, then the white noise: M before the modes are added
 *     W   += w_b                                               (a scalar on the host, same order)
 * and  mean = R + A1 / W,  var = max(0, (A2 - (A1 A1) / W) / W),  ratio = Q / W,  background = G / W,  min = mn,  max = mx.
 * The shift by R keeps the variance meaningful when the posterior spread is 1e-6 of the model: the mean lies within
 * (n + 2) 2^-53 max|M| and the variance within 8 (n + 2) 2^-53 (sigma^2 + sigma max|d|) of their exact values over n vectors
 * (tests/test_model_stats_reference.py, against 50-digit arithmetic; the unshifted sums fail that at a spread of 1e-12).
 * A non-finite M propagates into mean, var and ratio of the bins it touches, like a non-finite model into logL; min and max ignore a NaN.
 * The result of a bin depends on the sequence of accepted vectors alone: not on the chunk size, on how the vectors are split over
 * calls, on TAMCMC_OPT_WORKGROUP / _BINS_PER_THREAD / _PRECISION, nor on zero-weight or failed vectors in between.
 *
 * create: the handle BORROWS the context (destroy the handle first); inputs [Nparams] and relax [Nparams] (1 = free; NULL: add_params
 *   only) serve add_vars; plength as for tamcmc_hip_loglike_params_batch; chunk = vectors per launch (0 = default 1024, <= 65535).
 *   Models: ids 3, 11, 12, 13, 14, 23 (host table builders) and 25, 27 (device pre-step: the per-vector status stays on the device and the
 *   kernel skips failed vectors there).  The envelope models, ids 0 and 1, have no tables and are out of scope: TAMCMC_ERR_BAD_MODEL.
 *   No spectrum: TAMCMC_ERR_NO_SPECTRUM.  y is read at add time.
 * add_params: n rows of Nparams doubles, row_stride doubles apart.  add_vars: n rows of the Nvars free variables, scattered into a copy of
 *   inputs through relax; with row_stride = Nchains Nvars, chain 0 of a tamcmc_sampler_run record [n x Nchains x Nvars] is passed in
 *   place.  weights [n] or NULL (all 1).  A negative or non-finite weight: TAMCMC_ERR_BAD_ARG, the handle unchanged.  A vector whose table
 *   fails is skipped and counted; the call still returns TAMCMC_OK.
 * get: W, counts = {accepted, skipped: table failed, skipped: weight 0}, and the six results, each [Nx] or NULL.  TAMCMC_ERR_BAD_ARG on a
 *   handle with nothing accepted.  A context whose Nx is no longer the one at creation: TAMCMC_ERR_BAD_ARG from add_* and get.
 * reset: forgets everything added (the handle is as after create). */
typedef struct tamcmc_model_stats tamcmc_model_stats;
int tamcmc_hip_model_stats_create(tamcmc_model_stats **ms, tamcmc_hip_ctx *ctx, int model_id, const double *inputs, int64_t Nparams,
                                  const int32_t *relax, const int32_t *plength, int32_t chunk);
int tamcmc_hip_model_stats_add_params(tamcmc_model_stats *ms, int64_t n, const double *params, int64_t row_stride, const double *weights);
int tamcmc_hip_model_stats_add_vars(tamcmc_model_stats *ms, int64_t n, const double *vars, int64_t row_stride, const double *weights);
int tamcmc_hip_model_stats_get(const tamcmc_model_stats *ms, double *W, int64_t counts[3], double *mean, double *var, double *min, double *max,
                               double *ratio, double *background);
int tamcmc_hip_model_stats_reset(tamcmc_model_stats *ms);
void tamcmc_hip_model_stats_destroy(tamcmc_model_stats *ms);

#ifdef __cplusplus
}
#endif
#endif /* TAMCMC_HIP_H */
