// dev_sampler.h -- interface of the device-resident sampler engine (dev_sampler.hip).
#pragma once
#include <stdint.h>

#include "../../include/tamcmc_hip.h"
#if defined(__HIPCC__)
#include "dev_unpack.h"
#include "envelope_row.h"
#endif

#define TAMCMC_MAX_CHAINS 64  // the reference caps at 24 (MALA.cpp:580-587); BASELINE config 5 asks for 40

namespace tamcmc {

#if defined(__HIPCC__)
// Kernel argument block: device pointers + scalars (passed by value).
struct DevSamplerArgs {
    ModelDesc desc;       // model_id, prior_class, Np, per, stride, Nx, grid, plength/priors/extra/poly pointers
    int C, Nv, ntiles, chol_in_lds;
#ifdef TAMCMC_PROBE       // probe build only (tools/learn_probe.py): leave adapt_chain after phase N -- the chains are then WRONG, only times are read
    int probe = 0;
#endif
    int swap_rule;        // 1: chain B's stored logPosterior after a swap as MALA.cpp:433,444 execute it
    long pl;              // likelihood_params truncated to long (likelihoods.h:14)
    long dN_mixing;
    uint64_t seed;
    double c0, epsilon1, epsi2, A1, target_acceptance;
    const int *index_to_relax;
    const double *Tcoefs;
    // chain state
    double *vars_cur, *params_cur, *logL_cur, *logPr_cur, *logPost_cur, *init_logL;
    double *vars_prop, *params_prop, *logPr_prop;
    int *status_prop, *moved;
    double *Pmove;
    long *counters;       // [0] iteration, [1] accepted moves of chain 0, [2] swap attempts, [3] swaps accepted, [8 + m] recorded moves of chain m
    // proposal law
    double *LT, *cov, *mu, *sigma;   // LT = transposed Cholesky factor of (cov+eps2)*sigma
    int *fvalid;          // [C] the chain's factor is marked valid: a condition of the rank-one step (factor_update.h)
    long *fcount;         // [4] since creation, over all chains: rank-one steps, scheduled full steps, forced full steps, rank-one steps refused
    double *lz;           // [2][C][Nv] L z of the NEXT iteration, computed ahead by spare workgroups while L is frozen
    double *grad_cur, *gradP_cur;  // Langevin step: [2][C][Nv] gradient of the tempered log-posterior at the chains' positions, and the prior's share
    // likelihood-kernel input block written by k_propose_unpack
    tamcmc_multiplet *mults;
    int *pairs, *nh, *nn;
    double *noise;
    double *partials;
    double *bg;           // [C x ntiles x 8] background series per (slot, tile), FAST far field only (else nullptr)
    int tile_bins;
    EnvRow *env_rows;     // [C] Gaussian-envelope models (ids 0 / 1): the row of each chain's proposal, what its evaluation reads (else nullptr)
    // records
    double *samples, *stats;
};
#endif

struct DevSamplerInit {
    int model_id, prior_class, C, Np, Nv;
    double likelihood_params;
    const int *plength, *index_to_relax, *priors_switch;
    const double *priors, *extra_priors, *Tcoefs;
    uint64_t seed;
    long dN_mixing;
    double c0, epsilon1, epsi2, A1, target_acceptance;
    int chain_groups = 0;  // 0 = default (2 from 8 chains on): stream groups of the lockstep scheme
    int swap_rule = 0;     // tamcmc_sampler_config.swap_rule
    int factor_refresh = 0;  // R of TAMCMC_OPT_FACTOR_REFRESH as the context held it at creation
    int use_drift = 0;     // 1: Langevin step (dev_mala_impl.h)
    double delta = 0, fd_step_rel = 1e-7;  // drift truncation (0 = none), relative forward-difference step
};

class DevSampler {
    struct Impl;
    Impl *impl;

  public:
    DevSampler();
    ~DevSampler();
    DevSampler(const DevSampler &) = delete;
    DevSampler &operator=(const DevSampler &) = delete;
    int init(tamcmc_hip_ctx *ctx, const DevSamplerInit &in);
    int upload_state(const double *vars, const double *params, const double *logL, const double *logPr,
                     const double *logPost, const double *init_logL);
    int upload_proposal(int m, const double *L_rowmajor, const double *cov, const double *mu, double sigma);
    int download_state(double *vars, double *params, double *logL, double *logPr, double *logPost, double *Pmove,
                       int *moved, long *counters, long *moves_per_chain = nullptr);
    int download_proposal(int m, double *cov, double *mu, double *sigma);
    int download_factor(int m, double *L_rowmajor);  // the factor in force for chain m, lower triangular (tamcmc_sampler_get_factor)
    int download_gradient(double *grad, double *grad_prior);  // use_drift: [C x Nv] gradient the engine holds for the chains' positions
    int download_last_proposal(double *vars_prop, double *grad_prop);  // use_drift: what the last iteration tested
    // [0] Nvars [1] Nparams [2] adaptation workspace in LDS (1) / global scratch (0) [3] fused step available [4] chain groups
    // [5] iterations run fused [6] iterations run by the lockstep kernels [7] chains [8] fused stretches
    // [9] quick_decide fallbacks taken by the likelihood tiles [10] tile tests decided from a kind-2 record (outside a swap pair)
    // [11] of [5] with two chain groups: iterations run as one joint launch [12] ... run in a window (step_schedule.h: StepPlanner)
    // [13] tests that quick_decide decided otherwise than the exact decide() (counted by the commit workgroups: 0, or a bug)
    // [14] rank-one steps of the factor [15] scheduled full factorisations [16] forced ones (all over the chains) [17] rank-one steps refused
    void info(long out[18]) const;
    // Audit (tamcmc_sampler_get_tables): the tables the last stretch of the last run() left in the likelihood kernel's input block and the
    // parameter vector each was built from, read from the engine's own buffers.  shape = {scheme, slots, rows per slot, noise stride}.
    // scheme 1 (lockstep): slot m = chain m's proposal of the last iteration, vector = params_prop of that iteration's parity;
    // scheme 2 (fused): slot e NS + s = candidate slot s of candidate set e (NS = 2 Nchains + 8), vector = cand_params of the same slot
    int download_tables(int32_t shape[4], tamcmc_multiplet *rows, int32_t *nrows, double *noise, int32_t *nharvey, int32_t *nnoise,
                        int32_t *status, int32_t *written, double *logPr, double *params);
    // Audit (tamcmc_sampler_get_envelope_rows), ids 0 / 1: per chain the row of the last iteration's proposal (EnvRow as 24 doubles, the
    // layout of tamcmc_sampler.h), the vector it was built from (params_prop of that iteration's parity), its log-prior and status
    int download_envelope_rows(double *rows, double *params, double *logPr, int32_t *status);
    // Audit (tamcmc_sampler_get_envelope_gradient_sums), ids 0 / 1 with use_drift: what k_env_grad_fold left for the last iteration's
    // proposals -- S [C], the tile sums [C x 16], the xi sums [C x 12] -- before the chain rule on the device
    int download_envelope_sums(double *S, double *tile_sums, double *xi_sums);
    int run(long it0, long n_iter, const char *learn, double *samples, double *stats);
};

}  // namespace tamcmc
