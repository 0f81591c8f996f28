// envelope.h -- Gaussian-envelope background fits (model ids 0 and 1) on the device (envelope.hip).
//   model_Kallinger2014_Gaussian (id 0)   tamcmc/sources/models.cpp (after model_Harvey_Gaussian), Kallinger2014 / get_ksinorm /
//                                         eta_squared_Kallinger2014 in noise_models.cpp:70-153
//   model_Harvey_Gaussian (id 1)          tamcmc/sources/models.cpp (before model_Kallinger2014_Gaussian), harvey_like noise_models.cpp:15-39
// Every bin of the fitted range depends on every parameter: no mode table, no window.  The host forms a few scalars per vector
// (EnvRow); the device walks the bins.  These are envelope.hip's doors: two for evaluations (a batch of vectors; the sampler's rows
// already on the device), one per C entry behind them.  What they share underneath is stated once in envelope.hip and envelope_row.h.
#pragma once
#include <stdint.h>

#include "ctx.h"

namespace tamcmc {

__host__ __device__ inline bool is_envelope_model(int model_id) {
    return model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN || model_id == TAMCMC_MODEL_HARVEY_GAUSSIAN;
}
// parameters each model reads: [H1, tc1, p1, H2, tc2, p2, B0, Amax, numax, Gauss_sigma] / 14 noise, Amax, numax, sigma, mu_numax, omega_numax
inline int64_t envelope_nparams(int model_id) { return model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN ? 19 : 10; }

// B parameter vectors (B x Nparams) -> S[b] = sum_i (y_i/M_i + ln M_i) on the resident spectrum, in a fixed order (a vector's S does not
// depend on the batch it sits in).  model (device pointer or nullptr): B x Nx rows.  Enqueued on the context stream; S_dev is the
// context's d_S (B doubles); the caller copies it back.
int envelope_enqueue(tamcmc_hip_ctx *c, int model_id, int B, const double *params, int64_t Nparams, double *model_dev);

// The device-resident sampler's lockstep route (dev_sampler.hip): k_env_ksi (id 0) and k_env_eval for `cnt` chains whose rows (EnvRow,
// envelope_row.h) k_iterate has left on the device, enqueued on `st`.  rows_dev, ksi_part (cnt x chunks x 3) and partials (cnt x tiles x
// 2) point at the FIRST of these chains' entries: every buffer is indexed by chain, so chain groups on different streams share no slot.
int envelope_stage_enqueue(tamcmc_hip_ctx *c, int model_id, int cnt, const void *rows_dev, double *ksi_part, double *partials, hipStream_t st);

// The device-resident Langevin step's door (dev_sampler.hip; TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN): the analytic gradient's kernels --
// k_env_ksi_grad (id 0), k_env_grad, k_env_grad_fold, the launches the gradient entries make -- for `cnt` chains whose rows
// k_env_mala_front has left on the device, enqueued on `st`.  Every buffer is the caller's and indexed by chain:
struct EnvGradBuffers {
    double *ksi_part = nullptr, *ksi_gpart = nullptr;  // id 0: chunk partials, cnt x chunks x 3 and x 9
    double *part = nullptr, *gpart = nullptr;          // tile partials, cnt x tiles x 2 and x (16 | 10)
    double *S = nullptr, *gsum = nullptr, *ksum = nullptr;  // folded: S [cnt] (the evaluation's bits), tile sums cnt x 16, xi sums cnt x 12
};
int envelope_grad_stage_enqueue(tamcmc_hip_ctx *c, int model_id, int cnt, const void *rows_dev, const EnvGradBuffers &b, hipStream_t st);

// tamcmc_hip_loglike_params_batch for ids 0 and 1
int envelope_loglike_params_batch(tamcmc_hip_ctx *c, int model_id, int B, const double *params, int64_t Nparams, const double *Tcoefs,
                                  double p, double *logL, double *model, int32_t *status);

// tamcmc_hip_fd_gradient (with_prior false) and tamcmc_hip_fd_gradient_posterior (true) for ids 0 and 1, from the entry's first line
// on: the argument rules, the refusal under TAMCMC_GRADIENT_ADJOINT, the prior-class rule (class 0 with id 0, class 1 with id 1), and
// the route -- TAMCMC_OPT_ENVELOPE_GRADIENT is read here and nowhere else.  The likelihood's share: C x (Nvars + 1) full evaluations in
// one batch (option 0), or the analytic gradient, one pass over the bins per chain (k_env_ksi_grad, k_env_grad, k_env_grad_fold; the
// chain rule from row quantities to parameters on the host in long double, env_row_jacobian).  The prior's share and logPr0 on either
// route: the log-priors of the forward and backward points on the device, one thread per point (priors_impl.h)
int envelope_gradient(tamcmc_hip_ctx *c, int model_id, bool with_prior, int prior_class, int C, const double *params, int64_t Nparams,
                      const int32_t *index_to_relax, int Nvars, const double *hstep, const double *Tcoefs, double p, const double *priors,
                      const int32_t *priors_switch, double *logL0, double *logPr0, double *grad, double *grad_prior);

// tamcmc_hip_envelope_gradient_sums: S [C], dS / d(row quantity) [C x TAMCMC_ENVELOPE_GRAD_N], the xi sums [C x 9] (id 0; ksi may be nullptr)
int envelope_gradient_sums(tamcmc_hip_ctx *c, int model_id, int C, const double *params, int64_t Nparams, double *S, double *sums, double *ksi);

}  // namespace tamcmc
