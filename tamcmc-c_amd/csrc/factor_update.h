// factor_update.h -- the opt-in rank-one step of the proposal factor (TAMCMC_OPT_FACTOR_REFRESH), what the host engine (host_mala.cpp),
// the device engine (dev_iterate_impl.h) and the host-only entry tamcmc_factor_rank_one_update must agree on, written once: when an
// adapting iteration takes the rank-one step, the step's two scalars, the coefficients of a column and the serial form of the update.
// Plain arithmetic only: no HIP types, so a plain C++ compiler can include it.  (The schedule -- which adapting iterations are full by
// the count k -- is factor_step_mode in step_schedule.h.)
//
// The Robbins-Monro step Sigma' = (1 - g) Sigma + g d d^T is a scaled rank-one change.  With L L^T = sigma (Sigma + eps I) in force,
//     beta^2 L L^T + w w^T,   beta^2 = (1 - g) sigma' / sigma,   w = sqrt(g sigma') d
// is sigma' (Sigma' + (1 - g) eps I): the factor follows the covariance in O(Nv^2), the regulariser decays by (1 - g) per step until the
// next full factorisation (tamcmc_sampler.h states the law).
//
// Solve, then scale.  p = L^-1 w (one forward substitution, reciprocal pivots), alpha_k = beta^2 + sum_{j <= k} p_j^2 (alpha_-1 =
// beta^2).  Then beta^2 L L^T + w w^T = L (beta^2 I + p p^T) L^T and the Cholesky factor G of beta^2 I + p p^T is known in closed form,
//     G_kk = beta sqrt(alpha_k / alpha_k-1) =: a_k,     G_ik = p_i b_k (i > k),  b_k = beta p_k / sqrt(alpha_k alpha_k-1),
// so L' = L G, row by row:  L'_ik = L_ik a_k + s_ik b_k  with the suffix sums  s_ik = sum_{k < j <= i} L_ij p_j  (k descending: a row
// needs its own elements, p, a and b only).  Every alpha_k >= beta^2 > 0: nothing is subtracted anywhere but in the substitution.
#pragma once
#include <math.h>

#include "rng.h"

namespace tamcmc {

// Is this adapting iteration a rank-one step?  mode: factor_step_mode (step_schedule.h); g: the gain c0 / (1 + i); rescaled: p2_fct
// scaled the covariance (its norm exceeded A1); valid: the chain's factor is marked valid.
TAMCMC_HD bool factor_takes_rank_one(int mode, double g, bool rescaled, bool valid) { return mode == 2 && g > 0.0 && g < 1.0 && !rescaled && valid; }

// beta^2 and the scale of w = scale x (x - mu'), from the gain and the scale before / after its own update
TAMCMC_HD double factor_beta2(double g, double sigma_old, double sigma_new) { return (1.0 - g) * sigma_new / sigma_old; }
TAMCMC_HD double factor_w_scale(double g, double sigma_new) { return sqrt(g * sigma_new); }

// a_k, b_k of column k from beta, alpha_k-1, alpha_k, p_k.  false: not finite and positive (the step is refused)
TAMCMC_HD bool factor_column(double beta, double alpha_prev, double alpha, double p, double *a, double *b) {
    const double t = beta / sqrt(alpha * alpha_prev);
    *a = alpha * t;
    *b = p * t;
    return *a > 0.0 && *a <= 1.7976931348623157e308 && fabs(*b) <= 1.7976931348623157e308;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The serial form: L [n x n] lower triangular, row-major with row stride ld, updated in place to the factor of beta2 L L^T + w w^T;
// work [3 n].  false (L untouched): a pivot or a coefficient is not finite and positive.  Element by element the operations of the
// device function (dev_iterate_impl.h::factor_rank_one_as) in their order.
inline bool factor_rank_one_serial(long n, double *L, long ld, const double *w, double beta2, double *work) {
    double *p = work, *a = work + n, *b = work + 2 * n;
    if (!(beta2 > 0.0) || !(beta2 <= 1.7976931348623157e308)) return false;
    const double beta = sqrt(beta2);
    double alpha = beta2;
    for (long k = 0; k < n; k++) {  // column k of the substitution: p_k, then every row below loses L_ik p_k
        if (k == 0)
            for (long i = 0; i < n; i++) p[i] = w[i];
        const double pk = p[k] * (1.0 / L[k * ld + k]);
        p[k] = pk;
        for (long i = k + 1; i < n; i++) p[i] = p[i] - L[i * ld + k] * pk;
        const double ap = alpha;
        alpha = alpha + pk * pk;
        if (!factor_column(beta, ap, alpha, pk, a + k, b + k)) return false;
    }
    for (long i = 0; i < n; i++) {
        double s = 0.0;
        double *row = L + i * ld;
        for (long k = i; k >= 0; k--) {
            const double v = row[k];
            row[k] = v * a[k] + s * b[k];
            s = s + v * p[k];
        }
    }
    return true;
}
#endif

}  // namespace tamcmc
