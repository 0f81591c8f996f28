// grad_assemble.h -- the rules every gradient entry's host side states once: the tempered log-likelihood of a sum, and the assembly of
// logL0, logPr0, grad and grad_prior from a finished batch.  Plain C++, no HIP include, so that a host test can compile it
// (tests/grad_assemble_driver.cpp).  The device's counterpart (mala_gradient, dev_mala_impl.h) is a different statement, in double.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/tamcmc_hip.h"

namespace tamcmc {

// call_likelihood (model_def.cpp:399-401): f = -p * (sum1 + sum2) in long double with p truncated to long, then / Tcoefs[m], one
// rounding to double at the end.  S is a sum, a difference of sums or a derivative of one; a double converts exactly.
inline double tempered_loglike(long double S, double p, double T) {
    const long pl = (long)p;
    long double f = S;
    f = -pl * f;
    return (double)(f / T);
}
inline double temperature_of(const double *Tcoefs, int m) { return Tcoefs ? Tcoefs[m] : 1.0; }

// Where the likelihood's share of a gradient comes from.  B = C (Nvars + 1) slots, slot c * (Nvars + 1) the base point of chain c.
//   FullSums      S [B]: the sum at every slot; the share is the difference of two tempered values over the applied step
//   Differences   S [C + B]: C base sums, then per slot the difference against its chain's base sum
//   Derivative    S [C]: the base sums; dlogL [C x Nvars]: d logL / d theta_k, tempered already
enum class LikelihoodShare { FullSums, Differences, Derivative };

// Sums and log-priors of a finished batch -> logL0, logPr0, grad, grad_prior.  lpp / lpm: log-priors at the forward / backward points
// by slot (lpp == nullptr: no prior, logPr0 = 0, grad is the likelihood's share untouched); status by slot (nullptr: no evaluation can
// fail; not read for Derivative); logPr0 and grad_prior may be nullptr.  With a prior a non-finite likelihood share counts as 0, and the
// prior's share is forward, else backward, else flat.  Returns the first status that is not TAMCMC_OK.
inline int assemble_gradient(int C, int Nvars, const double *params, int64_t Nparams, const int32_t *index_to_relax, const double *hstep,
                             const double *Tcoefs, double p, LikelihoodShare share, const double *S, const double *dlogL, const double *lpp,
                             const double *lpm, const int *status, double *logL0, double *logPr0, double *grad, double *grad_prior) {
    const int E = Nvars + 1;
    const size_t Np = (size_t)Nparams, Nv = (size_t)Nvars;
    const bool full = share == LikelihoodShare::FullSums, ready = share == LikelihoodShare::Derivative;
    int first_err = TAMCMC_OK;
    for (int ch = 0; ch < C; ch++) {
        const double T = temperature_of(Tcoefs, ch);
        auto failed = [&](int e) {
            const int st = (status && !ready) ? status[(size_t)ch * E + e] : TAMCMC_OK;
            if (first_err == TAMCMC_OK) first_err = st;
            return st != TAMCMC_OK;
        };
        const double L0 = failed(0) ? (double)NAN : tempered_loglike(full ? S[(size_t)ch * E] : S[ch], p, T);
        auto dlogL_of = [&](int e) {  // logL(theta + h e_k) - logL(theta)
            if (failed(e)) return (double)NAN;
            if (!full) return tempered_loglike(S[(size_t)C + (size_t)ch * E + e], p, T);
            return tempered_loglike(S[(size_t)ch * E + e], p, T) - L0;
        };
        logL0[ch] = L0;
        const double pr0 = lpp ? lpp[(size_t)ch * E] : 0.0;
        if (logPr0) logPr0[ch] = pr0;
        for (int k = 0; k < Nvars; k++) {
            double happ = 0.0;  // the step actually applied (the device adds the same two doubles); not needed by a bare derivative
            if (!ready || lpp) {
                const double x0 = params[(size_t)ch * Np + index_to_relax[k]];
                volatile double xp = x0 + hstep[k];
                happ = xp - x0;
            }
            double g = ready ? dlogL[(size_t)ch * Nv + k] : dlogL_of(k + 1) / happ;
            if (lpp) {
                if (!std::isfinite(g)) g = 0.0;
                const double prp = lpp[(size_t)ch * E + k + 1], prm = lpm[(size_t)ch * E + k + 1];
                double gp;
                if (std::isfinite(prp)) gp = (prp - pr0) / happ;
                else gp = std::isfinite(prm) ? (pr0 - prm) / happ : 0.0;  // forward point outside the support: backward, else flat
                g += gp;
                if (grad_prior) grad_prior[(size_t)ch * Nv + k] = gp;
            }
            grad[(size_t)ch * Nv + k] = g;
        }
    }
    return first_err;
}

}  // namespace tamcmc
