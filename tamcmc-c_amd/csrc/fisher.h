// fisher.h -- expected (Fisher) information of the chi^2(2p) likelihood (fisher.hip; tamcmc_hip_fisher, tamcmc_hip_weighted_gram).
//
//   F_jk = (p / T) sum_i (d_j M_i)(d_k M_i) / M0_i^2 = (p / T) (U U^T)_jk,   U_k,i = (M+_k,i - M-_k,i) / (h_applied,k M0_i),
// M+- the model rows at theta +- h_k e_k with every window held at the base table's [i0, i1) (frozen window, as adjoint.h).  The rows come
// from a gradient batch run with FdBatch::rows_only (fd_batch.h); k_fisher_gram forms U on the fly, one slab of bins per workgroup, and
// accumulates the upper 16x16 blocks of U U^T with v_mfma_f64_16x16x4_f64; k_fisher_fold adds the slabs in slab order, mirrors and scales.
// Red giants (ids 25 / 27, TAMCMC_OPT_RGB_FISHER): the same rows and the same two kernels; what differs is which windows the two perturbed
// tables of a (chain, variable) get and which step divides their difference (k_fisher_freeze_rgb below, fisher_rgb_rule.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tamcmc_hip.h"

namespace tamcmc {

constexpr int FISHER_SLAB = TAMCMC_FISHER_SLAB;  // bins per workgroup of k_fisher_gram

// One Gram launch: C sets of N rows over K bins.  Element (j, i) of set c is
//   X = (P[c set + j K + i] - Mn[same]) rh[c N + j] / M0[c set + i]      (Mn, rh, M0: each may be nullptr -> no subtraction / factor 1),
// and G_c = sum_i w_i X_j,i X_k,i (w nullptr: 1).  `set` = doubles between the row sets of two chains.
struct GramArgs {
    const double *P = nullptr, *Mn = nullptr, *M0 = nullptr, *rh = nullptr, *w = nullptr;
    size_t set = 0;
    int C = 0, N = 0, NP = 0, nslab = 0;  // NP = N padded to a multiple of 16
    long K = 0;
    double *part = nullptr;  // [C x nslab x NP x NP], upper 16x16 blocks written
    // fold: F[c][j][k] = F[c][k][j] = (sum over slabs, in slab order) * p / T[c]; status / E: per slot of the row batch (nullptr: none) --
    // a failed base table makes the chain's F NaN, a failed table at theta +- h_k e_k its row and column k
    const double *T = nullptr;
    double p = 1.0;
    const int *status = nullptr;
    int E = 0;
    double *F = nullptr;  // [C x N x N]
};
inline int fisher_padded(int N) { return (N + 15) / 16 * 16; }
inline int fisher_slabs(long K) { return (int)((K + FISHER_SLAB - 1) / FISHER_SLAB); }
hipError_t launch_fisher_gram(const GramArgs &g, hipStream_t st);  // k_fisher_gram, then k_fisher_fold
// frozen windows: every perturbed table (slot c E + e, e >= 1) takes [i0, i1) of each row from the chain's base table (slot c E); tables
// that failed (status != 0) are left alone
hipError_t launch_fisher_freeze(tamcmc_multiplet *mults, const int *pairs, const int *status, int per, int C, int E, hipStream_t st);

// Red-giant models (ids 25 / 27, TAMCMC_OPT_RGB_FISHER): a perturbation may change the set of mixed modes, and "the base row's window" then
// means nothing for the rows after the change.  k_fisher_freeze_rgb, one workgroup per (chain, variable), classifies BOTH perturbed slots
// against the base table (adj_rgb_match.h) and applies fisher_rgb_rule.h: it freezes the windows of the sides that correspond, overwrites a
// side that does not with the base table when the other one does (rows, row count, noise row, Harvey counts: its model row is then M0 bit
// for bit and the central-difference formula of k_fisher_gram gives the one-sided difference), leaves both alone when neither does, and
// writes rh[c][k], the step reciprocal of the form it chose.  E = 2 N + 1 slots per chain.
struct FisherRgbArgs {
    tamcmc_multiplet *mults = nullptr;  // the batch's tables: slot s at mults + pairs[2 s], `per` rows of room
    int *pairs = nullptr, *nh = nullptr, *nn = nullptr;
    double *noise = nullptr;  // [slots x stride]
    const int *status = nullptr;
    int per = 0, stride = 0, C = 0, N = 0;
    const double *rh3 = nullptr;  // [3 x C x N]: 1 / (x+ - x-), 1 / (x+ - x0), 1 / (x0 - x-) (FISHER_RGB_RH_*)
    double *rh = nullptr;         // [C x N], written
    unsigned long long *counts = nullptr;  // (optional) [3]: central, one-sided, unfrozen pairs, added to with integer atomics
};
hipError_t launch_fisher_freeze_rgb(const FisherRgbArgs &a, hipStream_t st);

}  // namespace tamcmc
