// adjoint.h -- table-space adjoint of the log-likelihood sum S = sum_i (y_i / M_i + ln M_i) (adjoint.hip), the third route of a gradient
// batch (fd_batch.hip, TAMCMC_OPT_GRADIENT = TAMCMC_GRADIENT_ADJOINT).
//
// Every parameter of a Lorentzian model reaches S only through the flat mode table and the noise row, so
//   dS = sum_rows sum_f G[row][f] dT[row].f + sum_j Gn[j] d|noise_j|,   f in {nu_m[7], hv_m[7], gamma, asym, fc},
// with G = sum_i r_i dM_i/df over the row's own window [i0, i1) of the BASE table (the window does not move with the parameters: the
// "frozen window" derivative) and r_i = (1/M0_i)(1 - y_i/M0_i) = dS/dM_i from the two planes the base launch leaves.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tamcmc_hip.h"

namespace tamcmc {

constexpr int ADJ_F = 17;         // fields of a row's adjoint: nu[7], hv[7], gamma, asym, fc
constexpr int ADJ_NTILE = 2048;   // bins per workgroup of the noise adjoint
constexpr int ADJ_SEG = 4096;     // bins of a row's window per workgroup of the row adjoint (segments counted from the row's i0)

struct AdjArgs {
    const double *x, *logx;  // resident spectrum grid and its logarithm
    int Nx;
    const double *planes;    // base points: [C x Nx] 1/M0, then `plane` doubles on [C x Nx] y/M0
    size_t plane;
    int C, E, per, stride;   // chains, evaluations per chain (slot of chain c's base table: c*E), rows per slot, noise row stride
    const tamcmc_multiplet *mults;  // [slots x per]
    const int *pairs, *nh, *nn, *status;  // by slot
    const double *noise;     // [slots x stride]
    double *G;               // [C x per x ADJ_F]
    double *Gpart;           // [C x per x nseg x ADJ_F] per-segment partials of G (only a row's own segments are written and read)
    int nseg;                // ceil(Nx / ADJ_SEG): the most segments a window can have
    double *Gn;              // [C x stride]
    double *npart;           // [C x ntn x stride] per-tile partials of Gn
    int ntn;                 // ceil(Nx / ADJ_NTILE)
    // Red giants (the hybrid batch of fd_batch.hip), all nullptr / 0 for the fixed-length models:
    //   cls [slots]: the batch's d_flags; a perturbed slot without ADJ_RGB_FLAG_LINEAR (adj_rgb_match.h) is a fallback slot, whose
    //   difference k_adj_contract copies from fall [slots] (the DELTA launch's sums) instead of contracting
    const int *cls = nullptr;
    const double *fall = nullptr;
    unsigned long long *counts = nullptr;  // (optional) [2]: perturbed slots k_adj_contract contracted / took from `fall`, added up over the launches
};

// G and Gn of the C base tables (k_adj_rows, k_adj_noise and the fixed-order sums of their segments / tiles).  ev (optional, 2 events):
// recorded after the row pass and after the noise pass + fold
hipError_t launch_adjoint(const AdjArgs &a, hipStream_t st, hipEvent_t *ev = nullptr);
// dS[slot] = sum_rows sum_f G (T_slot.f - T_base.f) + sum_j Gn (noise_slot[j] - noise_base[j]) for every slot of the batch (0 for a base
// slot, NaN where either table failed): what the DELTA launch of the windowed route leaves in the same place
hipError_t launch_adjoint_contract(const AdjArgs &a, double *dS, hipStream_t st);

}  // namespace tamcmc
