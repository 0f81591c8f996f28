// adj_rgb_match.h -- which perturbed tables of a red-giant gradient batch the table-space adjoint may contract row by row with their base
// table (the hybrid batch of fd_batch.hip), plain C++ for host and device so that a host test can compile it
// (tests/adj_rgb_match_driver.cpp).
//
// The rows of a red-giant table are the l=0 list, the l=1 mixed modes in frequency order, then the l=2 and l=3 lists (rgb_prestep.hip:
// k_rgb_finish).  A perturbation may change the SET of mixed modes; every later row then shifts and row j of the two tables is no longer
// the same mode.  A perturbed slot is LINEARISABLE when
//   - its status and the base's are TAMCMC_OK,
//   - it has the base table's row count,
//   - every row has the base row's l,
//   - every l=1 row's fc lies within half the distance from the base row's fc to that row's nearest l=1 neighbour in the base table
//     (the rows next to it: the mixed modes are stored in frequency order).  A set that lost one mode and gained another keeps its count
//     and fails this; a row with no l=1 neighbour has nothing to be confused with.
// Every other perturbed slot with two valid tables is a FALLBACK slot; a slot with a failed table is neither (NaN component, status).
#pragma once
#include <math.h>

#include "../../include/tamcmc_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADJ_RGB_HD __host__ __device__
#else
#define ADJ_RGB_HD
#endif

namespace tamcmc {

enum : int { ADJ_RGB_FAILED = 0, ADJ_RGB_LINEARISABLE = 1, ADJ_RGB_FALLBACK = 2 };
// How the class travels in the batch's d_flags (bits 0 and 1 are the DELTA launch's: noise changed, "full table"): set = linearisable,
// the slot's delta entry is empty and k_adj_contract writes its difference
constexpr int ADJ_RGB_FLAG_LINEAR = 4;

// Row j of two tables of n rows each: same degree, and an l=1 row has not moved half-way to its nearest l=1 neighbour (strictly less: a mode
// exactly half-way is as close to the neighbour's place as to its own).  A NaN frequency fails.
ADJ_RGB_HD inline bool adj_rgb_row_matches(const tamcmc_multiplet *base, const tamcmc_multiplet *pert, int n, int j) {
    if (pert[j].l != base[j].l) return false;
    if (base[j].l != 1) return true;
    double gap = HUGE_VAL;
    if (j > 0 && base[j - 1].l == 1) gap = fabs(base[j].fc - base[j - 1].fc);
    if (j + 1 < n && base[j + 1].l == 1) {
        const double up = fabs(base[j + 1].fc - base[j].fc);
        if (up < gap) gap = up;
    }
    return fabs(pert[j].fc - base[j].fc) < 0.5 * gap;
}

// The class of one perturbed slot from its finished table and the chain's base table.
ADJ_RGB_HD inline int adj_rgb_class(int status_base, int status_pert, const tamcmc_multiplet *base, int n_base, const tamcmc_multiplet *pert,
                                    int n_pert) {
    if (status_base != TAMCMC_OK || status_pert != TAMCMC_OK) return ADJ_RGB_FAILED;
    if (n_base != n_pert) return ADJ_RGB_FALLBACK;
    for (int j = 0; j < n_base; j++)
        if (!adj_rgb_row_matches(base, pert, n_base, j)) return ADJ_RGB_FALLBACK;
    return ADJ_RGB_LINEARISABLE;
}

}  // namespace tamcmc
