// fd_route.h -- which of its four routes a gradient batch (fd_batch.h) takes, plain C++ so that a host test can compile it
// (tests/fd_route_driver.cpp).
#pragma once
#include "../../include/tamcmc_hip.h"

namespace tamcmc {

// What comes after the tables of the C x (Nvars + 1) vectors:
//   Brute     every table evaluated in full: B sums;
//   Windowed  the C base points in full (planes 1/M0, y/M0, M0 kept), then the DELTA launch on the rows a perturbation changed: C base sums
//             and B differences;
//   Adjoint   the C base points as in Windowed, then the table-space adjoint G / Gn of each (adjoint.h) contracted with (table e - base
//             table), written where the DELTA launch writes its difference: the sums read like Windowed's.  Red giants (rgb, with
//             TAMCMC_OPT_RGB_ADJOINT): the hybrid batch -- the contraction for the slots whose rows correspond one to one with the base
//             table's (adj_rgb_match.h), Windowed's DELTA launch for the others;
//   Rows      every perturbed table given its base table's windows, then ONE launch that leaves the B model rows (fisher.h): no sums.
//             Red giants (rgb, with TAMCMC_OPT_RGB_FISHER): the windows per (chain, variable) by the rule of fisher_rgb_rule.h.
enum class FdRoute { Brute, Windowed, Adjoint, Rows };
// Who asks: the gradient entries and the sampler follow the context's options, the audit entry (tamcmc_hip_adjoint_table) and the Fisher
// information (tamcmc_hip_fisher) name their route whatever the options say; Tables (tamcmc_hip_rgb_batch_tables, tamcmc_hip_fd_batch_tables) asks for the batch's
// tables and nothing after them: the smallest layout, Brute's, in every arithmetic mode.
enum class FdRequest { FromOptions, Adjoint, Rows, Tables };

// gradient = TAMCMC_OPT_GRADIENT, fd_windowed = TAMCMC_OPT_FD_WINDOWED, precision = TAMCMC_OPT_PRECISION, delta_geometry: the DELTA variant
// of the likelihood kernel exists for the context's workgroup geometry; rgb: a red-giant model (tables of variable length); rgb_adjoint =
// TAMCMC_OPT_RGB_ADJOINT: the red-giant models may take the adjoint route, as the hybrid batch (FdBatch::layout then asks for a geometry
// that has the DELTA variant); rgb_fisher = TAMCMC_OPT_RGB_FISHER: the red-giant models may take the Rows route.
// Returns TAMCMC_OK and the route, or the refusal.
inline int fd_route(FdRequest request, int gradient, int fd_windowed, int precision, bool delta_geometry, int Nvars, bool rgb, FdRoute *route,
                    bool rgb_adjoint = false, bool rgb_fisher = false) {
    const bool strict = precision == TAMCMC_PRECISION_STRICT;
    if (request == FdRequest::Tables) {
        *route = FdRoute::Brute;
    } else if (request == FdRequest::Rows) {
        if ((rgb && !rgb_fisher) || strict) return TAMCMC_ERR_BAD_ARG;  // (tamcmc_hip_fisher refuses both before it gets here)
        *route = FdRoute::Rows;
    } else if (request == FdRequest::Adjoint || gradient == TAMCMC_GRADIENT_ADJOINT) {
        if (rgb && !rgb_adjoint) return TAMCMC_ERR_BAD_MODEL;  // (no row-by-row contraction of tables that differ in length, unless opted in)
        if (strict) return TAMCMC_ERR_BAD_ARG;  // (the planes are the FAST base launch's)
        *route = FdRoute::Adjoint;
    } else {
        // only the multiplets a perturbation changes are re-evaluated, on their windows, against the stored base model row (SURVEY
        // section 7, step 6: "the main algorithmic lever")
        *route = (fd_windowed && !strict && delta_geometry && Nvars > 0) ? FdRoute::Windowed : FdRoute::Brute;
    }
    return TAMCMC_OK;
}

}  // namespace tamcmc
