// fisher_rgb_rule.h -- which form of the derivative the Fisher information of a red-giant model (ids 25 / 27; fisher.hip:
// k_fisher_freeze_rgb) takes for one chain and one variable, plain C++ for host and device so that a host test can compile it
// (tests/rgb_fisher_rule_driver.cpp).
//
// The two perturbed tables, at theta + h e_k and at theta - h e_k, are each classified against the chain's base table with adj_rgb_class
// (adj_rgb_match.h, used unchanged).  From the two classes:
//   both linearisable     CENTRAL    both tables take the base table's windows, U = (M+ - M-) / ((x+ - x-) M0);
//   one linearisable      ONE_SIDED  that table takes the base table's windows and the OTHER slot is overwritten with the base table, so that
//                                    its model row is M0 bit for bit: U = (M+ - M0) / ((x+ - x0) M0) or (M0 - M-) / ((x0 - x-) M0);
//   both fallback         UNFROZEN   two valid tables, neither corresponds row by row: U = (M+ - M-) / ((x+ - x-) M0), each table on its
//                                    own windows;
//   a failed table        FAILED     nothing is written; row and column k of the chain's F are NaN (k_fisher_fold, from the statuses).
// The step reciprocal is one of three the host forms from the doubles as stored: 1 / (x+ - x-), 1 / (x+ - x0), 1 / (x0 - x-).
#pragma once
#include "adj_rgb_match.h"

namespace tamcmc {

enum : int { FISHER_RGB_FAILED = 0, FISHER_RGB_CENTRAL = 1, FISHER_RGB_ONE_SIDED = 2, FISHER_RGB_UNFROZEN = 3 };
enum : int { FISHER_RGB_RH_CENTRAL = 0, FISHER_RGB_RH_PLUS = 1, FISHER_RGB_RH_MINUS = 2 };  // which of the three reciprocals
enum : int { FISHER_RGB_SIDE_NONE = 0, FISHER_RGB_SIDE_PLUS = 1, FISHER_RGB_SIDE_MINUS = 2 };

struct FisherRgbChoice {
    int form;        // FISHER_RGB_*
    int rh;          // FISHER_RGB_RH_*
    int substitute;  // the side whose slot becomes a copy of the base table (FISHER_RGB_SIDE_*)
    bool freeze_plus, freeze_minus;  // the side's rows take the base rows' [i0, i1)
};

// class_plus / class_minus: ADJ_RGB_* of the two perturbed slots.
ADJ_RGB_HD inline FisherRgbChoice fisher_rgb_choose(int class_plus, int class_minus) {
    FisherRgbChoice c = {FISHER_RGB_FAILED, FISHER_RGB_RH_CENTRAL, FISHER_RGB_SIDE_NONE, false, false};
    if (class_plus == ADJ_RGB_FAILED || class_minus == ADJ_RGB_FAILED) return c;
    const bool lp = class_plus == ADJ_RGB_LINEARISABLE, lm = class_minus == ADJ_RGB_LINEARISABLE;
    if (lp && lm) {
        c.form = FISHER_RGB_CENTRAL; c.freeze_plus = c.freeze_minus = true;
    } else if (lp) {
        c.form = FISHER_RGB_ONE_SIDED; c.rh = FISHER_RGB_RH_PLUS; c.substitute = FISHER_RGB_SIDE_MINUS; c.freeze_plus = true;
    } else if (lm) {
        c.form = FISHER_RGB_ONE_SIDED; c.rh = FISHER_RGB_RH_MINUS; c.substitute = FISHER_RGB_SIDE_PLUS; c.freeze_minus = true;
    } else {
        c.form = FISHER_RGB_UNFROZEN;
    }
    return c;
}

// The same from the three finished tables (the serial form of what k_fisher_freeze_rgb does with lanes over rows).
ADJ_RGB_HD inline FisherRgbChoice fisher_rgb_choose_tables(int status_base, int status_plus, int status_minus, const tamcmc_multiplet *base,
                                                           int n_base, const tamcmc_multiplet *plus, int n_plus,
                                                           const tamcmc_multiplet *minus, int n_minus) {
    return fisher_rgb_choose(adj_rgb_class(status_base, status_plus, base, n_base, plus, n_plus),
                             adj_rgb_class(status_base, status_minus, base, n_base, minus, n_minus));
}

}  // namespace tamcmc
