// step_schedule.h -- what the host engine, the device engine and the host-side launch planning of the device engine must agree on, bit
// for bit, written once: the parallel-tempering swap pair of an iteration (one Philox draw) and the schedule of a run() call (which
// iterations run as fused steps, which of those as one launch over all chains).  Integer logic and rng.h only: no HIP types, so a plain
// C++ compiler can include it (tests/step_schedule_driver.cpp).
#pragma once
#include "rng.h"

namespace tamcmc {

// ---- the swap pair (MALA.cpp:397-405) ----

// (inlined into every caller whatever its size: on the device, decide() and k_iterate keep the code they have with the draw in line)
#define TAMCMC_HD_FLAT TAMCMC_HD __attribute__((always_inline))

// Does iteration `it` end with a swap attempt?  (the reference mixes every dN_mixing iterations, never at iteration 0)
TAMCMC_HD_FLAT bool is_swap_iteration(int C, long dN_mixing, long it) { return dN_mixing > 0 && (it % dN_mixing == 0) && it != 0 && C > 1; }

// The draw itself, whatever the iteration: first chain A of the pair (A, A+1) -- -1 for a single chain -- and the uniform of the swap
// test.
TAMCMC_HD_FLAT int swap_draw(uint64_t seed, int C, long it, double *u_out) {
    double u, u2;
    rng_uniform2(seed, RNG_SWAP, 0, (uint64_t)it, 0, u, u2);
    int A = (int)(u2 * (double)(C - 1));
    if (A > C - 2) A = C - 2;
    if (u_out) *u_out = u;
    return A;
}

// First chain of iteration `it`'s swap pair, -1 when the iteration has none.
TAMCMC_HD_FLAT int swap_pair(uint64_t seed, int C, long dN_mixing, long it, double *u_out) {
    return is_swap_iteration(C, dN_mixing, it) ? swap_draw(seed, C, it, u_out) : -1;
}

// ---- the proposal factor in an adapting iteration (TAMCMC_OPT_FACTOR_REFRESH = R; factor_update.h has the rule's other conditions) ----

// What the k-th adapting iteration of a sampler (k counted from 0 since its creation, on the host) does with the factor: 1 = a full
// factorisation, scheduled (always with R < 2: today's sampler; every R-th adapting iteration otherwise), 2 = a rank-one step where the
// chain's state allows it.  (0 is "no adaptation" in the kernels' learn arguments.)
TAMCMC_HD int factor_step_mode(int R, long k) { return (R >= 2 && k % R != 0) ? 2 : 1; }

// ---- chain groups ----

// Group of `chain` among the G contiguous groups [goff[g], goff[g+1]).
TAMCMC_HD int group_of(int chain, const int *goff, int G) {
    int g = 0;
    while (g + 1 < G && chain >= goff[g + 1]) g++;
    return g;
}

// ---- stretches of a run() call ----

constexpr long MIN_FUSED = 3;  // a fused stretch pays one entry launch: shorter quiet runs stay in lockstep

// End of the run of iterations without adaptation that starts at `from` (learn == nullptr: nothing learns).
TAMCMC_HD long quiet_end(const char *learn, long n_iter, long from) {
    long q = from;
    while (q < n_iter && !(learn && learn[q])) q++;
    return q;
}

// The stretch [i, *end) that a call of n_iter iterations runs next (i < n_iter), and its scheme: a quiet run of at least MIN_FUSED
// iterations is one fused stretch; everything up to the start of the next such run (or the end of the call) is one lockstep stretch.
TAMCMC_HD void next_stretch(const char *learn, long n_iter, long i, bool use_fused, long *end, bool *is_fused) {
    const long jn = quiet_end(learn, n_iter, i);
    if (use_fused && jn - i >= MIN_FUSED) {
        *end = jn;
        *is_fused = true;
        return;
    }
    long k = i;
    for (;;) {
        const long q = quiet_end(learn, n_iter, k);
        if (use_fused && q - k >= MIN_FUSED && k > i) break;
        k = q;
        while (k < n_iter && learn && learn[k]) k++;
        if (k >= n_iter) break;
    }
    *end = k;
    *is_fused = false;
}

// ---- fused stretch with two chain groups [0, xsplit) and [xsplit, C) (split_ok; otherwise every iteration is one launch) ----

// A swap pair (A, A+1) with one chain in each group.
TAMCMC_HD bool straddles(bool split_ok, int xsplit, int A) { return split_ok && A == xsplit - 1; }

// Is an iteration ONE launch over all chains?  A: its swap pair, A_prev: the previous iteration's (-1: none), first: the stretch's first
// iteration (the chains are settled, the previous iteration's swap is not this stretch's business).  The launch of a straddling swap's
// iteration builds the pair's cross candidates on both chains' vectors, the next one decides the swap from both chains' sums.
TAMCMC_HD bool joint_launch(bool split_ok, int xsplit, int A, int A_prev, bool first) {
    return !split_ok || straddles(split_ok, xsplit, A) || (!first && straddles(split_ok, xsplit, A_prev));
}

// ---- the launches of a two-group fused stretch, iteration by iteration (host only) ----
//
// Between straddling pairs the groups are [0, xsplit) on the first stream ("st") and [xsplit, C) on the second ("s1").  Around a
// straddling pair (xsplit-1, xsplit) the boundary moves instead of the groups merging: an iteration is in a WINDOW when its own pair or
// the previous iteration's straddles, and runs as [0, xsplit+1) on st and [xsplit+1, C) on s1 -- chain xsplit rides with the first
// group, so both pairs lie inside one launch and the second group's other chains never stop.  A window iteration whose own or previous
// pair is (xsplit, xsplit+1) -- it straddles the moved boundary -- or whose second group would be empty is the joint launch of
// joint_launch().  Who waits for whom (stream events only):
//   * st waits for s1 before the first launch of a window (chain xsplit's earlier launches ran on s1);
//   * s1 waits for st before the first two-group launch after a window (chain xsplit returns), and after a joint launch;
//   * st waits for s1 before a joint launch that follows two-group launches;
//   * inside a window, past its first iteration, the two streams also meet where they share the SECOND EXTRA BLOCK of candidate slots
//     (the cross candidates of chains >= xsplit, FusedArgs::xsplit: chain xsplit's on st, the other chains' on s1).  Launch i writes
//     the block of candidate set (i+1) mod 3 and reads those of sets i mod 3 and (i-1) mod 3, so a writer must follow the other stream's
//     two previous launches: s1 waits for st before a window launch whose pair lies in [xsplit+1, C), st waits for s1 before a window
//     launch whose pair straddles again.  (tests/step_hazard_driver.cpp replays the plan against every buffer of the fused step.)
// Everything else of the fused step is per chain, and a chain changes streams only across one of these waits.
struct StepPlan {
    int b;             // group 0 = chains [0, b) on st, group 1 = [b, C) on s1; b == C: one launch over all chains, on st
    bool window;       // two launches with the moved boundary b = xsplit + 1
    bool st_waits_s1;  // event hops before this iteration's launches
    bool s1_waits_st;
};

struct StepPlanner {
    bool split_ok;
    int C, xsplit;
    // who has not waited for whom (RunCall::run_fused sets s1_must_wait at the entry of a stretch)
    bool s1_must_wait = false;  // st holds launches that s1's next launch must follow
    bool s1_ahead = false;      // s1 holds launches that st has not waited for
    bool in_window = false;     // the previous iteration ran as a window
    bool first = true;          // nothing planned yet: the chains are settled, the pair before the stretch is nobody's business
    int A_prev = -1;

    StepPlanner(bool split_ok_, int C_, int xsplit_) : split_ok(split_ok_), C(C_), xsplit(xsplit_) {}

    // The plan of the next iteration, whose swap pair is (A, A+1) (-1: none).  A = -1 after the stretch's last iteration plans its
    // closing launches (the commit workgroups of the last iteration, which decide that iteration's swap).
    StepPlan next(int A) {
        StepPlan p;
        p.window = false; p.st_waits_s1 = false; p.s1_waits_st = false;
        const int Ap = first ? -1 : A_prev;
        const bool near = joint_launch(split_ok, xsplit, A, A_prev, first);  // its own pair or the previous one straddles (or no split)
        const bool joint = !split_ok || (near && (A == xsplit || Ap == xsplit || xsplit + 1 >= C));
        if (joint) {
            p.b = C;
            p.st_waits_s1 = s1_ahead;
            s1_ahead = false;
            s1_must_wait = true;
            in_window = false;
        } else if (near) {
            p.b = xsplit + 1;
            p.window = true;
            p.st_waits_s1 = s1_ahead && (!in_window || A == xsplit - 1);
            p.s1_waits_st = s1_must_wait || (in_window && A > xsplit);
            s1_ahead = true;
            s1_must_wait = false;
            in_window = true;
        } else {
            p.b = xsplit;
            p.s1_waits_st = s1_must_wait || in_window;
            s1_ahead = true;
            s1_must_wait = false;
            in_window = false;
        }
        A_prev = A;
        first = false;
        return p;
    }
};

}  // namespace tamcmc
