// fd_block.h -- the head of a gradient batch's device block (fd_batch.h): the seven arrays a caller fills and the three it reads back.
// Plain C++ so that a host test can compile it (tests/fd_block_driver.cpp).  What lies behind the head -- tables, delta tables, adjoint
// workspace -- is FdBatch::layout()'s and is read by fd_batch.hip alone.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace tamcmc {

inline size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }  // every region of the block starts on a multiple of 16

// What a caller has for the batch; any pointer may be null (its area stays zero).  Sizes: params [C x Np], hstep and index_to_relax
// [Nvars], priors [4 x Np], priors_switch [Np], extra_priors [10], plength [11].
struct FdInputs {
    const double *params = nullptr, *hstep = nullptr, *priors = nullptr, *extra_priors = nullptr;
    const int32_t *index_to_relax = nullptr, *priors_switch = nullptr, *plength = nullptr;
};

// The results of the B = C (Nvars + 1) slots, in a host copy of the block or in the device block itself (then not to be read on the host)
struct FdResults {
    const double *lpp = nullptr, *lpm = nullptr;  // log-prior at the evaluation point / at theta - h e_k
    const int *status = nullptr;
    int B = 0;
    int first_status() const {  // the first status that is not TAMCMC_OK (0), in slot order
        for (int s = 0; s < B; s++)
            if (status[s] != 0) return status[s];
        return 0;
    }
};

// Offsets from the start of the block, each a multiple of 16: inputs [0, in_bytes) in the order of the members, results
// [in_bytes, in_bytes + out_bytes) behind them
struct FdBlockHead {
    size_t o_params = 0, o_h = 0, o_pr = 0, o_ex = 0, o_pl = 0, o_idx = 0, o_sw = 0, in_bytes = 0;
    size_t o_lpp = 0, o_lpm = 0, o_st = 0, out_bytes = 0;
    size_t C = 0, Np = 0, Nvars = 0;
    FdBlockHead() = default;
    FdBlockHead(int C_, int64_t Np_, int Nvars_) : C((size_t)C_), Np((size_t)Np_), Nvars((size_t)Nvars_) {
        const size_t B = C * (Nvars + 1);
        size_t o = 0;
        o_params = o; o = al16(o + C * Np * 8);
        o_h = o; o = al16(o + Nvars * 8);
        o_pr = o; o = al16(o + 4 * Np * 8);
        o_ex = o; o = al16(o + 10 * 8);
        o_pl = o; o = al16(o + 11 * 4);
        o_idx = o; o = al16(o + Nvars * 4);
        o_sw = o; o = al16(o + Np * 4);
        in_bytes = o;
        o_lpp = o; o = al16(o + B * 8);
        o_lpm = o; o = al16(o + B * 8);
        o_st = o; o = al16(o + B * 4);
        out_bytes = o - in_bytes;
    }
    // the input area of a host block: zeros, then what the caller has
    void stage(unsigned char *hb, const FdInputs &in) const {
        memset(hb, 0, in_bytes);
        if (in.params) memcpy(hb + o_params, in.params, C * Np * 8);
        if (in.hstep) memcpy(hb + o_h, in.hstep, Nvars * 8);
        if (in.priors) memcpy(hb + o_pr, in.priors, 4 * Np * 8);
        if (in.extra_priors) memcpy(hb + o_ex, in.extra_priors, 10 * 8);
        if (in.plength) memcpy(hb + o_pl, in.plength, 11 * 4);
        if (in.index_to_relax) memcpy(hb + o_idx, in.index_to_relax, Nvars * 4);
        if (in.priors_switch) memcpy(hb + o_sw, in.priors_switch, Np * 4);
    }
    // block: the start of a block (device, or a host copy of at least in_bytes + out_bytes)
    double *hstep(unsigned char *block) const { return (double *)(block + o_h); }  // (the device Langevin step writes its steps there)
    FdResults results(const unsigned char *block) const {
        FdResults r;
        r.lpp = (const double *)(block + o_lpp); r.lpm = (const double *)(block + o_lpm); r.status = (const int *)(block + o_st);
        r.B = (int)(C * (Nvars + 1));
        return r;
    }
};

}  // namespace tamcmc
