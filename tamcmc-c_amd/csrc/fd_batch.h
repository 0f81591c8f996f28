// fd_batch.h -- one finite-difference batch (C chains x (Nvars + 1) evaluations) as an object: layout of its device block, launch from
// parameter vectors already on the device (fd_batch.hip).  Three routes: brute force, windowed delta tables, table-space adjoint.  Used by the host entry points (tamcmc_hip_fd_gradient*) and by the
// device-resident Langevin step (dev_mala.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctx.h"
#include "fd_rgb_chunk.h"

namespace tamcmc {

struct FdBatch {
    int model_id = 0, prior_class = 0, C = 0, E = 0, B = 0, Nvars = 0, per = 0, stride = 1, ntiles = 0;
    int64_t Np = 0;
    bool windowed = false;
    // TAMCMC_OPT_GRADIENT = TAMCMC_GRADIENT_ADJOINT: no perturbed likelihood at all.  The C base points are evaluated as in the windowed
    // route (same launch, same planes), the table-space adjoint G / Gn of each is taken in one pass over its windows (adjoint.h), and the
    // "difference" of evaluation e is the contraction of G / Gn with (table e - base table), written where the DELTA launch writes its
    // difference -- so the sums read like the windowed route's (deltas()).  `windowed` is then false: no delta tables exist.
    bool adjoint = false;
    bool deltas() const { return windowed || adjoint; }  // S = C base sums, then B differences against them
    // Fisher rows (fisher.h; set BEFORE layout(), off by default): neither windowed nor adjoint whatever the context's options say; enqueue()
    // stops after the tables -- every perturbed table gets its base table's windows [i0, i1) ("frozen window", k_fisher_freeze) -- and ONE
    // likelihood launch that leaves the B model rows in `model` ([B x Nx]; the sums S are not formed).  The caller passes 2 Nvars "variables":
    // idx = [index_to_relax, index_to_relax], h = [+h, -h], so with N the caller's variables (this batch's Nvars / 2) slot c*E + 1 + k is theta + h_k e_k and slot c*E + 1 + N + k is theta - h_k e_k.
    bool rows_only = false;
    size_t model_doubles = 0;  // doubles of `model` that enqueue() needs (0: none)
    size_t bg_rows = 0;        // rows of `bgbuf` (x ntiles x 8 doubles) under FAST arithmetic
    bool rgb = false;  // red-giant models (ids 25 / 27): tables through the device pre-step, `chunk` vectors at a time
    int chunk = 0;
    // red giants: the host's long-double scalar unpack of the B vectors (rgb::Prep[B], rgb::RowIn[B], the table block's header with counts
    // and noise rows; pinned memory that outlives the launches), uploaded by enqueue instead of the device unpack; nullptr: the device
    // unpacks, in double.  STRICT promises the reference's long-double unpack, so under STRICT enqueue() REQUIRES these (it returns
    // TAMCMC_ERR_BAD_ARG without them): a caller whose vectors live on the device only cannot run a STRICT red-giant batch.
    const void *h_prep = nullptr, *h_rows = nullptr, *h_header = nullptr;
    // offsets inside the device block: host-filled constants [0, in_bytes), results [in_bytes, in_bytes + out_bytes), tables after
    size_t o_params = 0, o_h = 0, o_pr = 0, o_ex = 0, o_pl = 0, o_idx = 0, o_sw = 0, in_bytes = 0;
    size_t o_lpp = 0, o_lpm = 0, o_st = 0, out_bytes = 0;
    size_t o_tab = 0, o_dtab = 0, o_btab = 0, o_drange = 0, o_dflags = 0, o_drow = 0, o_dnold = 0, total_bytes = 0;
    size_t o_adjG = 0, o_adjGn = 0, o_adjpart = 0, o_adjGpart = 0;  // adjoint workspace inside the block: G [C x per x 17], Gn [C x stride], noise tile partials, row segment partials
    int adj_ntn = 0, adj_nseg = 0;
    size_t nS = 0;  // sums the batch produces: C base sums + B differences (deltas()) or B full sums
    int layout(tamcmc_hip_ctx *c, int model_id, int prior_class, int C, int64_t Nparams, const int32_t *plength, int Nvars);
    int enqueue(tamcmc_hip_ctx *c, unsigned char *block, const double *d_params, double *part, double *S, double *model, double *bgbuf,
                hipEvent_t ev0, hipEvent_t ev1);
    // [B x ntiles] flags of the last enqueue (device memory, inside `model`): 1 = that (evaluation, tile) was a far-only tile taken from
    // the base point's moments -- no bin of it was read; nullptr: no such pass (roofline bookkeeping: bins_not_walked)
    const unsigned char *d_done = nullptr;
    int tile_bins_ = 0;
    long bins_not_walked() const;  // (synchronous copy; call after the batch has finished)
};
int fd_ensure_poly(tamcmc_hip_ctx *c);  // Pslm/Qlm tables in c->d_poly

}  // namespace tamcmc
