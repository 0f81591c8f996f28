// fd_batch.h -- one gradient batch (C chains x (Nvars + 1) evaluations) as an object: the route it takes (fd_route.h), the layout of its
// device block, its workspace, and its launch from parameter vectors already on the device (fd_batch.hip).  Used by the host entry points
// (tamcmc_hip_fd_gradient*, tamcmc_hip_adjoint_table, tamcmc_hip_fisher) and by the device-resident Langevin step (dev_sampler.hip: run_mala).
// Who owns what: the head of the block -- the arrays a caller fills and reads back -- is fd_block.h's (FdBlockHead: offsets, stage(),
// results()); the host entries go through begin() / finish() and never see an offset.  Everything behind the head (tables, delta tables,
// adjoint workspace) is layout()'s and is read by fd_batch.hip alone.  What a finished batch's sums become -- logL0, logPr0, grad,
// grad_prior -- is grad_assemble.h's (host only: assemble_gradient, tempered_loglike), shared with the envelope fits (envelope.hip), whose
// two gradient entries fd_batch.hip hands to envelope_gradient() unread.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctx.h"
#include "fd_block.h"
#include "fd_rgb_chunk.h"
#include "fd_route.h"
#include "rgb_prestep.h"

namespace tamcmc {

struct FdBatch {
    using Route = FdRoute;
    using Request = FdRequest;
    int model_id = 0, prior_class = 0, C = 0, E = 0, B = 0, Nvars = 0, per = 0, stride = 1, ntiles = 0;
    int64_t Np = 0;
    Route route = Route::Brute;
    bool deltas() const { return route == Route::Windowed || route == Route::Adjoint; }  // S = C base sums, then B differences against them
    // Red giants on the adjoint route (TAMCMC_OPT_RGB_ADJOINT): the hybrid batch.  Windowed's layout and launches -- k_fd_compare also
    // classifies every slot (adj_rgb_match.h) and leaves an empty delta entry for a linearisable one --, then the adjoint of the C base
    // tables; k_adj_contract is the one writer of S[C + slot]: its contraction for a linearisable slot, the DELTA launch's sum (folded
    // into S[C + B + slot], scratch) for a fallback slot, 0 for a base slot
    bool hybrid() const { return route == Route::Adjoint && rgb; }
    bool tables_only = false;  // Request::Tables: enqueue() stops after the batch's table builder
    // Route::Rows: the caller passes 2 N "variables" for its N, idx = [index_to_relax, index_to_relax], h = [+h, -h]: slot c*E + 1 + k is
    // theta + h_k e_k, slot c*E + 1 + N + k is theta - h_k e_k.
    // What enqueue() needs beside the block, in doubles.  part: tile partials; S: the sums; model: the base points' planes 1/M0, y/M0, M0
    // (Adjoint), + tile moments in two layouts + done flags (Windowed), the B model rows (Rows); bg: background series, FAST arithmetic only
    struct Workspace { size_t part = 0, S = 0, model = 0, bg = 0; } ws;
    struct Buffers { DevBuf<double> &part, &S, &model, &bg; };  // the context's d_part, d_S, d_model, d_bg, or a sampler's own
    hipError_t reserve(const tamcmc_hip_ctx *c, const Buffers &w) const;  // (model only when needed, bg only under TAMCMC_PRECISION_FAST)
    int table_slots() const { return (route == Route::Windowed && !rgb) ? 2 * B : B; }  // Windowed: slots [B, 2B) = per-block copies of the base table (not for red giants)
    bool rgb = false;  // red-giant models (ids 25 / 27): tables through the device pre-step, `chunk` vectors at a time
    int chunk = 0;
    // red giants: the host's long-double scalar unpack of the B vectors (rgb::Prep[B], rgb::RowIn[B], the table block's header with counts
    // and noise rows; pinned memory that outlives the launches), uploaded by enqueue instead of the device unpack; nullptr: the device
    // unpacks, in double.  STRICT promises the reference's long-double unpack, so under STRICT enqueue() REQUIRES these (it returns
    // TAMCMC_ERR_BAD_ARG without them): a caller whose vectors live on the device only cannot run a STRICT red-giant batch.
    const void *h_prep = nullptr, *h_rows = nullptr, *h_header = nullptr;
    // the device block: its head (fd_block.h: host-filled constants [0, in_bytes), results [in_bytes, in_bytes + out_bytes)), tables after
    FdBlockHead head;
    size_t o_tab = 0, o_dtab = 0, o_btab = 0, o_drange = 0, o_dflags = 0, o_drow = 0, o_dnold = 0, total_bytes = 0;
    size_t o_adjG = 0, o_adjGn = 0, o_adjpart = 0, o_adjGpart = 0;  // adjoint workspace inside the block: G [C x per x 17], Gn [C x stride], noise tile partials, row segment partials
    int adj_ntn = 0, adj_nseg = 0;
    // Route::Rows of a red giant (TAMCMC_OPT_RGB_FISHER; N = Nvars / 2 variables): the three candidate step reciprocals [3 x C x N] the
    // caller uploads, the ones k_fisher_freeze_rgb chose [C x N], and three integers -- the (chain, variable) pairs that took the central,
    // the one-sided and the unfrozen form -- which the kernel adds to when count_forms is set (the caller zeroes and reads them)
    size_t o_frh3 = 0, o_frh = 0, o_fcount = 0;
    bool count_forms = false;
    size_t o_adjcount = 0;  // hybrid: two integers, the perturbed slots k_adj_contract contracted / took from the DELTA launch (count_slots)
    int layout(tamcmc_hip_ctx *c, Request request, int model_id, int prior_class, int C, int64_t Nparams, const int32_t *plength, int Nvars);
    // block: the batch's device block (total_bytes), constants in place; d_params: C x Np parameter vectors on the device (nullptr: the
    // block's own params area); w: reserve()d.  ev0 / ev1 (optional) bracket the likelihood launches.  split (optional, hybrid batches: 7
    // events) marks the stages: start, tables, base launch, fallback delta, row pass, noise pass + fold, contraction
    int enqueue(tamcmc_hip_ctx *c, unsigned char *block, const double *d_params, const Buffers &w, hipEvent_t ev0, hipEvent_t ev1,
                hipEvent_t *split = nullptr);
    // The host entries' way round enqueue(), on the context's own blocks (h_fd, d_fd) and workspace.  begin: the inputs staged and
    // uploaded (red giants under STRICT: the host's long-double unpack too), the workspace reserved unless tables_only; *block is what
    // enqueue() takes.  finish: the results copied back behind whatever the caller enqueued after the batch, the stream synchronised
    int begin(tamcmc_hip_ctx *c, const FdInputs &in, unsigned char **block);
    int finish(tamcmc_hip_ctx *c, FdResults *out);
    // enqueue() as a host entry calls it between the two: the block's own vectors, the workspace begin() reserved
    int enqueue(tamcmc_hip_ctx *c, unsigned char *block, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, hipEvent_t *split = nullptr) {
        return enqueue(c, block, nullptr, context_buffers(c), ev0, ev1, split);
    }
    static Buffers context_buffers(tamcmc_hip_ctx *c) { return Buffers{c->d_part, c->d_S, c->d_model, c->d_bg}; }
    // hybrid: k_adj_contract counts the perturbed slots it contracted / took from the DELTA launch into two integers of the block
    // (o_adjcount) when count_slots is set.  The caller zeroes them once after laying the block out (zero_slot_counts); hybrid_stats
    // reads them and zeroes them again (it synchronises the stream)
    bool count_slots = false;
    hipError_t zero_slot_counts(tamcmc_hip_ctx *c, unsigned char *block) const { return hipMemsetAsync(block + o_adjcount, 0, 16, c->stream); }
    hipError_t hybrid_stats(tamcmc_hip_ctx *c, unsigned char *block, long *linearised, long *fallback) const;
    // Windowed, after the batch has finished (synchronous copies; roofline bookkeeping): bins the DELTA launch really walked -- the affected
    // ranges less the far-only tiles taken from the base point's moments -- and (full != nullptr) its "full table" evaluations
    hipError_t delta_stats(const unsigned char *block, long *bins, long *full) const;
    // [B x ntiles] flags of the last enqueue (device memory, inside `model`): 1 = that (evaluation, tile) was a far-only tile; nullptr: no such pass
    const unsigned char *d_done = nullptr;
    int tile_bins_ = 0;
};

// The argument checks the gradient entries share, after the context and the model: spectrum, counts, pointers, layout, variables.
// rest_ok: the entry's own pointers (outputs, priors) are there.  GA_PLENGTH: plength required, and its sum must be Nparams.  GA_VARS:
// index_to_relax (in range) and hstep required.  GA_FISHER: 1 <= Nvars <= 16384 and no zero step.  GA_EMPTY_FIRST: an empty batch
// (C == 0) is accepted before plength and the variables are looked at.
enum : unsigned { GA_PLENGTH = 1, GA_VARS = 2, GA_FISHER = 4, GA_EMPTY_FIRST = 8 };
int check_gradient_args(const tamcmc_hip_ctx *c, int C, const double *params, int64_t Nparams, const int32_t *plength,
                        const int32_t *index_to_relax, int Nvars, const double *hstep, bool rest_ok, unsigned rules);

}  // namespace tamcmc
