// fd_batch.hip -- gradient batches built ON the device.
//
// The forward-difference gradient (the drift the reference leaves as a stub, MALA.cpp:321-337) needs, per chain,
// Nvars+1 evaluations.  Building those tables on the host costs far more than evaluating them (C3: 1880 tables,
// ~20 us each, against ~4 ms of likelihood kernel); here one workgroup per (chain, perturbed variable) perturbs the
// parameter vector, evaluates the log-prior (and the prior at the backward point, for the one-sided fallback at the
// edge of a prior's support) and writes its multiplet table straight into the likelihood kernel's input block.
// A batch is: the tables (build_tables), then what its route (FdBatch::Route, fd_route.h) does with them; every route begins with the
// same launch on some of the tables (evaluate_tables):
//   Brute     k_fd_unpack -> k_loglike on all B = C*(Nvars+1) tables -> k_finalize;
//   Windowed  (FAST arithmetic: the default) k_fd_unpack -> k_fd_compare (delta tables) -> k_loglike on the C base points (planes 1/M0,
//             y/M0, M0 kept) -> k_finalize -> k_fd_moments (tile moments of the base points) -> k_fd_far (far-only tiles of the light
//             evaluations from the moments) -> k_loglike<DELTA> (everything else) -> k_finalize;
//   Adjoint   (TAMCMC_OPT_GRADIENT = TAMCMC_GRADIENT_ADJOINT; FAST arithmetic, fixed-length tables) k_fd_unpack -> k_adj_base -> k_loglike
//             on the C base points (planes kept) -> k_finalize -> k_adj_rows, k_adj_noise, k_adj_fold (adjoint.hip: dS/d(table entry) of
//             each base point) -> k_adj_contract (dS of every perturbed table to first order, frozen windows);
//             Red giants (TAMCMC_OPT_RGB_ADJOINT = 1), the HYBRID batch: a perturbation may change the set of mixed modes, and the rows
//             after the change then no longer correspond.  Windowed's layout and launches with the adjoint between them and the sums:
//             k_fd_rgb_perturb -> rgb_device_stage -> k_fd_compare, which first classifies the slot (adj_rgb_match.h: same row count,
//             same l row by row, every l=1 row within half the distance to its nearest l=1 neighbour) and leaves an EMPTY delta entry
//             with ADJ_RGB_FLAG_LINEAR in d_flags for a linearisable slot, its normal entry otherwise -> the windowed base launch,
//             argument for argument -> k_finalize -> k_fd_moments, k_fd_far, k_loglike<DELTA> (all but the fallback slots' tiles leave
//             at once) -> k_finalize into scratch sums S[C + B ..) -> k_adj_rows, k_adj_noise, k_adj_fold on the C base tables ->
//             k_adj_contract, the ONE writer of S[C + slot]: the contraction (linearisable), the scratch sum as it is (fallback), 0
//             (base), NaN (a failed table).  The moments are taken for every chain: which chains have a fallback slot is known on the
//             device only.  The row pass keeps its (segment, row, chain) grid: see DESIGN section 9 for what a work list cost;
//   Rows      (tamcmc_hip_fisher) k_fd_unpack -> k_fisher_freeze (every perturbed table gets its base table's windows) -> k_loglike on
//             all B tables, model rows kept, no sums.  Red giants (TAMCMC_OPT_RGB_FISHER = 1): k_fd_rgb_perturb -> rgb_device_stage ->
//             k_fisher_freeze_rgb (per chain and variable, both sides classified as the hybrid batch classifies a slot: windows frozen,
//             a side replaced by the base table, or both left alone -- fisher_rgb_rule.h) -> the same launch.
// Red-giant models (ids 25 / 27): the table of a vector needs the mixed-mode solver, so k_fd_unpack's place is taken by
//   k_fd_rgb_perturb (perturbed vector, class-4 log-prior, scalar unpack into the pre-step workspace) -> rgb_device_stage (solver, rows),
// in chunks of vectors through ONE workspace slice; everything after the tables is the same.
// Who owns what.  The head of the device block (inputs, results) is fd_block.h's; the host entries here and in fisher.hip reach it through
// FdBatch::begin() / finish(), the device sampler through FdBlockHead::stage() / results().  The rest of the block is layout()'s, read
// by enqueue() and the audit copies of this file.  The red-giant front end inside k_fd_rgb_perturb is rgb_front.h's, shared with the
// sampler's proposal kernel; the polynomial tables are ensure_poly()'s (rgb_prestep.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "envelope.h"
#include "dev_unpack.h"
#include "kernels.h"
#include "fd_batch.h"
#include "grad_assemble.h"
#include "rgb_prestep.h"
#include "rgb_front.h"
#include "adjoint.h"
#include "adj_rgb_match.h"
#include "fisher.h"

namespace tamcmc {
namespace {

constexpr int FB = 128;

struct FdArgs {
    ModelDesc desc;
    TablePtrs T;
    int C, E, Nv;
    const double *params;  // [C x Np]
    const int *idx;        // [Nv] index_to_relax
    const double *h;       // [Nv] steps
    double *logPr_plus;    // [C x E] log-prior at the evaluation point (e=0: the base point)
    double *logPr_minus;   // [C x E] log-prior at theta - h e_k (e>=1)
    int *status;           // [C x E]
    // windowed mode (delta tables): rows [B*per, 2B*per) of T.mults hold each block's copy of the BASE table (red giants: no copies,
    // the base table of chain c is slot c*E itself: base_copies = 0),
    // D is the delta launch's input block (2*per rows per evaluation: +new / -old of the changed multiplets)
    int windowed, base_copies;
    TablePtrs D;
    int *d_range, *d_flags, *d_row;
    double *d_noise_old;
    TablePtrs Bs;          // base launch (C evaluations): ranges / counts / noise rows indexed by chain
    int full_tables;       // 1: "full table" delta evaluations allowed (the base launch's background series are at hand: FAST arithmetic)
    int hybrid;            // 1: red giants on the adjoint route -- k_fd_compare classifies the slot first (adj_rgb_match.h)
};

__global__ void __launch_bounds__(FB) k_fd_unpack(const FdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int Np = a.desc.Np;
    double *s_params = (double *)s_raw;
    const UnpackLds U = carve_unpack_lds((unsigned char *)(s_params + Np));
    const int slot = blockIdx.x, c = slot / a.E, e = slot - c * a.E, tid = threadIdx.x;
    const int B = a.C * a.E;
    for (int i = tid; i < Np; i += FB) s_params[i] = a.params[(size_t)c * Np + i];
    unpack_begin(a.desc, U);
    if (a.windowed && e > 0) {
        // this block's own copy of the BASE table (slot B+slot): k_fd_compare finds the changed rows by comparing with it
        if (tid == FB - 1) mt::shared_scalars_base(a.desc.model_id, s_params, a.desc.plength, *U.S);
        __syncthreads();
        wg_unpack(a.desc, s_params, U, B + slot, a.T, true);
        __syncthreads();
        if (tid == 0) { *U.status = TAMCMC_OK; *U.reject = 0; }
        __syncthreads();
    }
    const bool with_prior = a.desc.prior_class != 0;
    const int ip = e > 0 ? a.idx[e - 1] : 0;
    const double x0 = e > 0 ? a.params[(size_t)c * Np + ip] : 0.0, hh = e > 0 ? a.h[e - 1] : 0.0;
    if (e > 0) {
        if (tid == 0) s_params[ip] = x0 + hh;
        __syncthreads();
    }
    double lp = 0.0;
    if (with_prior) lp = wg_log_prior(a.desc, s_params, U, true);
    else {
        if (tid == FB - 1) mt::shared_scalars_base(a.desc.model_id, s_params, a.desc.plength, *U.S);
        __syncthreads();
    }
    // the likelihood is evaluated whatever the prior says: the caller combines the parts.  A prior the device cannot evaluate (an unsupported
    // id or option: TAMCMC_ERR_BAD_MODEL, as tamcmc_log_prior says) is not a "-inf": its status is kept across the reset and fails the slot
    int st_prior = TAMCMC_OK;
    if (tid == 0) { st_prior = *U.status; *U.status = TAMCMC_OK; }
    __syncthreads();
    wg_unpack(a.desc, s_params, U, slot, a.T, true);
    if (tid == 0) {
        a.logPr_plus[slot] = lp;
        a.status[slot] = st_prior != TAMCMC_OK ? st_prior : *U.status;
    }
    // the log-prior at theta - h e_k is only ever looked at when the forward point lies outside a prior's support (one-sided fallback of
    // the gradient's prior share): evaluated in that case alone (workgroup-uniform: every lane holds the same lp)
    double lp_minus = 0.0;
    if (e > 0 && with_prior && !isfinite(lp)) {
        __syncthreads();
        if (tid == 0) { s_params[ip] = x0 - hh; *U.reject = 0; }
        __syncthreads();
        lp_minus = wg_log_prior(a.desc, s_params, U, false);
    }
    if (tid == 0) a.logPr_minus[slot] = lp_minus;
}

// Red-giant models (ids 25 / 27), the counterpart of k_fd_unpack up to the table: one workgroup per slot of the chunk [slot0, slot0 + gridDim.x).
// The perturbed vector is staged in LDS and goes through the red-giant front end (rgb_front.h, shared with the device sampler's proposal
// kernel) on this kernel's own schedule: the whole class-4 log-prior by the first wave while the second runs the scalar unpack of the
// same vector, published into entry blockIdx.x of the pre-step workspace slice; rgb_device_stage builds the table from there.
// The likelihood is evaluated whatever the prior says (the caller combines the parts), so an infinite prior does not empty the entry.
// host_unpack (STRICT, host entry): the workspace entries, noise rows and counts were filled by the host's long-double unpack and uploaded
// (fd_run); the kernel then only evaluates the prior and resets the solver's counters.
__global__ void __launch_bounds__(FB) k_fd_rgb_perturb(const FdArgs a, const rgb::Slice rs, const int slot0, const int host_unpack) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int Np = a.desc.Np;
    double *s_params = (double *)s_raw;
    mt::xreal *terms = (mt::xreal *)(s_params + Np);  // [Np] generic prior terms (xreal = double on the device)
    __shared__ rgb::FrontLds F;
    const int rb = blockIdx.x, slot = slot0 + rb, c = slot / a.E, e = slot - c * a.E, tid = threadIdx.x;
    const bool with_prior = a.desc.prior_class != 0;
    for (int i = tid; i < Np; i += FB) s_params[i] = a.params[(size_t)c * Np + i];
    const int ip = e > 0 ? a.idx[e - 1] : 0;
    const double x0 = e > 0 ? a.params[(size_t)c * Np + ip] : 0.0, hh = e > 0 ? a.h[e - 1] : 0.0;
    if (tid == 0) { F.stp = TAMCMC_OK; F.lp = 0.0; }
    __syncthreads();
    if (e > 0 && tid == 0) s_params[ip] = x0 + hh;
    __syncthreads();
    // log-prior of the vector in LDS: the same value in every lane.  All of it is wave 0's -- the generic terms one per lane, a wavefront
    // barrier, the serial tail on lane 0 -- so that it runs beside wave 1's scalar unpack; the workgroup meets at the one barrier at the end
    auto log_prior = [&]() -> double {
        if (tid < 64) {
            for (int i = tid; i < Np; i += 64) {
                int st = TAMCMC_OK;
                terms[i] = pr::generic_prior_term(s_params, Np, a.desc.priors, a.desc.priors_switch, i, &st);
                if (st != TAMCMC_OK) F.stp = st;
            }
            WaveSync()();
            if (tid == 0) rgb::front_prior_serial(a.desc, s_params, terms, F.stp, F);
        }
        __syncthreads();
        return F.lp;
    };
    // wave 1: the scalar unpack, while wave 0 is in log_prior() below
    if ((tid >> 6) == 1 && !host_unpack) rgb::front_unpack(a.desc, s_params, rs, F);
    const double lp = with_prior ? log_prior() : 0.0;
    __syncthreads();
    // a prior the device cannot evaluate: the slot fails (status, NaN); an infinite one changes nothing here
    if (host_unpack) {
        if (tid == 0) {
            if (F.stp != TAMCMC_OK) { rs.preps[rb].status = F.stp; rs.rows[rb].status = F.stp; }
            rgb::front_reset(rs, rb);
        }
    } else {
        if (tid == 0 && F.stp != TAMCMC_OK) { F.P.status = F.stp; F.R.status = F.stp; }
        __syncthreads();
        rgb::front_publish<FB>(F, rs, rb, slot, a.desc.stride, a.T.noise, a.T.nh, a.T.nn);
    }
    if (tid == 0) a.logPr_plus[slot] = lp;
    // the log-prior at theta - h e_k: only where the forward point lies outside a prior's support (as k_fd_unpack; workgroup-uniform)
    double lp_minus = 0.0;
    if (e > 0 && with_prior && !isfinite(lp)) {
        __syncthreads();
        if (tid == 0) s_params[ip] = x0 - hh;
        __syncthreads();
        lp_minus = log_prior();
    }
    if (tid == 0) a.logPr_minus[slot] = lp_minus;
}

// The base launch's index (C evaluations, model rows written): chain c's ranges, counts and noise row are those of its base slot c*E --
// the launch reads the SAME table rows.  By one workgroup of NT lanes.
template <int NT>
__device__ __forceinline__ void write_base_index(const FdArgs &a, int c, int tid) {
    const int slot = c * a.E, stride = a.desc.stride;
    if (tid == 0) {
        a.Bs.pairs[2 * c] = a.T.pairs[2 * slot];
        a.Bs.pairs[2 * c + 1] = a.T.pairs[2 * slot + 1];
        a.Bs.nh[c] = a.T.nh[slot];
        a.Bs.nn[c] = a.T.nn[slot];
    }
    for (int i = tid; i < stride; i += NT) a.Bs.noise[(size_t)c * stride + i] = a.T.noise[(size_t)slot * stride + i];
}

// An empty delta entry: no row, no bin, the slot's class in d_flags (0, or ADJ_RGB_FLAG_LINEAR for a slot the adjoint contracts).  One lane.
__device__ __forceinline__ void write_empty_delta(const FdArgs &a, int slot, int c, int flags) {
    a.D.pairs[2 * slot] = 0; a.D.pairs[2 * slot + 1] = 0; a.D.nh[slot] = 0; a.D.nn[slot] = 1;
    a.d_range[2 * slot] = 0; a.d_range[2 * slot + 1] = 0; a.d_flags[slot] = flags; a.d_row[slot] = c;
}

// Windowed mode, after the tables: one workgroup per slot compares slot e's finished table with the chain's base table row by row and writes
// the delta launch's input -- it reads two tables and does not care which builder made them.  The tables may differ in length (a red-giant
// perturbation can change the number of mixed modes: every row after the first difference then differs, and the rows beyond the end of the
// shorter table count as changed against an absent row).
__global__ void __launch_bounds__(FB) k_fd_compare(const FdArgs a) {
    const int slot = blockIdx.x, c = slot / a.E, e = slot - c * a.E, tid = threadIdx.x;
    const int B = a.C * a.E, per = a.desc.per, stride = a.desc.stride;
    __shared__ int s_lo, s_hi, s_noise_chg, s_nrows, s_wtot[FB / 64], s_moved;
    if (e == 0) {
        // base evaluation of chain c: its entry of the base launch's index, and no delta work for this slot
        write_base_index<FB>(a, c, tid);
        if (tid == 0) write_empty_delta(a, slot, c, 0);
        return;
    }
    // ---- delta table: the multiplets whose row differs from the base row, +new / -old, and the affected bin range ----
    const int bs = a.base_copies ? B + slot : c * a.E;  // the slot holding the base table
    const int n_new = a.T.pairs[2 * slot + 1] - a.T.pairs[2 * slot], n_old = a.T.pairs[2 * bs + 1] - a.T.pairs[2 * bs];
    if (a.hybrid) {
        // hybrid batch: a slot whose rows correspond one to one with the base table's is the adjoint's -- an empty delta entry (as e = 0
        // above) with its class in d_flags, and k_adj_contract writes its difference; every other slot goes on as in the windowed route
        const bool same = a.status[slot] == TAMCMC_OK && a.status[bs] == TAMCMC_OK && n_new == n_old;  // (uniform)
        if (tid == 0) s_moved = 0;
        __syncthreads();
        if (same) {
            const tamcmc_multiplet *base = a.T.mults + (size_t)bs * per, *pert = a.T.mults + (size_t)slot * per;
            for (int j = tid; j < n_old && j < per; j += FB)
                if (!adj_rgb_row_matches(base, pert, n_old, j)) s_moved = 1;  // (every writer stores the same value)
        }
        __syncthreads();
        if (same && !s_moved) {
            if (tid == 0) write_empty_delta(a, slot, c, ADJ_RGB_FLAG_LINEAR);
            return;
        }
    }
    if (tid == 0) { s_lo = a.desc.Nx; s_hi = 0; s_noise_chg = 0; s_nrows = 0; }
    __syncthreads();
    const bool ok = (a.status[slot] == TAMCMC_OK) && (n_old > 0);  // (a base table that failed is empty)
    tamcmc_multiplet *drows = a.D.mults + (size_t)slot * 2 * per;
    for (int i = tid; i < stride; i += FB) {
        const double vn = a.T.noise[(size_t)slot * stride + i], vo = a.T.noise[(size_t)bs * stride + i];
        a.D.noise[(size_t)slot * stride + i] = vn;
        a.d_noise_old[(size_t)slot * stride + i] = vo;
        if (ok && i < a.T.nn[slot] && vn != vo) s_noise_chg = 1;
    }
    // how row jdx changed: 0 not at all, 1 heights only (a parameter that only rescales heights -- inclination, visibilities, heights --
    // leaves frequencies, width, asymmetry and window untouched: +new and -old are then ONE row with the height differences), 2 otherwise;
    // 3 / 4: the row exists in the perturbed / the base table only
    auto change_of = [&](int jdx) -> int {
        if (!ok || jdx >= per) return 0;
        const bool has_n = jdx < n_new, has_o = jdx < n_old;
        if (!has_n || !has_o) return has_n ? 3 : (has_o ? 4 : 0);
        const unsigned long long *pn = (const unsigned long long *)&a.T.mults[(size_t)slot * per + jdx];
        const unsigned long long *po = (const unsigned long long *)&a.T.mults[(size_t)bs * per + jdx];
        bool chg = false;
        for (int w = 0; w < (int)(sizeof(tamcmc_multiplet) / 8); w++) chg = chg || (pn[w] != po[w]);
        if (!chg) return 0;
        const tamcmc_multiplet &rn = a.T.mults[(size_t)slot * per + jdx], &ro = a.T.mults[(size_t)bs * per + jdx];
        bool amp_only = (rn.l == ro.l) && (rn.i0 == ro.i0) && (rn.i1 == ro.i1) && (rn.fc == ro.fc) && (rn.gamma == ro.gamma) && (rn.asym == ro.asym);
        for (int m = 0; m < 7; m++) amp_only = amp_only && (rn.nu[m] == ro.nu[m]);
        return amp_only ? 1 : 2;
    };
    for (int j0 = 0; j0 < per; j0 += FB) {
        const int k = change_of(j0 + tid);
        if (k) atomicAdd(&s_nrows, k == 2 ? 2 : 1);  // rows the pair table would take
    }
    __syncthreads();
    // "full table": the pairs would be longer than the perturbed point's whole table (a parameter that moves most multiplets: a splitting
    // coefficient, the asymmetry, a red giant's period spacing) -- the delta launch then evaluates that table and subtracts the base model
    // row (loglike_tile.h)
    const bool full = ok && !s_noise_chg && a.full_tables && (s_nrows > n_new);
    int nchg = 0;
    if (full) {
        for (int jdx = tid; jdx < n_new; jdx += FB) drows[jdx] = a.T.mults[(size_t)slot * per + jdx];
    } else
        // the changed rows in table order (an ordered compaction: the delta launch sums the rows in the order they are stored, so the
        // result is the same from call to call): rows per lane -> scan over the wave -> wave totals in LDS
        for (int j0 = 0; j0 < per; j0 += FB) {
            const int jdx = j0 + tid, k = change_of(jdx), nr = (k == 2) ? 2 : (k ? 1 : 0);
            int inc = nr;
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(inc, off, 64);
                if ((tid & 63) >= off) inc += up;
            }
            if ((tid & 63) == 63) s_wtot[tid >> 6] = inc;
            __syncthreads();
            int pos = nchg + inc - nr;
            for (int w = 0; w < FB / 64; w++) {
                if (w < (tid >> 6)) pos += s_wtot[w];
                nchg += s_wtot[w];
            }
            if (k) {
                // rows move as 8-byte words, global to global (no private copy of a row): 12 words of degree, window, centre, width,
                // asymmetry and frequencies, then the 7 heights -- differences (k = 1), as they are (+new) or negated (-old)
                constexpr int NW = (int)(sizeof(tamcmc_multiplet) / 8), HV = NW - 7;
                const tamcmc_multiplet *rn = &a.T.mults[(size_t)slot * per + jdx], *ro = &a.T.mults[(size_t)bs * per + jdx];
                const unsigned long long *wn = (const unsigned long long *)rn, *wo = (const unsigned long long *)ro;
                int lo = a.desc.Nx, hi = 0;
                if (k != 4) {
                    lo = rn->i0; hi = rn->i1;
                    if (k != 1) {
                        unsigned long long *d = (unsigned long long *)&drows[pos];
                        for (int w = 0; w < NW; w++) d[w] = wn[w];
                    }
                }
                if (k != 3) {
                    lo = min(lo, ro->i0); hi = max(hi, ro->i1);
                    tamcmc_multiplet *dr = &drows[pos + (k == 2 ? 1 : 0)];
                    unsigned long long *d = (unsigned long long *)dr;
                    for (int w = 0; w < HV; w++) d[w] = wo[w];
                    for (int m = 0; m < 7; m++) dr->hv[m] = (k == 1) ? rn->hv[m] - ro->hv[m] : -ro->hv[m];
                }
                atomicMin(&s_lo, lo);
                atomicMax(&s_hi, hi);
            }
            __syncthreads();  // (s_wtot is rewritten by the next pass)
        }
    __syncthreads();
    if (tid == 0) {
        const int n = full ? n_new : nchg;
        const bool all_bins = s_noise_chg || full;
        a.D.pairs[2 * slot] = slot * 2 * per;
        a.D.pairs[2 * slot + 1] = slot * 2 * per + n;  // n = rows written (one or two per changed multiplet, or the whole table)
        a.D.nh[slot] = a.T.nh[slot];
        a.D.nn[slot] = a.T.nn[slot];
        a.d_flags[slot] = s_noise_chg | (full ? 2 : 0);
        a.d_row[slot] = c;
        a.d_range[2 * slot] = all_bins ? 0 : (n ? s_lo : 0);
        a.d_range[2 * slot + 1] = all_bins ? a.desc.Nx : (n ? s_hi : 0);
    }
}

// Adjoint route: the base launch's index and nothing else -- there are no delta tables for k_fd_compare to write.
__global__ void __launch_bounds__(64) k_adj_base(const FdArgs a) { write_base_index<64>(a, blockIdx.x, threadIdx.x); }
}  // namespace
}  // namespace tamcmc

using namespace tamcmc;

// ---------------------------------------------------------------------------------------------------------------
// One gradient batch = C chains x (Nvars + 1) evaluations.  layout() chooses the route and places the batch's constants, tables and
// results in ONE device block; enqueue() launches the batch on the context's stream from parameter vectors that are ALREADY on the device
// and leaves the results there (the device-resident Langevin step, run_mala in dev_sampler.hip, consumes them in its next kernel);
// fd_run() is the host entry: upload, enqueue, download, gradient assembly.
namespace tamcmc {


int FdBatch::layout(tamcmc_hip_ctx *c, Request request, int model_id_, int prior_class_, int C_, int64_t Nparams, const int32_t *plength, int Nvars_) {
    model_id = model_id_; prior_class = prior_class_; C = C_; Np = Nparams; Nvars = Nvars_;
    rgb = is_rgb_model(model_id);
    E = Nvars + 1; B = C * E;
    if (int rc = fd_route(request, c->gradient, c->fd_windowed, c->precision, delta_geometry(c->wgs, c->K), Nvars, rgb, &route, c->rgb_adjoint != 0,
                          c->rgb_fisher != 0))
        return rc;
    tables_only = request == Request::Tables;
    // (the hybrid batch's fallback slots go through the DELTA launch, which exists for the default geometries only: 256 x 4, 64 x 8, 64 x 4)
    if (hybrid() && !delta_geometry(c->wgs, c->K)) return TAMCMC_ERR_BAD_ARG;
    if (rgb) {
        // red giants: the tables come from the device pre-step, whose workspace is ~28 KB per vector (Prep, RowIn, three arrays of
        // rgb::MAXSOL doubles).  Chunk rule: the batch goes through ONE workspace slice of at most FD_RGB_WORKSPACE bytes, in chunks of
        // fd_rgb_chunk() vectors (all of them at once while they fit: ~9500); sized here, once per layout
        if ((long)C * E > 65535) return TAMCMC_ERR_BAD_ARG;  // (the limit of the batched red-giant entry)
        if (plength[10] < 6) return TAMCMC_ERR_BAD_ARG;       // (the unpack reads six configuration values behind the inclination)
        chunk = fd_rgb_chunk(B, rgb_device_workspace_bytes(1), FD_RGB_WORKSPACE);
        const int rc = rgb_device_prepare(c, chunk, 1, plength, &per, &stride);
        if (rc) return rc;
    } else {
        per = mt::count_multiplets(model_id, plength);
        if (per < 0) return TAMCMC_ERR_BAD_MODEL;
        stride = plength[8] > 0 ? plength[8] : 1;
        if ((stride - 1) / 3 > TAMCMC_MAX_HARVEY) return TAMCMC_ERR_BAD_ARG;
    }
    head = FdBlockHead(C, Np, Nvars);
    size_t o = head.in_bytes + head.out_bytes;
    const int nslots = table_slots();
    const StageLayout L(nslots, stride, (size_t)nslots * per);
    o_tab = o; o = al16(o + L.bytes);
    o_dtab = o_btab = o_drange = o_dflags = o_drow = o_dnold = 0;
    if (route == Route::Windowed || hybrid()) {
        const StageLayout LD(B, stride, (size_t)B * 2 * per);      // delta launch input block
        const StageLayout LB(C, stride, 0);                        // base launch: ranges / counts / noise rows by chain
        o_dtab = o; o = al16(o + LD.bytes);
        o_btab = o; o = al16(o + LB.bytes);
        o_drange = o; o = al16(o + (size_t)2 * B * 4);
        o_dflags = o; o = al16(o + (size_t)B * 4);
        o_drow = o; o = al16(o + (size_t)B * 4);
        o_dnold = o; o = al16(o + (size_t)B * stride * 8);
    }
    o_adjG = o_adjGn = o_adjpart = o_adjGpart = 0;
    adj_ntn = adj_nseg = 0;
    o_adjcount = 0;
    if (route == Route::Adjoint) {
        const StageLayout LB(C, stride, 0);
        adj_ntn = (int)((c->Nx + ADJ_NTILE - 1) / ADJ_NTILE);
        if (!hybrid()) { o_btab = o; o = al16(o + LB.bytes); }  // (hybrid: Windowed's, above)
        o_adjG = o; o = al16(o + (size_t)C * per * ADJ_F * 8);
        o_adjGn = o; o = al16(o + (size_t)C * stride * 8);
        o_adjpart = o; o = al16(o + (size_t)C * adj_ntn * stride * 8);
        adj_nseg = (int)((c->Nx + ADJ_SEG - 1) / ADJ_SEG);
        o_adjGpart = o; o = al16(o + (size_t)C * per * adj_nseg * ADJ_F * 8);
        if (hybrid()) { o_adjcount = o; o = al16(o + 16); }
    }
    o_frh3 = o_frh = o_fcount = 0;
    if (route == Route::Rows && rgb) {
        const size_t n_rh = (size_t)C * (Nvars / 2);
        o_frh3 = o; o = al16(o + 3 * n_rh * 8);
        o_frh = o; o = al16(o + n_rh * 8);
        o_fcount = o; o = al16(o + 24);
    }
    total_bytes = o;
    const int tbins = tile_bins(c->wgs, c->K);
    ntiles = (int)((c->Nx + tbins - 1) / tbins);
    const size_t planes = 3 * (size_t)C * c->Nx;
    ws.S = deltas() ? (size_t)C + B : (size_t)B;
    ws.part = ws.S * ntiles * 2;
    if (hybrid()) ws.S += (size_t)B;  // (the DELTA launch's sums, before k_adj_contract puts the fallback slots' in place)
    ws.model = 0;
    if (route == Route::Adjoint) ws.model = planes;
    if (route == Route::Windowed || hybrid()) ws.model = planes + 2 * (size_t)C * ntiles * FD_MOM + ((size_t)B * ntiles + 7) / 8;
    if (route == Route::Rows) ws.model = (size_t)B * c->Nx;
    ws.bg = (deltas() ? (size_t)C : (size_t)B) * ntiles * 8;
    return TAMCMC_OK;
}

hipError_t FdBatch::reserve(const tamcmc_hip_ctx *c, const Buffers &w) const {
    hipError_t e = w.part.reserve(ws.part);
    if (e == hipSuccess) e = w.S.reserve(ws.S);
    if (e == hipSuccess && ws.model) e = w.model.reserve(ws.model);
    if (e == hipSuccess && c->precision == TAMCMC_PRECISION_FAST) e = w.bg.reserve(ws.bg);
    return e;
}

namespace {

TablePtrs table_ptrs(unsigned char *base, const StageLayout &Lx) {
    TablePtrs T;
    T.mults = (tamcmc_multiplet *)(base + Lx.off_mults); T.pairs = (int *)(base + Lx.off_pairs);
    T.nh = (int *)(base + Lx.off_nh); T.nn = (int *)(base + Lx.off_nn); T.noise = (double *)(base + Lx.off_noise);
    return T;
}

// The tables of the B vectors in fa.T (red giants: chunk by chunk through the pre-step, with the host's unpack uploaded where there is
// one), then what the route reads beside them: the delta tables (Windowed), the base launch's ranges / counts / noise rows by chain
// (Windowed, Adjoint).
int build_tables(tamcmc_hip_ctx *c, const FdBatch &b, unsigned char *db, const StageLayout &L, FdArgs &fa) {
    hipStream_t st = c->stream;
    if (b.rgb) {
        RgbDeviceTables R;
        R.mults = fa.T.mults; R.pairs = fa.T.pairs; R.nh = fa.T.nh; R.nn = fa.T.nn; R.noise = fa.T.noise; R.status = fa.status; R.stride = b.stride;
        const rgb::Slice rs = rgb_device_slice(c, b.chunk, 0);
        if (b.h_prep)  // counts and noise rows of the host unpack: the table block's header
            HIPCHK(c, hipMemcpyAsync(db + b.o_tab, b.h_header, L.off_mults, hipMemcpyHostToDevice, st));
        for (int b0 = 0; b0 < b.B; b0 += b.chunk) {  // (one stream: a chunk's solver and row kernels are done with the slice before the next chunk's unpack)
            const int n = b.B - b0 < b.chunk ? b.B - b0 : b.chunk;
            if (b.h_prep) {
                HIPCHK(c, hipMemcpyAsync(rs.preps, (const rgb::Prep *)b.h_prep + b0, (size_t)n * sizeof(rgb::Prep), hipMemcpyHostToDevice, st));
                HIPCHK(c, hipMemcpyAsync(rs.rows, (const rgb::RowIn *)b.h_rows + b0, (size_t)n * sizeof(rgb::RowIn), hipMemcpyHostToDevice, st));
            }
            hipLaunchKernelGGL(k_fd_rgb_perturb, dim3(n), dim3(FB), (size_t)b.Np * 16, st, fa, rs, b0, b.h_prep ? 1 : 0);
            HIPCHK(c, hipGetLastError());
            const int rc = rgb_device_stage(c, b0, n, b.chunk, 0, b.per, R, st);
            if (rc) return rc;
        }
    } else {
        const size_t lds = (size_t)b.Np * 8 + unpack_lds_bytes() + 32;
        hipLaunchKernelGGL(k_fd_unpack, dim3(b.B), dim3(FB), lds, st, fa);
        HIPCHK(c, hipGetLastError());
    }
    if (b.tables_only) return TAMCMC_OK;
    if (b.route == FdRoute::Windowed || b.hybrid()) {
        hipLaunchKernelGGL(k_fd_compare, dim3(b.B), dim3(FB), 0, st, fa);
        HIPCHK(c, hipGetLastError());
    }
    if (b.route == FdRoute::Adjoint && !b.hybrid()) {
        fa.Bs = table_ptrs(db + b.o_btab, StageLayout(b.C, b.stride, 0));
        hipLaunchKernelGGL(k_adj_base, dim3(b.C), dim3(64), 0, st, fa);
        HIPCHK(c, hipGetLastError());
    }
    return TAMCMC_OK;
}

// Evaluate n tables -- every route's first likelihood launch.  The multiplets are fa.T's; ranges, counts and noise rows come from `ix`:
// fa.T (n = B, by slot) or fa.Bs (n = C, by chain).  keep: what stays in w.model -- nothing, the n model rows, or the three planes 1/M0,
// y/M0, M0 of the n points.  sums: the tile partials are folded into w.S[0, n).  `a` is left as launched (Windowed goes on from it).
enum class Keep { Nothing, Rows, Planes };
int evaluate_tables(tamcmc_hip_ctx *c, const FdArgs &fa, const TablePtrs &ix, int n, Keep keep, bool sums,
                    const FdBatch::Buffers &w, LoglikeArgs &a) {
    hipStream_t st = c->stream;
    a.B = n;
    a.mults = fa.T.mults; a.offsets = ix.pairs; a.noise = ix.noise; a.nharvey = ix.nh; a.nnoise = ix.nn;
    a.partials = w.part.p;
    if (keep != Keep::Nothing) a.model = w.model.p;
    if (keep == Keep::Planes) { a.fd_rows = w.model.p; a.fd_plane = (size_t)n * a.Nx; }  // (the planes instead of the rows)
    if (c->precision == TAMCMC_PRECISION_FAST) {
        HIPCHK(c, launch_bg_poly(a, c->wgs, c->K, w.bg.p, st));
        a.bg_poly = w.bg.p;
    }
    HIPCHK(c, launch_loglike(a, c->precision, c->wgs, c->K, keep != Keep::Nothing, st));
    if (sums) HIPCHK(c, launch_finalize(w.part.p, n, a.ntiles, w.S.p, st));
    return TAMCMC_OK;
}

}  // namespace

int FdBatch::enqueue(tamcmc_hip_ctx *c, unsigned char *db, const double *d_params, const Buffers &w, hipEvent_t ev0, hipEvent_t ev1,
                     hipEvent_t *split) {
    hipStream_t st = c->stream;
    const bool windowed = route == Route::Windowed || hybrid();  // (delta tables, the base launch's arrays by chain)
    if (!hybrid()) split = nullptr;
    double *const part = w.part.p, *const S = w.S.p, *const model = w.model.p, *const bgbuf = w.bg.p;
    FdArgs fa;
    fa.desc.model_id = model_id; fa.desc.prior_class = prior_class; fa.desc.Np = (int)Np; fa.desc.per = per;
    fa.desc.stride = stride; fa.desc.Nx = (int)c->Nx;
    fa.desc.x_first = c->hx[0]; fa.desc.x_last = c->hx[(size_t)c->Nx - 1]; fa.desc.step = c->hx[1] - c->hx[0];
    fa.desc.plength = (const int *)(db + head.o_pl); fa.desc.priors_switch = (const int *)(db + head.o_sw);
    fa.desc.priors = (const double *)(db + head.o_pr); fa.desc.extra = (const double *)(db + head.o_ex); fa.desc.poly = c->d_poly.p;
    const StageLayout L(table_slots(), stride, (size_t)table_slots() * per);
    fa.T = table_ptrs(db + o_tab, L);
    fa.C = C; fa.E = E; fa.Nv = Nvars;
    fa.params = d_params ? d_params : (const double *)(db + head.o_params);
    fa.idx = (const int *)(db + head.o_idx); fa.h = (const double *)(db + head.o_h);
    fa.logPr_plus = (double *)(db + head.o_lpp); fa.logPr_minus = (double *)(db + head.o_lpm); fa.status = (int *)(db + head.o_st);
    fa.windowed = windowed ? 1 : 0;
    fa.base_copies = rgb ? 0 : 1;
    fa.hybrid = hybrid() ? 1 : 0;
    fa.full_tables = (windowed && c->precision == TAMCMC_PRECISION_FAST && bgbuf) ? 1 : 0;
    fa.D = fa.T; fa.Bs = fa.T;
    fa.d_range = nullptr; fa.d_flags = nullptr; fa.d_row = nullptr; fa.d_noise_old = nullptr;
    if (windowed) {
        fa.D = table_ptrs(db + o_dtab, StageLayout(B, stride, (size_t)B * 2 * per));
        fa.Bs = table_ptrs(db + o_btab, StageLayout(C, stride, 0));
        fa.d_range = (int *)(db + o_drange); fa.d_flags = (int *)(db + o_dflags); fa.d_row = (int *)(db + o_drow);
        fa.d_noise_old = (double *)(db + o_dnold);
    }
    if (rgb && c->precision == TAMCMC_PRECISION_STRICT && !h_prep) return TAMCMC_ERR_BAD_ARG;  // (fd_batch.h: STRICT needs the host unpack)
    if (split) HIPCHK(c, hipEventRecord(split[0], st));
    if (int rc = build_tables(c, *this, db, L, fa)) return rc;
    if (tables_only) return TAMCMC_OK;
    if (split) HIPCHK(c, hipEventRecord(split[1], st));

    const int Nx = (int)c->Nx;
    LoglikeArgs a;
    a.x = c->dx.p; a.y = c->dy.p; a.logx = c->dlogx.p; a.Nx = Nx; a.ntiles = ntiles;
    a.x0 = c->hx[0]; a.step = c->hx[1] - c->hx[0];
    a.noise_stride = stride; a.model = nullptr;
    if (ev0) HIPCHK(c, hipEventRecord(ev0, st));
    d_done = nullptr;
    // After the base launch (`a` as evaluate_tables left it): moments of the base points per tile, behind the three planes (the delta
    // launch's far-only tiles take their sums from them), then the B log-likelihood DIFFERENCES from the delta tables, folded into dS
    auto delta_launches = [&](double *dS) -> int {
        double *mom = (c->precision == TAMCMC_PRECISION_FAST && c->wgs == 64) ? model + 3 * (size_t)C * Nx : nullptr;
        double *momT = mom ? mom + (size_t)C * ntiles * FD_MOM : nullptr;
        if (mom) HIPCHK(c, launch_fd_moments(a, c->wgs, c->K, mom, momT, st));
        LoglikeArgs d = a;
        d.fd_mom = mom;
        d.fd_momT = momT;
        d.B = B; d.model = nullptr; d.fd_rows = nullptr;
        d.bg_poly = fa.full_tables ? bgbuf : nullptr;  // (rows by base point: read by the "full table" evaluations only)
        d.mults = fa.D.mults; d.offsets = fa.D.pairs; d.noise = fa.D.noise; d.nharvey = fa.D.nh; d.nnoise = fa.D.nn;
        d.partials = part + (size_t)C * ntiles * 2;
        d.d_range = fa.d_range; d.d_flags = fa.d_flags; d.d_row = fa.d_row; d.d_noise_old = fa.d_noise_old; d.model0 = model;
        if (mom) {  // the far-only tiles of the light evaluations, one lane per tile; the delta launch skips what this marks done
            unsigned char *done = (unsigned char *)(momT + (size_t)C * ntiles * FD_MOM);
            HIPCHK(c, launch_fd_far(d, c->wgs, c->K, done, st));
            d.d_done = done;
        }
        d_done = d.d_done;
        tile_bins_ = tile_bins(c->wgs, c->K);
        HIPCHK(c, launch_loglike_delta(d, c->precision, c->wgs, c->K, st));
        HIPCHK(c, launch_finalize(d.partials, B, ntiles, dS, st));
        return TAMCMC_OK;
    };
    switch (route) {
    case Route::Brute:
        if (int rc = evaluate_tables(c, fa, fa.T, B, Keep::Nothing, true, w, a)) return rc;
        break;
    case Route::Rows:  // frozen windows, then the B model rows (no sums are read: the partials are the launch's scratch)
        if (rgb) {  // (per chain and variable, both sides seen together: fisher_rgb_rule.h)
            FisherRgbArgs r;
            r.mults = fa.T.mults; r.pairs = fa.T.pairs; r.nh = fa.T.nh; r.nn = fa.T.nn; r.noise = fa.T.noise; r.status = fa.status;
            r.per = per; r.stride = stride; r.C = C; r.N = Nvars / 2;
            r.rh3 = (const double *)(db + o_frh3); r.rh = (double *)(db + o_frh);
            r.counts = count_forms ? (unsigned long long *)(db + o_fcount) : nullptr;
            HIPCHK(c, launch_fisher_freeze_rgb(r, st));
        } else
            HIPCHK(c, launch_fisher_freeze(fa.T.mults, fa.T.pairs, fa.status, per, C, E, st));
        if (int rc = evaluate_tables(c, fa, fa.T, B, Keep::Rows, false, w, a)) return rc;
        break;
    case Route::Adjoint: {
        // (1) the C base points, exactly the windowed route's base launch
        if (int rc = evaluate_tables(c, fa, fa.Bs, C, Keep::Planes, true, w, a)) return rc;
        if (split) HIPCHK(c, hipEventRecord(split[2], st));
        // (1b) hybrid: the windowed route's launches on the delta tables -- empty but for the fallback slots -- into the scratch sums.
        // The moments are taken for every chain: which chains have a fallback slot is known on the device only, and the device engine
        // enqueues its batches without a synchronisation
        double *const fall = hybrid() ? S + C + B : nullptr;
        if (hybrid()) {
            if (int rc = delta_launches(fall)) return rc;
        }
        if (split) HIPCHK(c, hipEventRecord(split[3], st));
        // (2) dS/d(table entry) of each base point, (3) contracted with every perturbed table's difference from it
        AdjArgs g;
        g.x = c->dx.p; g.logx = c->dlogx.p; g.Nx = Nx;
        g.planes = model; g.plane = (size_t)C * Nx;
        g.C = C; g.E = E; g.per = per; g.stride = stride;
        g.mults = fa.T.mults; g.pairs = fa.T.pairs; g.nh = fa.T.nh; g.nn = fa.T.nn; g.status = fa.status; g.noise = fa.T.noise;
        g.G = (double *)(db + o_adjG); g.Gn = (double *)(db + o_adjGn); g.npart = (double *)(db + o_adjpart); g.ntn = adj_ntn;
        g.Gpart = (double *)(db + o_adjGpart); g.nseg = adj_nseg;
        if (hybrid()) {
            g.cls = fa.d_flags; g.fall = fall;
            g.counts = count_slots ? (unsigned long long *)(db + o_adjcount) : nullptr;
        }
        HIPCHK(c, launch_adjoint(g, st, split ? split + 4 : nullptr));
        HIPCHK(c, launch_adjoint_contract(g, S + C, st));
        if (split) HIPCHK(c, hipEventRecord(split[6], st));
        break;
    }
    case Route::Windowed:
        // (1) the C base points: full evaluation, planes kept; (2) the C*Nvars perturbed points from the delta tables
        if (int rc = evaluate_tables(c, fa, fa.Bs, C, Keep::Planes, true, w, a)) return rc;
        if (int rc = delta_launches(S + C)) return rc;
        break;
    }
    if (ev1) HIPCHK(c, hipEventRecord(ev1, st));
    return TAMCMC_OK;
}

hipError_t FdBatch::hybrid_stats(tamcmc_hip_ctx *c, unsigned char *db, long *linearised, long *fallback) const {
    unsigned long long v[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(v, db + o_adjcount, sizeof v, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(db + o_adjcount, 0, sizeof v, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    *linearised = (long)v[0];
    *fallback = (long)v[1];
    return e;
}

hipError_t FdBatch::delta_stats(const unsigned char *db, long *bins, long *full) const {
    std::vector<int> v((size_t)2 * B);
    std::vector<unsigned char> done(d_done ? (size_t)B * ntiles : 0);
    hipError_t e = hipMemcpy(v.data(), db + o_drange, v.size() * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess && d_done) e = hipMemcpy(done.data(), d_done, done.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    *bins = 0;
    for (int s = 0; s < B; s++) *bins += v[2 * (size_t)s + 1] - v[2 * (size_t)s];
    for (unsigned char t : done) *bins -= t ? (long)tile_bins_ : 0;  // (far-only tiles taken from the base point's moments: no bin of them was read)
    if (!full) return hipSuccess;
    e = hipMemcpy(v.data(), db + o_dflags, (size_t)B * sizeof(int), hipMemcpyDeviceToHost);
    *full = 0;
    for (int s = 0; s < B && e == hipSuccess; s++) *full += (v[(size_t)s] & 2) ? 1 : 0;
    return e;
}

int check_gradient_args(const tamcmc_hip_ctx *c, int C, const double *params, int64_t Nparams, const int32_t *plength,
                        const int32_t *index_to_relax, int Nvars, const double *hstep, bool rest_ok, unsigned rules) {
    const bool need_pl = rules & GA_PLENGTH, vars = rules & GA_VARS, fisher = rules & GA_FISHER;
    if (c->Nx <= 0) return TAMCMC_ERR_NO_SPECTRUM;
    if (C < 0 || !params || Nparams < 1 || !rest_ok || (need_pl && !plength)) return TAMCMC_ERR_BAD_ARG;
    if (vars && (Nvars < (fisher ? 1 : 0) || (fisher && Nvars > 16384) || !index_to_relax || !hstep)) return TAMCMC_ERR_BAD_ARG;
    if (C == 0 && (rules & GA_EMPTY_FIRST)) return TAMCMC_OK;
    long psum = 0;
    for (int i = 0; need_pl && i < 11; i++) psum += plength[i];
    if (need_pl && psum != Nparams) return TAMCMC_ERR_BAD_ARG;
    for (int k = 0; vars && k < Nvars; k++)
        if (index_to_relax[k] < 0 || index_to_relax[k] >= Nparams || (fisher && !(hstep[k] != 0.0))) return TAMCMC_ERR_BAD_ARG;
    return TAMCMC_OK;
}

}  // namespace tamcmc

// STRICT keeps the reference's arithmetic for a red giant's scalar unpack too: long double on the host, exactly what
// tamcmc_hip_loglike_params_batch does with the same vector -- a vector's STRICT logL is the same bits from either entry.  Fills the
// context's pinned h_rgb / h_stage for the B vectors and points the batch at them.
static int rgb_host_unpack(tamcmc_hip_ctx *c, FdBatch &fb, const FdInputs &in) {
    const double *params = in.params, *hstep = in.hstep;
    const int32_t *plength = in.plength, *index_to_relax = in.index_to_relax;
    const int E = fb.E, B = fb.B;
    const size_t Np = (size_t)fb.Np;
    const size_t bytes_prep = ((size_t)B * sizeof(rgb::Prep) + 15) & ~(size_t)15;
    const StageLayout L(B, fb.stride, (size_t)B * fb.per);
    HIPCHK(c, c->h_rgb.reserve(bytes_prep + (size_t)B * sizeof(rgb::RowIn)));
    HIPCHK(c, c->h_stage.reserve(L.off_mults));
    rgb::Prep *hp = (rgb::Prep *)c->h_rgb.p;
    rgb::RowIn *hr = (rgb::RowIn *)(c->h_rgb.p + bytes_prep);
    unsigned char *hh = c->h_stage.p;
    std::memset(hh, 0, L.off_mults);
    int32_t *h_nh = (int32_t *)(hh + L.off_nh), *h_nn = (int32_t *)(hh + L.off_nn);
    double *h_noise = (double *)(hh + L.off_noise);
    const bool cte = fb.model_id == TAMCMC_MODEL_RGB_ASYMPT_AJ_CTEWIDTH_V4_ID;
    const double ustep = c->hx[2] - c->hx[1];
    int nthr = B / 4 > 0 ? (B / 4 < 8 ? B / 4 : 8) : 1;
    (void)nthr;  // (only the host pass sees the OpenMP pragma)
#pragma omp parallel for schedule(static) num_threads(nthr)
    for (int s = 0; s < B; s++) {
        const int ch = s / E, e = s - ch * E;
        std::vector<double> v(params + (size_t)ch * Np, params + (size_t)(ch + 1) * Np);
        if (e > 0) {
            volatile double xp = v[(size_t)index_to_relax[e - 1]] + hstep[e - 1];
            v[(size_t)index_to_relax[e - 1]] = xp;
        }
        double fmin;
        rgb::unpack_vector(rgb::OneThread(), v.data(), plength, ustep, cte, c->armm_dense ? 1 : 0, hp[s], hr[s], h_noise + (size_t)s * fb.stride, h_nh + s,
                           h_nn + s, &fmin);
    }
    fb.h_prep = hp; fb.h_rows = hr; fb.h_header = hh;
    return TAMCMC_OK;
}

int tamcmc::FdBatch::begin(tamcmc_hip_ctx *c, const FdInputs &in, unsigned char **block) {
    HIPCHK(c, c->h_fd.reserve(head.in_bytes + head.out_bytes));
    HIPCHK(c, c->d_fd.reserve(total_bytes));
    head.stage(c->h_fd.p, in);
    HIPCHK(c, hipMemcpyAsync(c->d_fd.p, c->h_fd.p, head.in_bytes, hipMemcpyHostToDevice, c->stream));
    if (rgb && c->precision == TAMCMC_PRECISION_STRICT)
        if (int rc = rgb_host_unpack(c, *this, in)) return rc;
    if (!tables_only) HIPCHK(c, reserve(c, context_buffers(c)));
    *block = c->d_fd.p;
    return TAMCMC_OK;
}

int tamcmc::FdBatch::finish(tamcmc_hip_ctx *c, FdResults *out) {
    HIPCHK(c, hipMemcpyAsync(c->h_fd.p + head.in_bytes, c->d_fd.p + head.in_bytes, head.out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = head.results(c->h_fd.p);
    return TAMCMC_OK;
}

// What a host entry passes on to the block: the prior's arrays only where there is a prior (no kernel reads them otherwise)
static FdInputs host_inputs(int prior_class, const double *params, const int32_t *plength, const int32_t *index_to_relax, const double *hstep,
                            const double *priors, const int32_t *priors_switch, const double *extra_priors) {
    FdInputs in;
    in.params = params; in.plength = plength; in.index_to_relax = index_to_relax; in.hstep = hstep;
    if (prior_class != 0) { in.priors = priors; in.priors_switch = priors_switch; in.extra_priors = extra_priors; }
    return in;
}

static int fd_run(tamcmc_hip_ctx *c, int model_id, int prior_class, int C, const double *params, int64_t Nparams,
                  const int32_t *plength, const int32_t *index_to_relax, int Nvars, const double *hstep, const double *Tcoefs,
                  double p, const double *priors, const int32_t *priors_switch, const double *extra_priors, double *logL0,
                  double *logPr0, double *grad, double *grad_prior) {
    if (!c) return TAMCMC_ERR_BAD_ARG;
    int rc = check_gradient_args(c, C, params, Nparams, plength, index_to_relax, Nvars, hstep,
                                 logL0 && grad && (prior_class == 0 || (priors && priors_switch && extra_priors)), GA_PLENGTH | GA_VARS | GA_EMPTY_FIRST);
    if (rc || C == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    FdBatch fb;
    if ((rc = fb.layout(c, FdBatch::Request::FromOptions, model_id, prior_class, C, Nparams, plength, Nvars))) return rc;
    if ((rc = ensure_poly(c))) return rc;
    const size_t nS = fb.ws.S;
    unsigned char *db;
    if ((rc = fb.begin(c, host_inputs(prior_class, params, plength, index_to_relax, hstep, priors, priors_switch, extra_priors), &db))) return rc;
    HIPCHK(c, c->h_S.reserve(nS));
    hipEvent_t *split = nullptr;
    if (c->timing && fb.hybrid()) {  // slot counters and the stage split of the hybrid batch (tamcmc_hip_get_rgb_adjoint_stats / _times)
        for (hipEvent_t &e : c->ev_split)
            if (!e) HIPCHK(c, hipEventCreate(&e));
        split = c->ev_split;
        fb.count_slots = true;
        HIPCHK(c, fb.zero_slot_counts(c, db));
    }
    if ((rc = fb.enqueue(c, db, c->timing ? c->ev0 : nullptr, c->timing ? c->ev1 : nullptr, split))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_S.p, c->d_S.p, nS * 8, hipMemcpyDeviceToHost, st));
    FdResults res;
    if ((rc = fb.finish(c, &res))) return rc;
    if ((rc = account_kernel_time(c, fb.B))) return rc;
    if (c->timing) {
        if (fb.route == FdBatch::Route::Windowed) {  // what the delta launch really touched (roofline bookkeeping of bench.py)
            long bins = 0, full = 0;
            HIPCHK(c, fb.delta_stats(db, &bins, &full));
            c->fd_bins += bins;
            c->fd_delta_evals += fb.B;
            c->fd_full_evals += full;
        }
        if (split) {
            static const int from[6] = {0, 1, 3, 4, 2, 5};  // tables, base launch, row pass, noise pass + fold, fallback delta, contraction
            for (int i = 0; i < 6; i++) {
                float ms = 0;
                HIPCHK(c, hipEventElapsedTime(&ms, split[from[i]], split[from[i] + 1]));
                c->rgb_adj_ms[i] = ms;
            }
            long lin = 0, fall = 0;
            HIPCHK(c, fb.hybrid_stats(c, db, &lin, &fall));
            c->rgb_adj_lin += lin;
            c->rgb_adj_fallback += fall;
        }
    }
    return assemble_gradient(C, Nvars, params, Nparams, index_to_relax, hstep, Tcoefs, p,
                             fb.deltas() ? LikelihoodShare::Differences : LikelihoodShare::FullSums, c->h_S.p, nullptr,
                             prior_class != 0 ? res.lpp : nullptr, res.lpm, res.status, logL0, logPr0, grad, grad_prior);
}

extern "C" {

int tamcmc_hip_fd_gradient(tamcmc_hip_ctx *c, int model_id, int C, const double *params, int64_t Nparams,
                           const int32_t *plength, const int32_t *index_to_relax, int Nvars, const double *hstep,
                           const double *Tcoefs, double p, double *logL0, double *grad) {
    if (tamcmc::is_envelope_model(model_id))  // every parameter moves every bin: no table, no window (envelope.hip)
        return tamcmc::envelope_gradient(c, model_id, false, 0, C, params, Nparams, index_to_relax, Nvars, hstep, Tcoefs, p, nullptr, nullptr,
                                         logL0, nullptr, grad, nullptr);
    return fd_run(c, model_id, 0, C, params, Nparams, plength, index_to_relax, Nvars, hstep, Tcoefs, p, nullptr, nullptr, nullptr,
                  logL0, nullptr, grad, nullptr);
}

int tamcmc_hip_fd_gradient_posterior(tamcmc_hip_ctx *c, int model_id, int prior_class, int C, const double *params,
                                     int64_t Nparams, const int32_t *plength, const int32_t *index_to_relax, int Nvars,
                                     const double *hstep, const double *Tcoefs, double p, const double *priors,
                                     const int32_t *priors_switch, const double *extra_priors, double *logL0, double *logPr0,
                                     double *grad, double *grad_prior) {
    if (tamcmc::is_envelope_model(model_id))  // priors of classes 0 / 1 on the device (envelope.hip)
        return tamcmc::envelope_gradient(c, model_id, true, prior_class, C, params, Nparams, index_to_relax, Nvars, hstep, Tcoefs, p, priors,
                                         priors_switch, logL0, logPr0, grad, grad_prior);
    if (is_rgb_model(model_id) ? prior_class != 4 : (prior_class != 2 && prior_class != 3)) return TAMCMC_ERR_BAD_MODEL;  // io_asymptotic is the red giants' prior, and theirs only
    return fd_run(c, model_id, prior_class, C, params, Nparams, plength, index_to_relax, Nvars, hstep, Tcoefs, p, priors,
                  priors_switch, extra_priors, logL0, logPr0, grad, grad_prior);
}

// Audit entry of the envelope fits' analytic gradient (TAMCMC_OPT_ENVELOPE_GRADIENT): the row-space sums before the chain rule
int tamcmc_hip_envelope_gradient_sums(tamcmc_hip_ctx *c, int model_id, int C, const double *params, int64_t Nparams, double *S, double *sums,
                                      double *ksi) {
    if (!c) return TAMCMC_ERR_BAD_ARG;
    if (!tamcmc::is_envelope_model(model_id)) return TAMCMC_ERR_BAD_MODEL;
    if (c->Nx <= 0) return TAMCMC_ERR_NO_SPECTRUM;
    if (C < 0 || !params || !S || !sums) return TAMCMC_ERR_BAD_ARG;
    if (C == 0) return TAMCMC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return tamcmc::envelope_gradient_sums(c, model_id, C, params, Nparams, S, sums, ksi);
}

// Audit entry of the adjoint route: the batch with no perturbed vector (Nvars = 0) on Route::Adjoint, whatever the context's
// option says -- unpack, base launch, k_adj_rows, k_adj_noise -- and G / Gn brought back.  Red giants (with TAMCMC_OPT_RGB_ADJOINT): the
// hybrid batch with no perturbed slot, the row pass over its work list.
int tamcmc_hip_adjoint_table(tamcmc_hip_ctx *c, int model_id, int C, const double *params, int64_t Nparams, const int32_t *plength,
                             const double *Tcoefs, double p, double *G, double *Gn, int *nrows) {
    (void)Tcoefs; (void)p;  // (the adjoint of the un-tempered sum S: logL = -p S / T)
    if (!c) return TAMCMC_ERR_BAD_ARG;
    if (tamcmc::is_envelope_model(model_id)) return TAMCMC_ERR_BAD_MODEL;
    int rc = check_gradient_args(c, C, params, Nparams, plength, nullptr, 0, nullptr, true, GA_PLENGTH);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    FdBatch fb;
    if ((rc = fb.layout(c, FdBatch::Request::Adjoint, model_id, 0, C > 0 ? C : 1, Nparams, plength, 0))) return rc;
    if (nrows) *nrows = fb.per;
    if (C == 0) return TAMCMC_OK;
    if ((rc = ensure_poly(c))) return rc;
    unsigned char *db;
    if ((rc = fb.begin(c, host_inputs(0, params, plength, nullptr, nullptr, nullptr, nullptr, nullptr), &db))) return rc;
    if ((rc = fb.enqueue(c, db))) return rc;
    if (G) HIPCHK(c, hipMemcpyAsync(G, db + fb.o_adjG, (size_t)C * fb.per * ADJ_F * 8, hipMemcpyDeviceToHost, st));
    if (Gn) HIPCHK(c, hipMemcpyAsync(Gn, db + fb.o_adjGn, (size_t)C * fb.stride * 8, hipMemcpyDeviceToHost, st));
    FdResults res;
    if ((rc = fb.finish(c, &res))) return rc;
    return res.first_status();  // (a failed chain's G and Gn are zero)
}

// The audit entries' common body: the tables of the B = C (Nvars + 1) vectors as the batch's own builder leaves them and nothing after them
// (red giants: k_fd_rgb_perturb -> rgb_device_stage; STRICT: the host's long-double unpack uploaded, as fd_run does.  Others: k_fd_unpack).
static int batch_tables(tamcmc_hip_ctx *c, int model_id, int prior_class, int C, const double *params, int64_t Nparams, const int32_t *plength,
                        const int32_t *index_to_relax, int Nvars, const double *hstep, const double *priors, const int32_t *priors_switch,
                        const double *extra_priors, tamcmc_multiplet *rows, int32_t *nrows, double *noise, int32_t *nharvey,
                        int32_t *nnoise, int32_t *status, int *per) {
    int rc = check_gradient_args(c, C, params, Nparams, plength, index_to_relax, Nvars, hstep,
                                 prior_class == 0 || (priors && priors_switch && extra_priors), GA_PLENGTH | GA_VARS);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    FdBatch fb;
    if ((rc = fb.layout(c, FdBatch::Request::Tables, model_id, prior_class, C > 0 ? C : 1, Nparams, plength, Nvars))) return rc;
    if (per) *per = fb.per;
    if (C == 0) return TAMCMC_OK;
    if ((rc = ensure_poly(c))) return rc;
    const size_t B = (size_t)fb.B;
    unsigned char *db;
    if ((rc = fb.begin(c, host_inputs(prior_class, params, plength, index_to_relax, hstep, priors, priors_switch, extra_priors), &db))) return rc;
    if ((rc = fb.enqueue(c, db))) return rc;
    const StageLayout L((int)B, fb.stride, B * fb.per);
    const unsigned char *tb = db + fb.o_tab;
    std::vector<int32_t> pairs(2 * B);
    HIPCHK(c, hipMemcpyAsync(pairs.data(), tb + L.off_pairs, 2 * B * 4, hipMemcpyDeviceToHost, st));
    if (rows) HIPCHK(c, hipMemcpyAsync(rows, tb + L.off_mults, B * fb.per * sizeof(tamcmc_multiplet), hipMemcpyDeviceToHost, st));
    if (noise) HIPCHK(c, hipMemcpyAsync(noise, tb + L.off_noise, B * fb.stride * 8, hipMemcpyDeviceToHost, st));
    if (nharvey) HIPCHK(c, hipMemcpyAsync(nharvey, tb + L.off_nh, B * 4, hipMemcpyDeviceToHost, st));
    if (nnoise) HIPCHK(c, hipMemcpyAsync(nnoise, tb + L.off_nn, B * 4, hipMemcpyDeviceToHost, st));
    FdResults res;
    if ((rc = fb.finish(c, &res))) return rc;
    for (size_t s = 0; s < B; s++) {
        if (nrows) nrows[s] = pairs[2 * s + 1] - pairs[2 * s];
        if (status) status[s] = res.status[s];
    }
    return res.first_status();
}

int tamcmc_hip_rgb_batch_tables(tamcmc_hip_ctx *c, int model_id, int C, const double *params, int64_t Nparams, const int32_t *plength,
                                const int32_t *index_to_relax, int Nvars, const double *hstep, tamcmc_multiplet *rows, int32_t *nrows,
                                double *noise, int32_t *nharvey, int32_t *nnoise, int32_t *status, int *per) {
    if (!c) return TAMCMC_ERR_BAD_ARG;
    if (!is_rgb_model(model_id)) return TAMCMC_ERR_BAD_MODEL;
    return batch_tables(c, model_id, 0, C, params, Nparams, plength, index_to_relax, Nvars, hstep, nullptr, nullptr, nullptr, rows, nrows, noise,
                        nharvey, nnoise, status, per);
}

// Audit entry of the main-sequence batches: the tables k_fd_unpack leaves in the slots [0, B) (the Tables request takes Brute's layout: no
// base copies behind them), with the log-prior in front of the unpack (prior_class 2, 3) or without it (0).
int tamcmc_hip_fd_batch_tables(tamcmc_hip_ctx *c, int model_id, int prior_class, int C, const double *params, int64_t Nparams,
                               const int32_t *plength, const int32_t *index_to_relax, int Nvars, const double *hstep, const double *priors,
                               const int32_t *priors_switch, const double *extra_priors, tamcmc_multiplet *rows, int32_t *nrows,
                               double *noise, int32_t *nharvey, int32_t *nnoise, int32_t *status, int *per) {
    if (!c) return TAMCMC_ERR_BAD_ARG;
    if (is_rgb_model(model_id) || tamcmc::is_envelope_model(model_id)) return TAMCMC_ERR_BAD_MODEL;
    if (prior_class != 0 && prior_class != 2 && prior_class != 3) return TAMCMC_ERR_BAD_MODEL;
    return batch_tables(c, model_id, prior_class, C, params, Nparams, plength, index_to_relax, Nvars, hstep, priors, priors_switch,
                        extra_priors, rows, nrows, noise, nharvey, nnoise, status, per);
}

}  // extern "C"
