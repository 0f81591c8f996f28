// dev_sampler.hip -- device-resident MCMC iteration (sampler-side algebra on the device).
//
// The host-driven loop (host_mala.cpp) spends ~3/4 of a step on the host (proposal, priors, table build, copies, one sync per
// step).  Here the whole iteration of ALL tempered chains runs on the GPU; the host only enqueues launches and fetches the recorded
// samples once per run() call.  Two launch schemes, same chains bit for bit (same Philox streams, same arithmetic, same orders):
//
// (A) FUSED STEP (dev_step_impl.h), one launch per iteration and set of chains (k_step) -- used for every stretch of iterations WITHOUT
//     adaptation (the bulk of a run: the reference learns in [Nt_learn[0], Nt_learn[last]) only, config_default.cfg:17-18).  Launch i
//     holds 64-lane workgroups of four kinds, and NOTHING INSIDE A LAUNCH WAITS FOR ANYTHING ELSE INSIDE IT:
//       * likelihood tiles of iteration i (loglike_tile.h, the hot kernel's body).  Which table a chain's tiles read is the outcome of
//         iteration i-1's test, and EVERY WORKGROUP DECIDES THAT FOR ITSELF at its start from what launch i-1 left in memory
//         (quick_decide: the test as a threshold on the sum of the previous launch's partial sums; decide(), the test as written --
//         MALA.cpp:397-461,490-551 -- when the sum is within rounding of the threshold).  Same inputs, same code in every workgroup: the
//         same answer everywhere, no hand-off.  The tiles leave their two partial sums for launch i+1, and add their sum into their chain's
//         accumulators (FusedArgs::qacc), which is what quick_decide reads;
//       * commit workgroups, one wave per chain: the exact decide() of iteration i-1, then the chain's state of iteration i, the
//         sample/stat record of iteration i-1, move flags and counters, and for launch i+1 the slot, prior, status and threshold
//         record of the chain's proposal.  A launch of commit workgroups alone closes a stretch;
//       * branch-ahead candidates of iteration i+1, built WHILE the tiles run: the proposal of i+1 is x + L z(i+1) where x is one of
//         a few known vectors -- the chain's current position (test i rejects) or its proposal of i (accepts), and for the swap pair
//         also the partner's two -- so all 2C+4 candidates are prepared in advance, each by eight single-wave roles (position + first
//         half of the log-prior | table rows + noise row | second half of the log-prior | background series, a quarter of the tiles
//         each x4 | one spare);
//       * L z blocks two iterations ahead, one wave per chain.
//     From the size on at which one launch outgrows the GPU's resident waves the chains form TWO GROUPS, each with its own launch per
//     iteration on its own stream: the groups' launches fill each other's idle ends and share nothing, except in the iterations whose
//     swap pair straddles the groups -- for that iteration and the next the boundary between the groups moves by one chain, so that
//     the pair lies inside one launch, with one event hop each way and the rest of the second group running on through both; only a
//     pair on the moved boundary still makes an iteration one launch over all chains (step_schedule.h: StepPlanner, with every wait;
//     RunCall::run_fused enqueues its plan).
// (B) LOCKSTEP (dev_iterate_impl.h), two kernels per iteration and chain group (k_iterate, k_loglike) -- used where the proposal law is
//     adapted after every test (the next proposal needs the new Cholesky factor, so it cannot be prepared ahead):
//       k_iterate (one workgroup per chain) settles iteration it-1 (MH test, swap, record, Robbins-Monro update MALA.cpp:296-319,
//       Cholesky of (Sigma+eps2 I) sigma MALA.cpp:348-350) and proposes iteration it; k_loglike evaluates.
// (C) ENVELOPE STEP (dev_env_step_impl.h), the Gaussian-envelope models (ids 0 / 1, opt-in: TAMCMC_OPT_ENVELOPE_DEVICE_ENGINE).  They have no
//     table: k_iterate's proposal ends with the log-prior and the row of scalars the evaluation reads (env_front), and the lockstep
//     route evaluates it with envelope.hip's kernels on the group's stream (envelope_stage_enqueue) in place of k_loglike.  Stretches
//     without adaptation run as ONE launch per iteration (k_env_step: every tile of a chain settles, proposes and evaluates) for
//     spectra up to env_step_max_bins() bins (id 1: 32 768; id 0: 6 144, the measured crossover); the fused step (A) is not used.
//     Their Langevin step (opt-in of its own: TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN) is the Langevin engine below with the analytic gradient
//     as its batch (dev_mala_impl.h: k_env_mala_front, envelope_grad_stage_enqueue, k_env_mala_chain), lockstep only.
// All per-iteration state is double-buffered by parity: a workgroup reads parity P and writes parity P^1, so the swap needs no
// inter-workgroup synchronisation inside (B) and a launch never overwrites what it still reads in (A).  Both schemes keep the
// chains' state in the same arrays; a stretch hands over to the next with the parity only.
//
// This file: the entry points of DevSampler.  The engine's state is DevSampler::Impl (dev_sampler_state.h): the chains' state and
// constants, and one part per scheme -- chain groups, (A), (C), the Langevin step -- that owns its buffers, events and streams.  Here:
// init step by step, upload and download, and run(), which hands a call to the per-call object of dev_sampler_run.h,
// RunCall: the schedule of step_schedule.h over (A), (B) and (C), or the Langevin step (dev_mala_impl.h).
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/tamcmc_sampler.h"
#include "ctx.h"
#include "rgb_prestep.h"
#include "rgb_front.h"
#include "dev_sampler.h"
#include "kernels.h"
#include "loglike_tile.h"
#include "dev_unpack.h"
#include "envelope.h"
#include "fd_batch.h"
#include "mode_tables.h"
#include "rng.h"
#include "step_schedule.h"
#include "factor_update.h"

namespace tamcmc {

namespace {

#include "dev_iterate_impl.h"
#include "dev_env_step_impl.h"
#include "dev_step_impl.h"
#include "dev_mala_impl.h"

}  // namespace
// ---------------------------------------------------------------------------------------------------------------

#include "dev_sampler_state.h"
#include "dev_sampler_run.h"

DevSampler::DevSampler() : impl(new Impl()) {}
DevSampler::~DevSampler() {
    if (!impl) return;
    if (impl->ctx) {
        (void)hipSetDevice(impl->ctx->device);
        (void)hipStreamSynchronize(impl->ctx->stream);
        // after a HIP error in the middle of a call the other chain groups' streams may still hold launches that use the sampler's buffers
        for (int g = 1; g < 4; g++) if (impl->grp.gst[g]) (void)hipStreamSynchronize(impl->grp.gst[g]);
    }
#ifdef TAMCMC_PROBE
    impl->probe_report();
#endif
    delete impl;  // (the parts release what they own: dev_sampler_state.h)
}

#ifdef TAMCMC_PROBE
// the probe build's in-kernel stamps (TAMCMC_PROBE_STEP, TAMCMC_PROBE_ADAPT), read from the counters before they are freed
void DevSampler::Impl::probe_report() const {
    if (a.counters && getenv("TAMCMC_PROBE_STEP")) {
        long h[40];
        (void)hipMemcpy(h, a.counters + 8 + a.C, sizeof h, hipMemcpyDeviceToHost);
        if (h[35] > 0) fprintf(stderr, "build_multiplet, row 20 (us): decode + widths/heights %.2f | window %.2f | m loop %.2f\n", 0.01 * h[32] / h[35], 0.01 * h[33] / h[35], 0.01 * h[34] / h[35]);
        for (int r = 0; r < 4; r++)
            if (h[8 * r + 3] > 0)
                fprintf(stderr, "candidate role %d of slot 2 (us): decide %.2f | vectors + L z %.2f | role %.2f  [inside: %.2f | %.2f]  (%ld launches)\n", r,
                        0.01 * h[8 * r] / h[8 * r + 3], 0.01 * h[8 * r + 1] / h[8 * r + 3], 0.01 * h[8 * r + 2] / h[8 * r + 3],
                        0.01 * h[8 * r + 4] / h[8 * r + 3], 0.01 * h[8 * r + 5] / h[8 * r + 3], h[8 * r + 3]);
    }
    if (a.counters && getenv("TAMCMC_PROBE_ADAPT")) {
        long h[8];
        (void)hipMemcpy(h, a.counters, sizeof h, hipMemcpyDeviceToHost);
        if (h[7] > 0)
            fprintf(stderr, "Cholesky panels of chain 0 (us per panel): columns below %.2f | next panel's columns %.2f | next diagonal block beside the rest of the trailing update %.2f  (%ld panels)\n",
                    0.01 * h[4] / h[7], 0.01 * h[5] / h[7], 0.01 * h[6] / h[7], h[7]);
    }
}
#endif

// ---- init, step by step.  The order of the steps is the order of their work on the context stream.

// the model's flags and table dimensions; what the host keeps of the inputs; refusals that need no device
int DevSampler::Impl::validate(const DevSamplerInit &in) {
    tamcmc_hip_ctx *c = ctx;
    a.desc.model_id = in.model_id; a.desc.prior_class = in.prior_class; a.C = in.C; a.desc.Np = in.Np; a.Nv = in.Nv;
    rgb = is_rgb_model(in.model_id);
    env.on = is_envelope_model(in.model_id);
    if (env.on) {
        // opt-in, one option per step (read at creation: tamcmc_sampler_create has refused already, before building anything):
        // TAMCMC_OPT_ENVELOPE_DEVICE_ENGINE admits the random walk, TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN the Langevin step; neither implies the other
        if (!(in.use_drift ? c->envelope_device_langevin : c->envelope_device_engine)) return TAMCMC_ERR_BAD_MODEL;
        if (in.prior_class != in.model_id) return TAMCMC_ERR_BAD_MODEL;  // priors_ctrl.list pairs class 0 with id 0, class 1 with id 1
        if (in.Np < envelope_nparams(in.model_id) || c->Nx > 0x7fffffff / 2) return TAMCMC_ERR_BAD_ARG;
    }
#ifdef TAMCMC_PROBE
    if (const char *ep = getenv("TAMCMC_PROBE_ADAPT")) a.probe = atoi(ep);
#endif
    a.desc.per = (rgb || env.on) ? 0 : mt::count_multiplets(in.model_id, in.plength);  // (ids 0 / 1: no table)
    h_plength.assign(in.plength, in.plength + 11);
    prior_class = in.prior_class; model_id = in.model_id;
    factor_refresh = in.factor_refresh;
    lan.use_drift = in.use_drift != 0; lan.delta = in.delta; lan.fd_step_rel = in.fd_step_rel > 0 ? in.fd_step_rel : 1e-7;
    lan.h_priors.assign(in.priors, in.priors + 4 * (size_t)in.Np); lan.h_extra.assign(in.extra_priors, in.extra_priors + 10);
    lan.h_idx.assign(in.index_to_relax, in.index_to_relax + in.Nv); lan.h_sw.assign(in.priors_switch, in.priors_switch + in.Np);
    if (a.desc.per < 0) return TAMCMC_ERR_BAD_MODEL;
    a.desc.stride = in.plength[8] > 0 ? in.plength[8] : 1;
    if ((a.desc.stride - 1) / 3 > TAMCMC_MAX_HARVEY) return TAMCMC_ERR_BAD_ARG;
    return TAMCMC_OK;
}

void DevSampler::Impl::Groups::choose(const DevSamplerInit &in, bool rgb) {
    G = in.chain_groups > 0 ? in.chain_groups : (in.C >= 8 ? 2 : 1);
    // red giants: an iteration is a chain of four latency-bound launches per group (proposal + unpack, solver, rows, likelihood);
    // four groups keep the GPU busy while three of them are in their short kernels (C5, 40 chains: 3.4 / 3.8 / 4.0 / 4.05 k
    // iterations/s with 1 / 2 / 3 / 4 groups)
    if (in.chain_groups <= 0 && rgb && in.C >= 16) G = 4;
    if (G > 4) G = 4;
    if (G > in.C) G = in.C;
}

// Red giants: the pre-step workspace, which also gives the table dimensions (per, stride) the arrays are sized with.
// Langevin step: opt-in (TAMCMC_OPT_RGB_DEVICE_LANGEVIN, read here and nowhere else).  Its proposals are unpacked by the
// gradient batch (FdBatch::enqueue on a.params_prop: k_fd_rgb_perturb -> rgb_device_stage), which sizes the pre-step workspace
// for its own chunk at every call (FdBatch::layout); k_mala_test and k_mala_settle see the batch's sums, priors and statuses only.
// Such a sampler never runs k_iterate or the lockstep pre-step: no workspace slices per chain group, one slice of C vectors here
int DevSampler::Impl::rgb_workspace(const DevSamplerInit &in) {
    if (!rgb) return TAMCMC_OK;
    if (lan.use_drift && !ctx->rgb_device_langevin) return TAMCMC_ERR_BAD_MODEL;
    if (lan.use_drift && ((long)in.C * (in.Nv + 1) > 65535 || in.plength[10] < 6)) return TAMCMC_ERR_BAD_ARG;  // (FdBatch::layout's limits, at creation)
    const int slices = lan.use_drift ? 1 : grp.G;
    rgb_bmax = (in.C + slices - 1) / slices;
    return rgb_device_prepare(ctx, rgb_bmax, slices, in.plength, &a.desc.per, &a.desc.stride);  // random walk: one workspace slice per chain group
}

// the constants, the chains' arrays (zeroed where the kernels count), k_iterate's LDS plan, the polynomial tables
int DevSampler::Impl::create_chain_state(const DevSamplerInit &in) {
    tamcmc_hip_ctx *c = ctx;
    a.desc.Nx = (int)c->Nx;
    a.desc.x_first = c->hx[0]; a.desc.x_last = c->hx[(size_t)c->Nx - 1]; a.desc.step = c->hx[1] - c->hx[0];
    a.pl = (long)in.likelihood_params;
    a.seed = in.seed; a.dN_mixing = in.dN_mixing; a.swap_rule = in.swap_rule == 1 ? 1 : 0;
    a.c0 = in.c0; a.epsilon1 = in.epsilon1; a.epsi2 = in.epsi2; a.A1 = in.A1; a.target_acceptance = in.target_acceptance;
    const size_t C = (size_t)in.C, Np = (size_t)in.Np, Nv = (size_t)in.Nv;
    hipStream_t st = c->stream;
    int *d_pl, *d_idx, *d_sw;
    double *d_pr, *d_ex, *d_T;
    DCHK(mem.dalloc(&d_pl, 11)); DCHK(mem.dalloc(&d_idx, Nv)); DCHK(mem.dalloc(&d_sw, Np));
    DCHK(mem.dalloc(&d_pr, 4 * Np)); DCHK(mem.dalloc(&d_ex, 10)); DCHK(mem.dalloc(&d_T, C));
    DCHK(up(d_pl, in.plength, 11, st)); DCHK(up(d_idx, in.index_to_relax, Nv, st)); DCHK(up(d_sw, in.priors_switch, Np, st));
    DCHK(up(d_pr, in.priors, 4 * Np, st)); DCHK(up(d_ex, in.extra_priors, 10, st)); DCHK(up(d_T, in.Tcoefs, C, st));
    a.desc.plength = d_pl; a.index_to_relax = d_idx; a.desc.priors_switch = d_sw; a.desc.priors = d_pr; a.desc.extra = d_ex; a.Tcoefs = d_T;
    // every per-iteration array exists twice (parity): a workgroup reads parity P and writes parity P^1
    DCHK(mem.dalloc(&a.vars_cur, 2 * C * Nv)); DCHK(mem.dalloc(&a.params_cur, 2 * C * Np));
    DCHK(mem.dalloc(&a.vars_prop, 2 * C * Nv)); DCHK(mem.dalloc(&a.params_prop, 2 * C * Np));
    DCHK(mem.dalloc(&a.logL_cur, 2 * C)); DCHK(mem.dalloc(&a.logPr_cur, 2 * C)); DCHK(mem.dalloc(&a.logPost_cur, 2 * C));
    DCHK(mem.dalloc(&a.init_logL, C)); DCHK(mem.dalloc(&a.logPr_prop, 2 * C)); DCHK(mem.dalloc(&a.status_prop, 2 * C));
    DCHK(mem.dalloc(&a.Pmove, C)); DCHK(mem.dalloc(&a.moved, C)); DCHK(mem.dalloc(&a.counters, 8 + C + 64));  // (+64: timeline stamps of the probe build)
    DCHK(mem.dalloc(&a.lz, 2 * C * Nv)); DCHK(mem.dalloc(&a.LT, C * Nv * Nv)); DCHK(mem.dalloc(&a.cov, C * Nv * Nv)); DCHK(mem.dalloc(&a.mu, C * Nv)); DCHK(mem.dalloc(&a.sigma, C));
    DCHK(mem.dalloc(&a.mults, C * (size_t)a.desc.per + 1)); DCHK(mem.dalloc(&a.pairs, 2 * C)); DCHK(mem.dalloc(&a.nh, C)); DCHK(mem.dalloc(&a.nn, C));
    DCHK(mem.dalloc(&a.noise, C * (size_t)a.desc.stride));
    a.env_rows = nullptr;
    if (env.on) {
        DCHK(mem.dalloc(&a.env_rows, C));
        DCHK(hipMemsetAsync(a.env_rows, 0, C * sizeof(EnvRow), st));
    }
    DCHK(mem.dalloc(&a.fvalid, C)); DCHK(mem.dalloc(&a.fcount, 4));
    DCHK(hipMemsetAsync(a.fvalid, 0, C * sizeof(int), st));
    DCHK(hipMemsetAsync(a.fcount, 0, 4 * sizeof(long), st));
    DCHK(hipMemsetAsync(a.counters, 0, (8 + C + 64) * sizeof(long), st));
    DCHK(hipMemsetAsync(a.moved, 0, C * sizeof(int), st));
    DCHK(hipMemsetAsync(a.Pmove, 0, C * sizeof(double), st));
    a.samples = nullptr; a.stats = nullptr;
    // Cholesky workspace: LDS when (Nv^2 + Nv) doubles fit beside the iteration's own LDS, else global scratch
    lds_base = (Np + 2 * Nv + 1) * sizeof(double) + unpack_lds_bytes() + 32;
    lds_adapt = (Nv * Nv + Nv) * sizeof(double);
    a.chol_in_lds = (lds_base + lds_adapt <= 150 * 1024) ? 1 : 0;  // (k_iterate also has ~6 KB of static LDS)
    if (!a.chol_in_lds) { DCHK(mem.dalloc(&adapt_scratch, C * (Nv * Nv + 3 * Nv))); lds_adapt = 0; }
    if (lds_base + lds_adapt > 64 * 1024) {
        DCHK(hipFuncSetAttribute((const void *)k_iterate<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_base + lds_adapt)));
        DCHK(hipFuncSetAttribute((const void *)k_iterate<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_base + lds_adapt)));
    }
    // polynomial tables Pslm/Qlm: computed ON the device (its own double arithmetic), read through a uniform pointer
    mt::PolyTab *d_tab;
    DCHK(mem.dalloc(&d_tab, 1));
    DCHK(fill_poly_table(d_tab, st));
    a.desc.poly = d_tab;
    return TAMCMC_OK;
}

// Langevin step: the gradients by parity beside the chains' state, and the per-chain work arrays of k_mala_test
int DevSampler::Impl::Langevin::create(Impl &I, const DevSamplerInit &in) {
    tamcmc_hip_ctx *c = I.ctx;
    DevSamplerArgs &a = I.a;
    const size_t C = (size_t)in.C, Nv = (size_t)in.Nv;
    a.grad_cur = nullptr; a.gradP_cur = nullptr;
    if (!use_drift) return TAMCMC_OK;
    DCHK(I.mem.dalloc(&a.grad_cur, 2 * C * Nv)); DCHK(I.mem.dalloc(&a.gradP_cur, 2 * C * Nv));
    DCHK(I.mem.dalloc(&mala.grad_prop, C * Nv)); DCHK(I.mem.dalloc(&mala.gradP_prop, C * Nv)); DCHK(I.mem.dalloc(&mala.drift_cur, C * Nv));
    DCHK(I.mem.dalloc(&mala.out, C * 5));
    if (!I.env.on) return TAMCMC_OK;
    // ids 0 / 1: the analytic batch (dev_mala_impl.h) in place of the finite-difference one
    const size_t Np = (size_t)in.Np, E = Nv + 1, Nx = (size_t)a.desc.Nx, ntiles = (Nx + ETILE - 1) / ETILE, nchunk = (Nx + ECHUNK - 1) / ECHUNK;
    const bool kal = in.model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN;
    EnvMalaArgs &k = envb.k;
    EnvGradBuffers &g = envb.g;
    double *gsum, *ksum;
    DCHK(I.mem.dalloc(&k.pts, C * (2 * Nv + 1) * Np)); DCHK(I.mem.dalloc(&k.lpp, C * E)); DCHK(I.mem.dalloc(&k.lpm, C * E));
    DCHK(I.mem.dalloc(&envb.h, Nv)); DCHK(I.mem.dalloc(&k.dlogL, C * Nv));
    DCHK(I.mem.dalloc(&g.S, C)); DCHK(I.mem.dalloc(&gsum, C * ENV_GRAD_NRAWMAX)); DCHK(I.mem.dalloc(&ksum, C * ENV_GRAD_NKRAW));
    DCHK(I.mem.dalloc(&g.part, C * ntiles * 2)); DCHK(I.mem.dalloc(&g.gpart, C * ntiles * (size_t)env_grad_nraw(in.model_id)));
    if (kal) { DCHK(I.mem.dalloc(&g.ksi_part, C * nchunk * 3)); DCHK(I.mem.dalloc(&g.ksi_gpart, C * nchunk * (ENV_GRAD_NKRAW - 3))); }
    DCHK(hipMemsetAsync(ksum, 0, C * ENV_GRAD_NKRAW * sizeof(double), c->stream));  // (id 1 never writes them)
    g.gsum = gsum; g.ksum = ksum;
    k.h = envb.h; k.gsum = gsum; k.ksum = ksum; k.hx = c->hx[1] - c->hx[0];
    return TAMCMC_OK;
}

// the groups' streams (group 0: the context's) and the events of their hand-overs
int DevSampler::Impl::Groups::create(Impl &I) {
    tamcmc_hip_ctx *c = I.ctx;
    gst[0] = c->stream;
    for (int g = 1; g < G; g++) DCHK(hipStreamCreateWithFlags(&gst[g], hipStreamNonBlocking));
    DCHK(I.events.make(&fork, false));
    for (int g = 0; g < 4; g++) { DCHK(I.events.make(&kb[g], false)); DCHK(I.events.make(&ki[g], false)); DCHK(I.events.make(&join[g], false)); }
    return TAMCMC_OK;
}

// (A) fused step: three sets (iteration mod 3) of 2C+8 candidate slots, per-chain hand-over arrays by parity (tables are sized at the first run())
int DevSampler::Impl::FusedStep::create(Impl &I, const DevSamplerInit &in) {
    tamcmc_hip_ctx *c = I.ctx;
    const DevSamplerArgs &a = I.a;
    DevArena &mem = I.mem;
    hipStream_t st = c->stream;
    const size_t C = (size_t)in.C, Np = (size_t)in.Np, Nv = (size_t)in.Nv;
    f.NS = 2 * in.C + 8;
    {   // two chain groups for the fused step (see run()): with the default groups, from 8 chains on
        const int h = (int)(((long)in.C * 1) / 2);
        f.xsplit = (I.grp.G == 2 && h >= 3 && in.C - h >= 3) ? h : in.C;
    }
    const size_t NS = (size_t)f.NS;
    DCHK(mem.dalloc(&f.cand_vars, 3 * NS * Nv)); DCHK(mem.dalloc(&f.cand_params, 3 * NS * Np)); DCHK(mem.dalloc(&f.cand_logPr, 6 * NS));
    DCHK(mem.dalloc(&f.cand_stP, 6 * NS)); DCHK(mem.dalloc(&f.cand_stR, 3 * NS)); DCHK(mem.dalloc(&f.cand_rej, 3 * NS));
    DCHK(mem.dalloc(&f.mults, 3 * NS * (size_t)a.desc.per + 1)); DCHK(mem.dalloc(&f.pairs, 6 * NS)); DCHK(mem.dalloc(&f.nh, 3 * NS)); DCHK(mem.dalloc(&f.nn, 3 * NS));
    DCHK(mem.dalloc(&f.noise, 3 * NS * (size_t)a.desc.stride));
    DCHK(mem.dalloc(&f.slot, 2 * C)); DCHK(mem.dalloc(&f.prop_logPr, 2 * C)); DCHK(mem.dalloc(&f.prop_st, 2 * C)); DCHK(mem.dalloc(&f.quick, 2 * C * QN)); DCHK(mem.dalloc(&f.lz, 2 * C * Nv));
    DCHK(mem.dalloc(&f.qcount, 3));
    DCHK(hipMemsetAsync(f.qcount, 0, 3 * sizeof(unsigned long long), st));
    // the tiles' per-chain accumulators: one 128-byte line per (set, chain) on a 128-byte boundary, zero between stretches -- once
    // here, then by the commit workgroups (commit_chain); their size does not follow the tile geometry
    static_assert(2 * QK * sizeof(double) == 128, "one line per (set, chain)");
    DCHK(mem.dalloc(&f.qacc, 3 * C * 2 * QK));
    if (((uintptr_t)f.qacc & 127) != 0) return TAMCMC_ERR_HIP;
    DCHK(hipMemset(f.qacc, 0, 3 * C * 2 * QK * sizeof(double)));
    f.qmargin = 1e-11;
    DCHK(hipMemsetAsync(f.nn, 0, 3 * NS * sizeof(int), st));
    DCHK(hipMemsetAsync(f.cand_stP, 0, 6 * NS * sizeof(int), st));
    DCHK(hipMemsetAsync(f.cand_rej, 0, 3 * NS * sizeof(int), st));
    DCHK(hipMemsetAsync(f.cand_stR, 0, 3 * NS * sizeof(int), st));
    f.part = nullptr;
    f.bg = nullptr;
    // the candidate roles borrow the tile workgroup's LDS: a parameter vector too long for it keeps the lockstep scheme
    ok = !I.rgb && !I.env.on && I.lds_base <= sizeof(tile::TileLds<tile::M_FAST_DIRECT, 64>);
    return TAMCMC_OK;
}

int DevSampler::init(tamcmc_hip_ctx *c, const DevSamplerInit &in) {
    Impl &I = *impl;
    I.ctx = c;
    if (c->Nx <= 0) return TAMCMC_ERR_NO_SPECTRUM;
    if (in.C < 1 || in.C > TAMCMC_MAX_CHAINS) return TAMCMC_ERR_BAD_ARG;
    DCHK(hipSetDevice(c->device));
    if (int rc = I.validate(in)) return rc;
    I.grp.choose(in, I.rgb);
    if (int rc = I.rgb_workspace(in)) return rc;
    if (int rc = I.create_chain_state(in)) return rc;
    if (int rc = I.lan.create(I, in)) return rc;
    for (auto &pair : I.ev) { DCHK(I.events.make(&pair[0], true)); DCHK(I.events.make(&pair[1], true)); }
    for (auto &pair : I.fu.gev) { DCHK(I.events.make(&pair[0], true)); DCHK(I.events.make(&pair[1], true)); }
    if (int rc = I.grp.create(I)) return rc;
    if (int rc = I.fu.create(I, in)) return rc;
    DCHK(hipStreamSynchronize(c->stream));
    return TAMCMC_OK;
}

// One preamble of the entry points that read what the last call left on the device: the device set, the context stream idle
// (every entry point returns with the sampler's streams idle)
int DevSampler::Impl::ready_to_read() {
    tamcmc_hip_ctx *c = ctx;
    DCHK(hipSetDevice(c->device));
    DCHK(hipStreamSynchronize(c->stream));
    return TAMCMC_OK;
}

int DevSampler::download_gradient(double *grad, double *grad_prior) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    if (!I.lan.use_drift || !I.a.grad_cur || !I.lan.grad_valid) return TAMCMC_ERR_BAD_ARG;
    if (int rc = I.ready_to_read()) return rc;
    const size_t n = (size_t)I.a.C * I.a.Nv;
    if (grad) DCHK(hipMemcpy(grad, I.a.grad_cur + (size_t)I.parity * n, n * sizeof(double), hipMemcpyDeviceToHost));
    if (grad_prior) DCHK(hipMemcpy(grad_prior, I.a.gradP_cur + (size_t)I.parity * n, n * sizeof(double), hipMemcpyDeviceToHost));
    return TAMCMC_OK;
}

int DevSampler::download_last_proposal(double *vars_prop, double *grad_prop) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    if (!I.lan.use_drift) return TAMCMC_ERR_BAD_ARG;  // (the random-walk schemes keep several candidate proposals per chain, not one)
    if (int rc = I.ready_to_read()) return rc;
    const size_t n = (size_t)I.a.C * I.a.Nv;
    if (vars_prop) DCHK(hipMemcpy(vars_prop, I.a.vars_prop, n * sizeof(double), hipMemcpyDeviceToHost));
    if (grad_prop) DCHK(hipMemcpy(grad_prop, I.lan.mala.grad_prop, n * sizeof(double), hipMemcpyDeviceToHost));
    return TAMCMC_OK;
}

int DevSampler::download_tables(int32_t shape[4], tamcmc_multiplet *rows, int32_t *nrows, double *noise, int32_t *nharvey, int32_t *nnoise,
                                int32_t *status, int32_t *written, double *logPr, double *params) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    const DevSamplerArgs &a = I.a;
    const FusedArgs &f = I.fu.f;
    // (ids 25 / 27, random walk: lockstep scheme, the rows k_rgb_finish left in the same block; rows per slot = Nfl0 + Nfl2 + Nfl3 + 400)
    if (I.lan.use_drift || I.env.on || (!I.rgb && mt::count_multiplets(a.desc.model_id, I.h_plength.data()) < 0)) return TAMCMC_ERR_BAD_MODEL;
    const int scheme = I.last.scheme;
    const bool fused = scheme == 2;
    const size_t C = (size_t)a.C, NS = (size_t)f.NS, n = fused ? 3 * NS : C, per = (size_t)a.desc.per, stride = (size_t)a.desc.stride, Np = (size_t)a.desc.Np;
    if (shape) { shape[0] = scheme; shape[1] = scheme ? (int32_t)n : 0; shape[2] = (int32_t)per; shape[3] = (int32_t)stride; }
    if (!scheme) return TAMCMC_OK;  // (no stretch yet: nothing to read)
    if (int rc = I.ready_to_read()) return rc;
    const size_t Q = (size_t)I.last.prop_parity;
    std::vector<int32_t> pairs(2 * n), st(n), nn(n), rej(n, 0);
    std::vector<double> lp(fused ? 2 * n : n);
    auto get = [](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
    DCHK(get(pairs.data(), fused ? f.pairs : a.pairs, 2 * n * 4));
    DCHK(get(nn.data(), fused ? f.nn : a.nn, n * 4));
    DCHK(get(st.data(), fused ? f.cand_stR : a.status_prop + Q * C, n * 4));
    DCHK(get(lp.data(), fused ? f.cand_logPr : a.logPr_prop + Q * C, lp.size() * 8));
    if (fused) DCHK(get(rej.data(), f.cand_rej, n * 4));
    if (rows) DCHK(get(rows, fused ? f.mults : a.mults, n * per * sizeof(tamcmc_multiplet)));
    if (noise) DCHK(get(noise, fused ? f.noise : a.noise, n * stride * 8));
    if (nharvey) DCHK(get(nharvey, fused ? f.nh : a.nh, n * 4));
    if (params) DCHK(get(params, fused ? f.cand_params : a.params_prop + Q * C * Np, n * Np * 8));
    for (size_t s = 0; s < n; s++) {
        // (fused: a slot no launch has written yet still has the nn = 0 and the status 0 the engine gave it at creation)
        const bool w = !fused || nn[s] != 0 || st[s] != TAMCMC_OK;
        if (written) written[s] = w ? 1 : 0;
        if (nrows) nrows[s] = w ? pairs[2 * s + 1] - pairs[2 * s] : 0;
        if (nnoise) nnoise[s] = nn[s];
        if (status) status[s] = st[s];
        if (logPr) logPr[s] = fused ? (rej[s] ? -INFINITY : lp[2 * s] + lp[2 * s + 1]) : lp[s];
    }
    return TAMCMC_OK;
}

int DevSampler::download_envelope_rows(double *rows, double *params, double *logPr, int32_t *status) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    const DevSamplerArgs &a = I.a;
    if (!I.env.on) return TAMCMC_ERR_BAD_MODEL;
    if (!I.last.scheme) return TAMCMC_ERR_BAD_ARG;  // (no iteration yet: no proposal)
    if (int rc = I.ready_to_read()) return rc;
    const size_t C = (size_t)a.C, Np = (size_t)a.desc.Np, Q = (size_t)I.last.prop_parity;
    if (rows) {
        std::vector<EnvRow> h(C);
        DCHK(hipMemcpy(h.data(), a.env_rows, C * sizeof(EnvRow), hipMemcpyDeviceToHost));
        for (size_t m = 0; m < C; m++) env_row_as_doubles(h[m], rows + m * TAMCMC_ENVELOPE_ROW_N);
    }
    if (params) DCHK(hipMemcpy(params, a.params_prop + Q * C * Np, C * Np * 8, hipMemcpyDeviceToHost));
    if (logPr) DCHK(hipMemcpy(logPr, a.logPr_prop + Q * C, C * 8, hipMemcpyDeviceToHost));
    if (status) DCHK(hipMemcpy(status, a.status_prop + Q * C, C * 4, hipMemcpyDeviceToHost));
    return TAMCMC_OK;
}

int DevSampler::download_envelope_sums(double *S, double *tile_sums, double *xi_sums) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    if (!I.env.on || !I.lan.use_drift) return TAMCMC_ERR_BAD_MODEL;
    if (!I.last.scheme) return TAMCMC_ERR_BAD_ARG;  // (no iteration yet: no batch)
    if (int rc = I.ready_to_read()) return rc;
    const size_t C = (size_t)I.a.C;
    const EnvGradBuffers &g = I.lan.envb.g;
    if (S) DCHK(hipMemcpy(S, g.S, C * 8, hipMemcpyDeviceToHost));
    if (tile_sums) DCHK(hipMemcpy(tile_sums, g.gsum, C * ENV_GRAD_NRAWMAX * 8, hipMemcpyDeviceToHost));
    if (xi_sums) DCHK(hipMemcpy(xi_sums, g.ksum, C * ENV_GRAD_NKRAW * 8, hipMemcpyDeviceToHost));
    return TAMCMC_OK;
}

void DevSampler::info(long out[18]) const {
    const Impl &I = *impl;
    unsigned long long qc[3] = {0, 0, 0};  // (every entry point returns with the sampler's streams idle)
    long fc[4] = {0, 0, 0, 0};
    if (I.fu.f.qcount && hipSetDevice(I.ctx->device) == hipSuccess) (void)hipMemcpy(qc, I.fu.f.qcount, sizeof qc, hipMemcpyDeviceToHost);
    if (I.a.fcount && hipSetDevice(I.ctx->device) == hipSuccess) (void)hipMemcpy(fc, I.a.fcount, sizeof fc, hipMemcpyDeviceToHost);
    out[14] = fc[0]; out[15] = fc[1]; out[16] = fc[2]; out[17] = fc[3];
    out[8] = I.n.n_stretch; out[9] = (long)qc[0]; out[10] = (long)qc[1]; out[13] = (long)qc[2];
    out[0] = I.a.Nv; out[1] = I.a.desc.Np;
    out[2] = I.lan.use_drift ? I.lan.chol_lds : I.a.chol_in_lds;
    out[3] = I.lan.use_drift ? 0 : I.env.on ? (I.a.desc.Nx <= env_step_max_bins(I.model_id) ? 1 : 0) : I.fu.ok ? 1 : 0;  // (ids 0 / 1: k_env_step)
    out[4] = I.grp.G; out[5] = I.n.it_fused; out[6] = I.n.it_lockstep; out[7] = I.a.C;
    out[11] = I.n.it_joint; out[12] = I.n.it_window;
}

// launch-order hint of k_loglike from chain 0's table at the uploaded position (ids 0 / 1: no table, the hint stays 0)
void DevSampler::Impl::set_tile_rot(const double *params) {
    tamcmc_hip_ctx *c = ctx;
    const int tb = tile_bins(c->wgs, c->K), ntiles = (int)((c->Nx + tb - 1) / tb);
    tile_rot = 0;
    if (env.on) return;
    if (rgb) {  // a little below the lowest radial mode (rgb_stage_params' rule)
        const double *fl0 = params + h_plength[0] + h_plength[1];
        const double fmin = *std::min_element(fl0, fl0 + h_plength[2]);
        const double t = (fmin - a.desc.x_first) / a.desc.step / (double)tb - 3.0;
        tile_rot = (t > 0 && t < ntiles) ? (int)t : 0;
        return;
    }
    std::vector<tamcmc_multiplet> tab((size_t)a.desc.per > 0 ? (size_t)a.desc.per : 1);
    std::vector<double> nz((size_t)a.desc.stride);
    int n = 0, nh = 0, nn = 0;
    if (build_mode_table(a.desc.model_id, params, h_plength.data(), c->hx.data(), c->Nx, tab.data(), a.desc.per, &n, nz.data(), &nh, &nn) == TAMCMC_OK && n <= a.desc.per)
        tile_rot = pick_tile_rot(tab.data(), n, a.desc.x_first, a.desc.step, tb, ntiles);
}

int DevSampler::upload_state(const double *vars, const double *params, const double *logL, const double *logPr,
                             const double *logPost, const double *init_logL) {
    Impl &I = *impl;
    I.fu.disarm();
    I.lan.grad_valid = false;
    tamcmc_hip_ctx *c = I.ctx;
    DevSamplerArgs &a = I.a;
    const size_t C = (size_t)a.C, Np = (size_t)a.desc.Np, Nv = (size_t)a.Nv;
    hipStream_t st = c->stream;
    DCHK(hipSetDevice(c->device));
    const size_t P = (size_t)I.parity;
    DCHK(up(a.vars_cur + P * C * Nv, vars, C * Nv, st)); DCHK(up(a.params_cur + P * C * Np, params, C * Np, st));
    DCHK(up(a.logL_cur + P * C, logL, C, st)); DCHK(up(a.logPr_cur + P * C, logPr, C, st)); DCHK(up(a.logPost_cur + P * C, logPost, C, st));
    DCHK(up(a.init_logL, init_logL, C, st));
    DCHK(hipStreamSynchronize(st));
    I.set_tile_rot(params);
    return TAMCMC_OK;
}

int DevSampler::upload_proposal(int m, const double *L_rowmajor, const double *cov, const double *mu, double sigma) {
    Impl &I = *impl;
    I.fu.disarm();
    tamcmc_hip_ctx *c = I.ctx;
    DevSamplerArgs &a = I.a;
    const size_t Nv = (size_t)a.Nv;
    std::vector<double> LT(Nv * Nv);
    for (size_t i = 0; i < Nv; i++)
        for (size_t k = 0; k < Nv; k++) LT[k * Nv + i] = (k <= i) ? L_rowmajor[i * Nv + k] : 0.0;
    hipStream_t st = c->stream;
    DCHK(hipSetDevice(c->device));
    DCHK(up(a.LT + (size_t)m * Nv * Nv, LT.data(), Nv * Nv, st));
    DCHK(up(a.cov + (size_t)m * Nv * Nv, cov, Nv * Nv, st));
    DCHK(up(a.mu + (size_t)m * Nv, mu, Nv, st));
    DCHK(up(a.sigma + m, &sigma, 1, st));
    DCHK(hipMemsetAsync(a.fvalid + m, 0, sizeof(int), st));  // a law from outside: the next adapting iteration is a full step
    DCHK(hipStreamSynchronize(st));
    return TAMCMC_OK;
}

int DevSampler::download_factor(int m, double *L_rowmajor) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    if (int rc = I.ready_to_read()) return rc;
    const size_t Nv = (size_t)I.a.Nv;
    std::vector<double> LT(Nv * Nv);
    DCHK(hipMemcpy(LT.data(), I.a.LT + (size_t)m * Nv * Nv, Nv * Nv * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < Nv; i++)
        for (size_t k = 0; k < Nv; k++) L_rowmajor[i * Nv + k] = (k <= i) ? LT[k * Nv + i] : 0.0;
    return TAMCMC_OK;
}

// gathers the chains' current state into one contiguous block: [vars C Nv | params C Np | logL C | logPr C | logPost C | Pmove C |
// moved C (as double) | counters 4 (as double: exact below 2^53) | per-chain move counts C]
__global__ void __launch_bounds__(256) k_pack_state(const DevSamplerArgs a, const int P, double *out) {
    const size_t C = (size_t)a.C, Np = (size_t)a.desc.Np, Nv = (size_t)a.Nv;
    const size_t n_v = C * Nv, n_p = C * Np, total = n_v + n_p + 6 * C + 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        double v;
        if (i < n_v) v = a.vars_cur[(size_t)P * n_v + i];
        else if (i < n_v + n_p) v = a.params_cur[(size_t)P * n_p + (i - n_v)];
        else {
            const size_t r = i - n_v - n_p, k = r / C, m = r - k * C;
            if (k == 0) v = a.logL_cur[(size_t)P * C + m];
            else if (k == 1) v = a.logPr_cur[(size_t)P * C + m];
            else if (k == 2) v = a.logPost_cur[(size_t)P * C + m];
            else if (k == 3) v = a.Pmove[m];
            else if (k == 4) v = (double)a.moved[m];
            else if (r < 5 * C + 4) v = (double)a.counters[r - 5 * C];
            else v = (double)a.counters[8 + (r - 5 * C - 4)];
        }
        out[i] = v;
    }
}
// One small kernel + ONE copy into pinned memory (eight copies into pageable memory cost ~150 us per tamcmc_sampler_run call).
int DevSampler::download_state(double *vars, double *params, double *logL, double *logPr, double *logPost, double *Pmove,
                               int *moved, long *counters, long *moves_per_chain) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    DevSamplerArgs &a = I.a;
    const size_t C = (size_t)a.C, Np = (size_t)a.desc.Np, Nv = (size_t)a.Nv;
    hipStream_t st = c->stream;
    DCHK(hipSetDevice(c->device));
    const size_t n_v = C * Nv, n_p = C * Np, total = n_v + n_p + 6 * C + 4;
    if (!I.pack.d) {
        DCHK(I.mem.dalloc(&I.pack.d, total));
        DCHK(hipHostMalloc((void **)&I.pack.h, total * sizeof(double), hipHostMallocDefault));
    }
    hipLaunchKernelGGL(k_pack_state, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, I.parity, I.pack.d);
    DCHK(hipMemcpyAsync(I.pack.h, I.pack.d, total * sizeof(double), hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    const double *h = I.pack.h;
    if (vars) std::memcpy(vars, h, n_v * 8);
    if (params) std::memcpy(params, h + n_v, n_p * 8);
    const double *sc = h + n_v + n_p;
    if (logL) std::memcpy(logL, sc, C * 8);
    if (logPr) std::memcpy(logPr, sc + C, C * 8);
    if (logPost) std::memcpy(logPost, sc + 2 * C, C * 8);
    if (Pmove) std::memcpy(Pmove, sc + 3 * C, C * 8);
    if (moved) for (size_t m = 0; m < C; m++) moved[m] = (int)sc[4 * C + m];
    if (counters) for (int k = 0; k < 4; k++) counters[k] = (long)sc[5 * C + (size_t)k];
    if (moves_per_chain) for (size_t m = 0; m < C; m++) moves_per_chain[m] = (long)sc[5 * C + 4 + m];
    return TAMCMC_OK;
}

int DevSampler::download_proposal(int m, double *cov, double *mu, double *sigma) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    DevSamplerArgs &a = I.a;
    const size_t Nv = (size_t)a.Nv;
    hipStream_t st = c->stream;
    DCHK(hipSetDevice(c->device));
    if (cov) DCHK(hipMemcpyAsync(cov, a.cov + (size_t)m * Nv * Nv, Nv * Nv * 8, hipMemcpyDeviceToHost, st));
    if (mu) DCHK(hipMemcpyAsync(mu, a.mu + (size_t)m * Nv, Nv * 8, hipMemcpyDeviceToHost, st));
    if (sigma) DCHK(hipMemcpyAsync(sigma, a.sigma + m, 8, hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    return TAMCMC_OK;
}

// n_iter iterations starting at iteration counter `it0`; learn[i] != 0 -> adaptation after iteration it0+i.
// Random walk: stretches without adaptation run as fused steps (A) -- ids 0 / 1: (C) --, the others in lockstep (B); see the head of
// this file.  Langevin step: RunCall::run_mala.
int DevSampler::run(long it0, long n_iter, const char *learn, double *samples, double *stats) {
    RunningCall running_call;
    CallTimeline tl;
    tl.mark();
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    if (n_iter <= 0) return TAMCMC_OK;
    DCHK(hipSetDevice(c->device));
    Impl::RunCall r(I, tl, it0, n_iter, learn, samples, stats);
    if (I.lan.use_drift) return r.run_mala();
    if (int rc = r.prepare()) return rc;
    tl.mark();  // (set-up of the call done: buffers, argument blocks)
    for (long i = 0, end = 0; i < n_iter; i = end) {
        bool is_fused;
        next_stretch(learn, n_iter, i, r.use_fused || r.env_step, &end, &is_fused);
        if (int rc = !is_fused ? r.run_lockstep(i, end) : r.env_step ? r.run_env_step(i, end) : r.run_fused(i, end)) return rc;
    }
    return r.finish();
}

}  // namespace tamcmc
