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
// All per-iteration state is double-buffered by parity: a workgroup reads parity P and writes parity P^1, so the swap needs no
// inter-workgroup synchronisation inside (B) and a launch never overwrites what it still reads in (A).  Both schemes keep the
// chains' state in the same arrays; a stretch hands over to the next with the parity only.
//
// This file: the engine's state (Impl), init, upload and download, and the two host drivers -- run() (RunCall: the schedule of
// step_schedule.h over the two schemes) and run_mala() (the Langevin step, dev_mala_impl.h).
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

namespace tamcmc {

namespace {

#include "dev_iterate_impl.h"
#include "dev_env_step_impl.h"
#include "dev_step_impl.h"
#include "dev_mala_impl.h"

}  // namespace

// ---------------------------------------------------------------------------------------------------------------

struct DevSampler::Impl {
    tamcmc_hip_ctx *ctx = nullptr;
    DevSamplerArgs a{};
    std::vector<void *> allocs;
    hipEvent_t ev[64][2];
    int n_ev = 0;
    bool poly_ready = false;
    double *adapt_scratch = nullptr;
    size_t smp_cap = 0, stat_cap = 0;
    size_t lds_base = 0, lds_adapt = 0;
    int parity = 0;  // which of the two state buffers holds the chains' current state
    FusedArgs f{};       // (A): candidate sets, per-chain slots and threshold records, partial sums, L z (dev_step_impl.h)
    unsigned char *d_argcopy = nullptr;  // device image of {DevSamplerArgs, FusedArgs} as last launched, and its host shadow
    std::vector<unsigned char> h_argcopy;
    // Langevin step (use_drift): the finite-difference batch object, its device block and scratch, the per-chain work arrays
    bool use_drift = false;
    double delta = 0, fd_step_rel = 1e-7;
    FdBatch fd;
    DevBuf<unsigned char> fd_block;
    DevBuf<double> fd_part, fd_S, fd_model, fd_bg;
    DevBuf<double> env_part;  // (C): the tiles' partial sums by launch parity
    bool env = false;         // ids 0 / 1: no table; rows (a.env_rows), envelope.hip's kernels or k_env_step
    DevBuf<double> fused_bg, fused_part;  // (A): the candidates' background series, the tiles' partial sums by parity (see run())
    MalaArgs mala{};
    bool grad_valid = false;
    int prior_class = 0, model_id = 0;
    std::vector<double> h_priors, h_extra;
    std::vector<int32_t> h_idx, h_sw;
    // (A) carried over between run() calls: the last launch of a fused stretch also prepares the candidates of the iteration that
    // follows and the L z of the one after; a call that continues right there starts without the two entry launches
    long armed_it = -1;
    int armed_q = 0;
    long it_fused = 0, it_lockstep = 0;  // iterations run by each scheme since creation (tamcmc_sampler_get_info)
    long n_stretch = 0;                  // fused stretches since creation (the first launch of each has nothing to decide)
    long it_joint = 0, it_window = 0;    // of it_fused with two chain groups: iterations run as one launch / as a window (StepPlanner)
    int mala_chol_lds = -1;
    int last_scheme = 0, last_prop_parity = 0;  // the last stretch run() enqueued: 1 lockstep (and the parity of its last proposals), 2 fused (download_tables)

    hipEvent_t gev[8][2];  // fused step with two chain groups: event pairs around sampled launches of the second group (on its stream)
    int n_gev = 0;
    bool rgb = false;  // ids 25 / 27: k_iterate leaves the table to the pre-step kernels (rgb_device_stage), lockstep scheme; Langevin step: the gradient batch builds the tables
    int rgb_bmax = 0;  // chains per workspace slice (one slice per chain group; Langevin step: unused after init)
    bool fused_ok = false;
    int fused_mode = -1, fused_K = 0;  // the geometry the (A) buffers were sized for
    int tile_rot = 0;  // launch-order hint of k_loglike (first near-field tile of chain 0's initial table)
    std::vector<int32_t> h_plength;
    // chain groups: the chains are split into G contiguous groups, each on its own stream, so that one group's k_iterate
    // overlaps the other groups' k_loglike (an iteration is a serial k_iterate -> k_loglike chain per group)
    int G = 1;
    hipStream_t gst[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_kb[4], ev_ki[4], ev_fork, ev_join[4];
    bool ev_made = false;
    double *d_pack = nullptr, *h_pack = nullptr;  // state download: device gather block and its pinned host image

    // The caller's record buffer as the device sees it when it is pinned, mapped host memory (tamcmc_hip_host_alloc): the settle step then
    // writes the records straight into it (15 KB per iteration over PCIe, posted) and a call ends without its two device-to-host copies.
    // (asked on every call: an address says nothing about what the caller has freed and allocated since the last one)
    double *device_view(const double *host, size_t bytes) {
        if (!host || !bytes) return nullptr;
        double *d = nullptr;
        void *dp = nullptr, *dq = nullptr;
        const char *last = (const char *)host + bytes - 1;
        // hipHostGetDevicePointer fails for pageable memory and returns the device address of THIS address for page-locked, mapped memory.
        // The whole record block [host, host + bytes) must lie inside ONE mapping: the last byte has to be page-locked too and map to the
        // first byte's device address + bytes - 1 -- a pinned buffer shorter than the call's records, or an interior pointer near the
        // end of one, would otherwise make the settle step write outside the mapping (a GPU fault instead of a host-side error)
        if (hipHostGetDevicePointer(&dp, const_cast<double *>(host), 0) == hipSuccess && dp &&
            hipHostGetDevicePointer(&dq, const_cast<char *>(last), 0) == hipSuccess && dq == (char *)dp + bytes - 1)
            d = (double *)dp;
        else (void)hipGetLastError();  // (pageable memory, or not one mapping over the whole block: the staged copy is used)
        return d;
    }

    // End of a call: the host waits for a stream by polling it for up to a millisecond before it blocks.  A blocking wait parks the
    // thread on an interrupt and wakes tens of microseconds after the last kernel has finished -- a tenth of a 20-iteration call (the
    // reference writes its ring buffer every Nbuffer iterations; a caller with short buffers makes short calls).
    // (only when this is the process's one running call: several host threads polling -- co-resident stars, tamcmc_sampler_run_packed --
    // would contend for the runtime's locks with the threads that are still enqueuing)
    static hipError_t wait_stream(hipStream_t st, bool poll) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int spin = 0; poll; spin++) {
            const hipError_t e = hipStreamQuery(st);
            if (e != hipErrorNotReady) return e;
            if ((spin & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(1000)) break;
        }
        (void)hipGetLastError();  // (hipErrorNotReady is sticky in the last-error slot)
        return hipStreamSynchronize(st);
    }

    template <typename T>
    hipError_t dalloc(T **p, size_t n) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, (n ? n : 1) * sizeof(T));
        if (e == hipSuccess) { allocs.push_back(q); *p = (T *)q; }
        return e;
    }

    struct KernelTiming;
    struct RunCall;  // one run() call
};

DevSampler::DevSampler() : impl(new Impl()) {}
DevSampler::~DevSampler() {
    if (!impl) return;
    if (impl->ctx) {
        (void)hipSetDevice(impl->ctx->device);
        (void)hipStreamSynchronize(impl->ctx->stream);
        // after a HIP error in the middle of a call the other chain groups' streams may still hold launches that use the buffers below
        for (int g = 1; g < 4; g++) if (impl->gst[g]) (void)hipStreamSynchronize(impl->gst[g]);
    }
#ifdef TAMCMC_PROBE
    if (impl->a.counters && getenv("TAMCMC_PROBE_STEP")) {
        long h[40];
        (void)hipMemcpy(h, impl->a.counters + 8 + impl->a.C, sizeof h, hipMemcpyDeviceToHost);
        if (h[35] > 0) fprintf(stderr, "build_multiplet, row 20 (us): decode + widths/heights %.2f | window %.2f | m loop %.2f\n", 0.01 * h[32] / h[35], 0.01 * h[33] / h[35], 0.01 * h[34] / h[35]);
        for (int r = 0; r < 4; r++)
            if (h[8 * r + 3] > 0)
                fprintf(stderr, "candidate role %d of slot 2 (us): decide %.2f | vectors + L z %.2f | role %.2f  [inside: %.2f | %.2f]  (%ld launches)\n", r,
                        0.01 * h[8 * r] / h[8 * r + 3], 0.01 * h[8 * r + 1] / h[8 * r + 3], 0.01 * h[8 * r + 2] / h[8 * r + 3],
                        0.01 * h[8 * r + 4] / h[8 * r + 3], 0.01 * h[8 * r + 5] / h[8 * r + 3], h[8 * r + 3]);
    }
    if (impl->a.counters && getenv("TAMCMC_PROBE_ADAPT")) {
        long h[8];
        (void)hipMemcpy(h, impl->a.counters, sizeof h, hipMemcpyDeviceToHost);
        if (h[7] > 0)
            fprintf(stderr, "Cholesky panels of chain 0 (us per panel): columns below %.2f | next panel's columns %.2f | next diagonal block beside the rest of the trailing update %.2f  (%ld panels)\n",
                    0.01 * h[4] / h[7], 0.01 * h[5] / h[7], 0.01 * h[6] / h[7], h[7]);
    }
#endif
    for (void *p : impl->allocs) (void)hipFree(p);
    impl->fd_block.release(); impl->fd_part.release(); impl->fd_S.release(); impl->fd_model.release(); impl->fd_bg.release(); impl->fused_bg.release(); impl->fused_part.release(); impl->env_part.release();
    if (impl->h_pack) (void)hipHostFree(impl->h_pack);
    for (int i = 0; i < impl->n_ev; i++) { (void)hipEventDestroy(impl->ev[i][0]); (void)hipEventDestroy(impl->ev[i][1]); }
    for (int i = 0; i < impl->n_gev; i++) { (void)hipEventDestroy(impl->gev[i][0]); (void)hipEventDestroy(impl->gev[i][1]); }
    if (impl->ev_made) {
        (void)hipEventDestroy(impl->ev_fork);
        for (int g = 0; g < 4; g++) { (void)hipEventDestroy(impl->ev_kb[g]); (void)hipEventDestroy(impl->ev_ki[g]); (void)hipEventDestroy(impl->ev_join[g]); }
        for (int g = 1; g < 4; g++) if (impl->gst[g]) (void)hipStreamDestroy(impl->gst[g]);
    }
    delete impl;
}

#define DCHK(call)                                                                   \
    do {                                                                             \
        hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                      \
            c->err = std::string(#call) + ": " + hipGetErrorString(e_);              \
            return TAMCMC_ERR_HIP;                                                   \
        }                                                                            \
    } while (0)

template <typename T>
static hipError_t up(T *dst, const T *src, size_t n, hipStream_t st) {
    return hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, st);
}

int DevSampler::init(tamcmc_hip_ctx *c, const DevSamplerInit &in) {
    Impl &I = *impl;
    I.ctx = c;
    if (c->Nx <= 0) return TAMCMC_ERR_NO_SPECTRUM;
    if (in.C < 1 || in.C > TAMCMC_MAX_CHAINS) return TAMCMC_ERR_BAD_ARG;
    DCHK(hipSetDevice(c->device));
    DevSamplerArgs &a = I.a;
    a.desc.model_id = in.model_id; a.desc.prior_class = in.prior_class; a.C = in.C; a.desc.Np = in.Np; a.Nv = in.Nv;
    I.rgb = is_rgb_model(in.model_id);
    I.env = is_envelope_model(in.model_id);
    if (I.env) {
        // opt-in (TAMCMC_OPT_ENVELOPE_DEVICE_ENGINE at creation: tamcmc_sampler_create has refused already, before building anything); the
        // Langevin step of these ids stays on the host engine
        if (!c->envelope_device_engine || in.use_drift) return TAMCMC_ERR_BAD_MODEL;
        if (in.prior_class != in.model_id) return TAMCMC_ERR_BAD_MODEL;  // priors_ctrl.list pairs class 0 with id 0, class 1 with id 1
        if (in.Np < envelope_nparams(in.model_id) || c->Nx > 0x7fffffff / 2) return TAMCMC_ERR_BAD_ARG;
    }
#ifdef TAMCMC_PROBE
    if (const char *ep = getenv("TAMCMC_PROBE_ADAPT")) a.probe = atoi(ep);
#endif
    a.desc.per = (I.rgb || I.env) ? 0 : mt::count_multiplets(in.model_id, in.plength);  // (ids 0 / 1: no table)
    I.h_plength.assign(in.plength, in.plength + 11);
    I.use_drift = in.use_drift != 0; I.delta = in.delta; I.fd_step_rel = in.fd_step_rel > 0 ? in.fd_step_rel : 1e-7;
    I.prior_class = in.prior_class; I.model_id = in.model_id;
    I.h_priors.assign(in.priors, in.priors + 4 * (size_t)in.Np); I.h_extra.assign(in.extra_priors, in.extra_priors + 10);
    I.h_idx.assign(in.index_to_relax, in.index_to_relax + in.Nv); I.h_sw.assign(in.priors_switch, in.priors_switch + in.Np);
    if (a.desc.per < 0) return TAMCMC_ERR_BAD_MODEL;
    a.desc.stride = in.plength[8] > 0 ? in.plength[8] : 1;
    if ((a.desc.stride - 1) / 3 > TAMCMC_MAX_HARVEY) return TAMCMC_ERR_BAD_ARG;
    {
        int G = in.chain_groups > 0 ? in.chain_groups : (in.C >= 8 ? 2 : 1);
        // red giants: an iteration is a chain of four latency-bound launches per group (proposal + unpack, solver, rows, likelihood);
        // four groups keep the GPU busy while three of them are in their short kernels (C5, 40 chains: 3.4 / 3.8 / 4.0 / 4.05 k
        // iterations/s with 1 / 2 / 3 / 4 groups)
        if (in.chain_groups <= 0 && I.rgb && in.C >= 16) G = 4;
        if (G > 4) G = 4;
        if (G > in.C) G = in.C;
        I.G = G;
    }
    if (I.rgb) {
        // Langevin step: opt-in (TAMCMC_OPT_RGB_DEVICE_LANGEVIN, read here and nowhere else).  Its proposals are unpacked by the
        // gradient batch (FdBatch::enqueue on a.params_prop: k_fd_rgb_perturb -> rgb_device_stage), which sizes the pre-step workspace
        // for its own chunk at every call (FdBatch::layout); k_mala_test and k_mala_settle see the batch's sums, priors and statuses only.
        // Such a sampler never runs k_iterate or the lockstep pre-step: no workspace slices per chain group, one slice of C vectors
        // here for the table dimensions (per, stride) the arrays below are sized with
        if (I.use_drift && !c->rgb_device_langevin) return TAMCMC_ERR_BAD_MODEL;
        if (I.use_drift && ((long)in.C * (in.Nv + 1) > 65535 || in.plength[10] < 6)) return TAMCMC_ERR_BAD_ARG;  // (FdBatch::layout's limits, at creation)
        const int slices = I.use_drift ? 1 : I.G;
        I.rgb_bmax = (in.C + slices - 1) / slices;
        int rc = rgb_device_prepare(c, I.rgb_bmax, slices, in.plength, &a.desc.per, &a.desc.stride);  // random walk: one workspace slice per chain group
        if (rc) return rc;
    }
    a.desc.Nx = (int)c->Nx;
    a.desc.x_first = c->hx[0]; a.desc.x_last = c->hx[(size_t)c->Nx - 1]; a.desc.step = c->hx[1] - c->hx[0];
    a.pl = (long)in.likelihood_params;
    a.seed = in.seed; a.dN_mixing = in.dN_mixing; a.swap_rule = in.swap_rule == 1 ? 1 : 0;
    a.c0 = in.c0; a.epsilon1 = in.epsilon1; a.epsi2 = in.epsi2; a.A1 = in.A1; a.target_acceptance = in.target_acceptance;
    const size_t C = (size_t)in.C, Np = (size_t)in.Np, Nv = (size_t)in.Nv;
    const size_t CD = C;
    hipStream_t st = c->stream;
    int *d_pl, *d_idx, *d_sw;
    double *d_pr, *d_ex, *d_T;
    DCHK(I.dalloc(&d_pl, 11)); DCHK(I.dalloc(&d_idx, Nv)); DCHK(I.dalloc(&d_sw, Np));
    DCHK(I.dalloc(&d_pr, 4 * Np)); DCHK(I.dalloc(&d_ex, 10)); DCHK(I.dalloc(&d_T, C));
    DCHK(up(d_pl, in.plength, 11, st)); DCHK(up(d_idx, in.index_to_relax, Nv, st)); DCHK(up(d_sw, in.priors_switch, Np, st));
    DCHK(up(d_pr, in.priors, 4 * Np, st)); DCHK(up(d_ex, in.extra_priors, 10, st)); DCHK(up(d_T, in.Tcoefs, C, st));
    a.desc.plength = d_pl; a.index_to_relax = d_idx; a.desc.priors_switch = d_sw; a.desc.priors = d_pr; a.desc.extra = d_ex; a.Tcoefs = d_T;
    // every per-iteration array exists twice (parity): a workgroup reads parity P and writes parity P^1
    DCHK(I.dalloc(&a.vars_cur, 2 * C * Nv)); DCHK(I.dalloc(&a.params_cur, 2 * C * Np));
    DCHK(I.dalloc(&a.vars_prop, 2 * CD * Nv)); DCHK(I.dalloc(&a.params_prop, 2 * CD * Np));
    DCHK(I.dalloc(&a.logL_cur, 2 * C)); DCHK(I.dalloc(&a.logPr_cur, 2 * C)); DCHK(I.dalloc(&a.logPost_cur, 2 * C));
    DCHK(I.dalloc(&a.init_logL, C)); DCHK(I.dalloc(&a.logPr_prop, 2 * CD)); DCHK(I.dalloc(&a.status_prop, 2 * CD));
    DCHK(I.dalloc(&a.Pmove, C)); DCHK(I.dalloc(&a.moved, C)); DCHK(I.dalloc(&a.counters, 8 + C + 64));  // (+64: timeline stamps of the probe build)
    a.grad_cur = nullptr; a.gradP_cur = nullptr;
    if (I.use_drift) {
        DCHK(I.dalloc(&a.grad_cur, 2 * C * Nv)); DCHK(I.dalloc(&a.gradP_cur, 2 * C * Nv));
        DCHK(I.dalloc(&I.mala.grad_prop, C * Nv)); DCHK(I.dalloc(&I.mala.gradP_prop, C * Nv)); DCHK(I.dalloc(&I.mala.drift_cur, C * Nv));
        DCHK(I.dalloc(&I.mala.out, C * 5));
    }
    DCHK(I.dalloc(&a.lz, 2 * C * Nv)); DCHK(I.dalloc(&a.LT, C * Nv * Nv)); DCHK(I.dalloc(&a.cov, C * Nv * Nv)); DCHK(I.dalloc(&a.mu, C * Nv)); DCHK(I.dalloc(&a.sigma, C));
    DCHK(I.dalloc(&a.mults, CD * (size_t)a.desc.per + 1)); DCHK(I.dalloc(&a.pairs, 2 * CD)); DCHK(I.dalloc(&a.nh, CD)); DCHK(I.dalloc(&a.nn, CD));
    DCHK(I.dalloc(&a.noise, CD * (size_t)a.desc.stride));
    a.env_rows = nullptr;
    if (I.env) {
        DCHK(I.dalloc(&a.env_rows, C));
        DCHK(hipMemsetAsync(a.env_rows, 0, C * sizeof(EnvRow), st));
    }
    DCHK(hipMemsetAsync(a.counters, 0, (8 + C + 64) * sizeof(long), st));
    DCHK(hipMemsetAsync(a.moved, 0, C * sizeof(int), st));
    DCHK(hipMemsetAsync(a.Pmove, 0, C * sizeof(double), st));
    a.samples = nullptr; a.stats = nullptr;
    // Cholesky workspace: LDS when (Nv^2 + Nv) doubles fit beside the iteration's own LDS, else global scratch
    I.lds_base = (Np + 2 * Nv + 1) * sizeof(double) + unpack_lds_bytes() + 32;
    I.lds_adapt = (Nv * Nv + Nv) * sizeof(double);
    a.chol_in_lds = (I.lds_base + I.lds_adapt <= 150 * 1024) ? 1 : 0;  // (k_iterate also has ~6 KB of static LDS)
    if (!a.chol_in_lds) { DCHK(I.dalloc(&I.adapt_scratch, C * (Nv * Nv + Nv))); I.lds_adapt = 0; }
    if (I.lds_base + I.lds_adapt > 64 * 1024) {
        DCHK(hipFuncSetAttribute((const void *)k_iterate<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(I.lds_base + I.lds_adapt)));
        DCHK(hipFuncSetAttribute((const void *)k_iterate<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(I.lds_base + I.lds_adapt)));
    }
    // polynomial tables Pslm/Qlm: computed ON the device (its own double arithmetic), read through a uniform pointer
    mt::PolyTab *d_tab;
    DCHK(I.dalloc(&d_tab, 1));
    DCHK(fill_poly_table(d_tab, st));
    a.desc.poly = d_tab;
    for (int i = 0; i < 64; i++) { DCHK(hipEventCreate(&I.ev[i][0])); DCHK(hipEventCreate(&I.ev[i][1])); I.n_ev = i + 1; }
    for (int i = 0; i < 8; i++) { DCHK(hipEventCreate(&I.gev[i][0])); DCHK(hipEventCreate(&I.gev[i][1])); I.n_gev = i + 1; }
    {
        const int G = I.G;
        I.gst[0] = st;
        for (int g = 1; g < G; g++) DCHK(hipStreamCreateWithFlags(&I.gst[g], hipStreamNonBlocking));
        DCHK(hipEventCreateWithFlags(&I.ev_fork, hipEventDisableTiming));
        for (int g = 0; g < 4; g++) {
            DCHK(hipEventCreateWithFlags(&I.ev_kb[g], hipEventDisableTiming));
            DCHK(hipEventCreateWithFlags(&I.ev_ki[g], hipEventDisableTiming));
            DCHK(hipEventCreateWithFlags(&I.ev_join[g], hipEventDisableTiming));
        }
        I.ev_made = true;
    }
    {  // (A) fused step: three sets (iteration mod 3) of 2C+8 candidate slots, per-chain hand-over arrays by parity (tables are sized at the first run())
        FusedArgs &f = I.f;
        f.NS = 2 * in.C + 8;
        {   // two chain groups for the fused step (see run()): with the default groups, from 8 chains on
            const int h = (int)(((long)in.C * 1) / 2);
            f.xsplit = (I.G == 2 && h >= 3 && in.C - h >= 3) ? h : in.C;
        }
        const size_t NS = (size_t)f.NS;
        DCHK(I.dalloc(&f.cand_vars, 3 * NS * Nv)); DCHK(I.dalloc(&f.cand_params, 3 * NS * Np)); DCHK(I.dalloc(&f.cand_logPr, 6 * NS));
        DCHK(I.dalloc(&f.cand_stP, 6 * NS)); DCHK(I.dalloc(&f.cand_stR, 3 * NS)); DCHK(I.dalloc(&f.cand_rej, 3 * NS));
        DCHK(I.dalloc(&f.mults, 3 * NS * (size_t)a.desc.per + 1)); DCHK(I.dalloc(&f.pairs, 6 * NS)); DCHK(I.dalloc(&f.nh, 3 * NS)); DCHK(I.dalloc(&f.nn, 3 * NS));
        DCHK(I.dalloc(&f.noise, 3 * NS * (size_t)a.desc.stride));
        DCHK(I.dalloc(&f.slot, 2 * C)); DCHK(I.dalloc(&f.prop_logPr, 2 * C)); DCHK(I.dalloc(&f.prop_st, 2 * C)); DCHK(I.dalloc(&f.quick, 2 * C * QN)); DCHK(I.dalloc(&f.lz, 2 * C * Nv));
        DCHK(I.dalloc(&f.qcount, 3));
        DCHK(hipMemsetAsync(f.qcount, 0, 3 * sizeof(unsigned long long), st));
        // the tiles' per-chain accumulators: one 128-byte line per (set, chain) on a 128-byte boundary, zero between stretches -- once
        // here, then by the commit workgroups (commit_chain); their size does not follow the tile geometry
        static_assert(2 * QK * sizeof(double) == 128, "one line per (set, chain)");
        DCHK(I.dalloc(&f.qacc, 3 * C * 2 * QK));
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
        const size_t role_lds = (Np + 2 * Nv + 1) * sizeof(double) + unpack_lds_bytes() + 32;
        I.fused_ok = !I.rgb && !I.env && role_lds <= sizeof(tile::TileLds<tile::M_FAST_DIRECT, 64>);
    }
    DCHK(hipStreamSynchronize(st));
    return TAMCMC_OK;
}

int DevSampler::download_gradient(double *grad, double *grad_prior) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    if (!I.use_drift || !I.a.grad_cur || !I.grad_valid) return TAMCMC_ERR_BAD_ARG;
    DCHK(hipSetDevice(c->device));
    const size_t n = (size_t)I.a.C * I.a.Nv;
    DCHK(hipStreamSynchronize(c->stream));
    if (grad) DCHK(hipMemcpy(grad, I.a.grad_cur + (size_t)I.parity * n, n * sizeof(double), hipMemcpyDeviceToHost));
    if (grad_prior) DCHK(hipMemcpy(grad_prior, I.a.gradP_cur + (size_t)I.parity * n, n * sizeof(double), hipMemcpyDeviceToHost));
    return TAMCMC_OK;
}

int DevSampler::download_last_proposal(double *vars_prop, double *grad_prop) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    if (!I.use_drift) return TAMCMC_ERR_BAD_ARG;  // (the random-walk schemes keep several candidate proposals per chain, not one)
    DCHK(hipSetDevice(c->device));
    const size_t n = (size_t)I.a.C * I.a.Nv;
    DCHK(hipStreamSynchronize(c->stream));
    if (vars_prop) DCHK(hipMemcpy(vars_prop, I.a.vars_prop, n * sizeof(double), hipMemcpyDeviceToHost));
    if (grad_prop) DCHK(hipMemcpy(grad_prop, I.mala.grad_prop, n * sizeof(double), hipMemcpyDeviceToHost));
    return TAMCMC_OK;
}

int DevSampler::download_tables(int32_t shape[4], tamcmc_multiplet *rows, int32_t *nrows, double *noise, int32_t *nharvey, int32_t *nnoise,
                                int32_t *status, int32_t *written, double *logPr, double *params) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    const DevSamplerArgs &a = I.a;
    const FusedArgs &f = I.f;
    // (ids 25 / 27, random walk: lockstep scheme, the rows k_rgb_finish left in the same block; rows per slot = Nfl0 + Nfl2 + Nfl3 + 400)
    if (I.use_drift || I.env || (!I.rgb && mt::count_multiplets(a.desc.model_id, I.h_plength.data()) < 0)) return TAMCMC_ERR_BAD_MODEL;
    const bool fused = I.last_scheme == 2;
    const size_t C = (size_t)a.C, NS = (size_t)f.NS, n = fused ? 3 * NS : C, per = (size_t)a.desc.per, stride = (size_t)a.desc.stride, Np = (size_t)a.desc.Np;
    if (shape) { shape[0] = I.last_scheme; shape[1] = I.last_scheme ? (int32_t)n : 0; shape[2] = (int32_t)per; shape[3] = (int32_t)stride; }
    if (!I.last_scheme) return TAMCMC_OK;  // (no stretch yet: nothing to read)
    DCHK(hipSetDevice(c->device));
    DCHK(hipStreamSynchronize(c->stream));  // (every entry point returns with the sampler's streams idle)
    const size_t Q = (size_t)I.last_prop_parity;
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
    if (!I.env) return TAMCMC_ERR_BAD_MODEL;
    if (!I.last_scheme) return TAMCMC_ERR_BAD_ARG;  // (no iteration yet: no proposal)
    DCHK(hipSetDevice(c->device));
    DCHK(hipStreamSynchronize(c->stream));  // (every entry point returns with the sampler's streams idle)
    const size_t C = (size_t)a.C, Np = (size_t)a.desc.Np, Q = (size_t)I.last_prop_parity;
    if (rows) {
        std::vector<EnvRow> h(C);
        DCHK(hipMemcpy(h.data(), a.env_rows, C * sizeof(EnvRow), hipMemcpyDeviceToHost));
        for (size_t m = 0; m < C; m++) {  // the layout of tamcmc_sampler.h
            const EnvRow &R = h[m];
            double *r = rows + m * TAMCMC_ENVELOPE_ROW_N;
            r[0] = R.amp; r[1] = R.numax; r[2] = R.sig2; r[3] = R.N0;
            for (int k = 0; k < 2; k++) { r[4 + k] = R.H[k]; r[6 + k] = R.lna[k]; r[8 + k] = R.pw[k]; r[22 + k] = R.hon[k] ? 1.0 : 0.0; }
            for (int k = 0; k < 3; k++) { r[10 + k] = R.b[k]; r[13 + k] = R.lnb[k]; r[16 + k] = R.c[k]; r[19 + k] = R.a2[k]; }
        }
    }
    if (params) DCHK(hipMemcpy(params, a.params_prop + Q * C * Np, C * Np * 8, hipMemcpyDeviceToHost));
    if (logPr) DCHK(hipMemcpy(logPr, a.logPr_prop + Q * C, C * 8, hipMemcpyDeviceToHost));
    if (status) DCHK(hipMemcpy(status, a.status_prop + Q * C, C * 4, hipMemcpyDeviceToHost));
    return TAMCMC_OK;
}

void DevSampler::info(long out[14]) const {
    const Impl &I = *impl;
    unsigned long long qc[3] = {0, 0, 0};  // (every entry point returns with the sampler's streams idle)
    if (I.f.qcount && hipSetDevice(I.ctx->device) == hipSuccess) (void)hipMemcpy(qc, I.f.qcount, sizeof qc, hipMemcpyDeviceToHost);
    out[8] = I.n_stretch; out[9] = (long)qc[0]; out[10] = (long)qc[1]; out[13] = (long)qc[2];
    out[0] = I.a.Nv; out[1] = I.a.desc.Np;
    out[2] = I.use_drift ? I.mala_chol_lds : I.a.chol_in_lds;
    out[3] = I.env ? (I.a.desc.Nx <= env_step_max_bins(I.model_id) ? 1 : 0) : (I.fused_ok && !I.use_drift) ? 1 : 0;  // (ids 0 / 1: k_env_step)
    out[4] = I.G; out[5] = I.it_fused; out[6] = I.it_lockstep; out[7] = I.a.C;
    out[11] = I.it_joint; out[12] = I.it_window;
}

int DevSampler::upload_state(const double *vars, const double *params, const double *logL, const double *logPr,
                             const double *logPost, const double *init_logL) {
    Impl &I = *impl;
    I.armed_it = -1;
    I.grad_valid = false;
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
    {  // launch-order hint from chain 0's table at the uploaded position
        std::vector<tamcmc_multiplet> tab((size_t)a.desc.per > 0 ? (size_t)a.desc.per : 1);
        std::vector<double> nz((size_t)a.desc.stride);
        int n = 0, nh = 0, nn = 0;
        const int tb = tile_bins(c->wgs, c->K);
        I.tile_rot = 0;
        if (I.env) I.tile_rot = 0;  // (no table, and k_loglike's launch order is not used)
        else if (I.rgb) {  // a little below the lowest radial mode (rgb_stage_params' rule)
            const double *fl0 = params + I.h_plength[0] + I.h_plength[1];
            const double fmin = *std::min_element(fl0, fl0 + I.h_plength[2]);
            const int ntiles = (int)((c->Nx + tb - 1) / tb);
            const double t = (fmin - a.desc.x_first) / a.desc.step / (double)tb - 3.0;
            I.tile_rot = (t > 0 && t < ntiles) ? (int)t : 0;
        } else if (build_mode_table(a.desc.model_id, params, I.h_plength.data(), c->hx.data(), c->Nx, tab.data(), a.desc.per, &n, nz.data(), &nh, &nn) == TAMCMC_OK && n <= a.desc.per)
            I.tile_rot = pick_tile_rot(tab.data(), n, a.desc.x_first, a.desc.step, tb, (int)((c->Nx + tb - 1) / tb));
    }
    return TAMCMC_OK;
}

int DevSampler::upload_proposal(int m, const double *L_rowmajor, const double *cov, const double *mu, double sigma) {
    Impl &I = *impl;
    I.armed_it = -1;
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
    DCHK(hipStreamSynchronize(st));
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
    if (!I.d_pack) {
        DCHK(I.dalloc(&I.d_pack, total));
        DCHK(hipHostMalloc((void **)&I.h_pack, total * sizeof(double), hipHostMallocDefault));
    }
    hipLaunchKernelGGL(k_pack_state, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, I.parity, I.d_pack);
    DCHK(hipMemcpyAsync(I.h_pack, I.d_pack, total * sizeof(double), hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    const double *h = I.h_pack;
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
// Stretches without adaptation run as fused steps (A), the others in lockstep (B); see the head of this file.
static std::atomic<int> g_running_calls{0};
struct RunningCall {
    RunningCall() { g_running_calls.fetch_add(1, std::memory_order_relaxed); }
    ~RunningCall() { g_running_calls.fetch_sub(1, std::memory_order_relaxed); }
};

// TAMCMC_CALL_TIMELINE=1: host-side stamps of every run() call on stderr (entry -> first launch -> all launches enqueued -> streams idle)
static const bool g_call_timeline = getenv("TAMCMC_CALL_TIMELINE") != nullptr;
struct CallTimeline {
    std::chrono::steady_clock::time_point t[5];
    int n = 0;
    void mark() { if (g_call_timeline && n < 5) t[n++] = std::chrono::steady_clock::now(); }
    ~CallTimeline() {
        if (!g_call_timeline || n < 2) return;
        fprintf(stderr, "run() timeline (us):");
        for (int k = 1; k < n; k++) fprintf(stderr, " %.1f", std::chrono::duration<double, std::micro>(t[k] - t[k - 1]).count());
        fprintf(stderr, "\n");
    }
};

// The likelihood kernel's time of one run() call (tamcmc_hip_get_timing; only with the context's timing option): which launches are
// bracketed by events, and what the brackets add up to.  The launch code asks for an event pair and gets one or none.
struct DevSampler::Impl::KernelTiming {
    Impl &I;
    tamcmc_hip_ctx *c;
    int used_ev = 0;                             // lockstep: pairs I.ev[0..] handed out since the last drain_events
    std::vector<std::pair<int, long>> fused_ev;  // one-launch fused stretches of this call: (pair of I.ev, launches it brackets)
    // fused step with two chain groups: the launches of an iteration overlap, so the stretch's elapsed time is not a launch duration;
    // sampled launches of the second group are bracketed on their own stream instead
    int g_used = 0;                    // pairs of I.gev handed out in this call
    long g_launches = 0, g_iters = 0;  // launches / iterations of the two-group stretches of this call
    double kernel_ms = 0;
    long n_launch = 0, n_eval = 0;
    bool stretch_timed = false;  // the current fused stretch: timed at all, its pair of I.ev, the next iteration to sample
    int fe = 0;
    long next_sample = 0;

    // lockstep stretch: the pair around launch k when every `every`-th one is sampled (the top 16 pairs: fused stretches)
    hipEvent_t *lockstep_pair(long k, long every) { return c->timing && k % every == 0 && used_ev < I.n_ev - 16 ? I.ev[used_ev++] : nullptr; }
    // ... and their average x launches_represented into the totals.  Call after a stream sync
    int drain_events(double launches_represented, long evals) {
        if (used_ev) {
            double tot = 0;
            for (int e = 0; e < used_ev; e++) {
                float ms = 0;
                DCHK(hipEventElapsedTime(&ms, I.ev[e][0], I.ev[e][1]));
                tot += ms;
            }
            kernel_ms += tot / used_ev * launches_represented;
            n_launch += (long)launches_represented;
            n_eval += evals;
        }
        used_ev = 0;
        return TAMCMC_OK;
    }
    // fused stretch of `len` iterations.  One launch per iteration: two events around the whole stretch, i.e. the average includes the
    // time between two launches.  Two groups: every 97th iteration, or the middle one of a short stretch -- the first two-group
    // iteration with the nominal groups at or after it: a joint iteration there must not leave a short call without a measured launch,
    // and a window's launches (eleven and nine chains at the headline shape) are not what the average is multiplied out for
    void begin_fused(long len) {
        stretch_timed = c->timing && fused_ev.size() < 16;
        fe = I.n_ev - 1 - (int)fused_ev.size();
        next_sample = len >= 97 ? 48 : len / 2;
    }
    hipEvent_t *stretch_pair() { return stretch_timed ? I.ev[fe] : nullptr; }
    hipEvent_t *sampled_pair(long k) {  // k: iteration of the stretch
        if (!(stretch_timed && g_used < I.n_gev && k >= next_sample)) return nullptr;
        next_sample += 97;
        return I.gev[g_used++];
    }
    void end_fused(long len, bool split, long n_split) {
        if (!stretch_timed) return;
        if (!split) fused_ev.push_back({fe, len});
        else { g_launches += 2 * n_split + (len - n_split); g_iters += len; }
    }
    // end of the call, streams idle: the fused stretches' events, then everything into the context's totals
    int total() {
        for (const auto &e : fused_ev) {
            float ms = 0;
            DCHK(hipEventElapsedTime(&ms, I.ev[e.first][0], I.ev[e.first][1]));
            kernel_ms += ms;
            n_launch += e.second;
            n_eval += e.second * (long)I.a.C;
        }
        if (g_launches > 0) {  // two-group stretches: (average duration of the sampled launches) x (launches); one launch = one group's chains
            double tot = 0;
            for (int e = 0; e < g_used; e++) {
                float ms = 0;
                DCHK(hipEventElapsedTime(&ms, I.gev[e][0], I.gev[e][1]));
                tot += ms;
            }
            if (g_used > 0) {
                kernel_ms += tot / g_used * (double)g_launches;
                n_launch += g_launches;
                n_eval += g_iters * (long)I.a.C;
            }
        }
        c->kernel_ms += kernel_ms;
        c->launches += n_launch;
        c->evals += n_eval;
        return TAMCMC_OK;
    }
};

// Copy of a call's records to the caller's (pageable) buffers, on the context stream
static hipError_t copy_records(double *samples, double *stats, const DevSamplerArgs &a, size_t n_iter, hipStream_t st) {
    const size_t C = (size_t)a.C, Nv = (size_t)a.Nv;
    hipError_t e = hipSuccess;
    if (samples) e = hipMemcpyAsync(samples, a.samples, n_iter * C * Nv * 8, hipMemcpyDeviceToHost, st);
    if (stats && e == hipSuccess) e = hipMemcpyAsync(stats, a.stats, n_iter * C * 3 * 8, hipMemcpyDeviceToHost, st);
    return e;
}

// One run() call of the two launch schemes: what every launch of the call needs, filled once by prepare().
struct DevSampler::Impl::RunCall {
    Impl &I;
    tamcmc_hip_ctx *c;
    DevSamplerArgs &a;
    const long it0, n_iter;
    const char *learn;
    double *samples, *stats;
    hipStream_t st;              // the context stream
    CallTimeline &tl;
    KernelTiming T;
    DevSamplerArgs args;         // a, with the record pointers of this call
    LoglikeArgs la[4], lf[3];    // likelihood arguments: (B) per chain group, (A) per candidate set (iteration mod 3)
    int goff[5];                 // chain groups [goff[g], goff[g+1]) of the lockstep scheme
    double *zc_smp = nullptr, *zc_st = nullptr;  // the caller's record buffers as the device sees them (Impl::device_view), else null
    bool use_fused = false;
    bool env_step = false;       // (C): quiet stretches run as k_env_step launches
    int env_nchunk = 0;
    bool split_ok = false;       // fused stretches run as two chain groups [0, f.xsplit), [f.xsplit, C)
    int P;                       // parity of the state buffers that hold the chains' current state
    // (A) the stretch being enqueued
    StepCtl sc{};
    int q = 0;                   // parity of the iteration being enqueued
    // (A) with two groups: the first group's and the joint launches go to st, the second group's to s1 = I.gst[1]; who waits for whom
    // is the plan's business (step_schedule.h: StepPlanner, with its s1_must_wait and s1_ahead)
    bool s1_open = false;        // s1 still holds launches at the end of the call: the host waits for both streams (finish)

    RunCall(Impl &I_, CallTimeline &tl_, long it0_, long n_iter_, const char *learn_, double *samples_, double *stats_)
        : I(I_), c(I_.ctx), a(I_.a), it0(it0_), n_iter(n_iter_), learn(learn_), samples(samples_), stats(stats_), st(I_.ctx->stream),
          tl(tl_), T{I_, I_.ctx}, P(I_.parity) {}

    // tile geometry, scratch and record buffers, the argument blocks
    int prepare() {
        const size_t C = (size_t)a.C, Nv = (size_t)a.Nv;
        const int tb = tile_bins(c->wgs, c->K);
        a.ntiles = (a.desc.Nx + tb - 1) / tb;
        DCHK(c->d_part.reserve(C * (size_t)a.ntiles * 2));
        a.partials = c->d_part.p;
        a.tile_bins = tb;
        a.bg = nullptr;
        use_fused = I.fused_ok && c->step_scheme != 1 && c->wgs == 64 && (c->K == 4 || c->K == 8 || c->K == 16);
        if (I.env) {
            // (C): envelope.hip's 1024-bin tiles whatever the context's geometry options say; the xi partials (id 0) and the tile
            // partials are indexed by chain, so chain groups on different streams never share a slot
            a.ntiles = (a.desc.Nx + ETILE - 1) / ETILE;
            a.tile_bins = ETILE;
            env_nchunk = (a.desc.Nx + ECHUNK - 1) / ECHUNK;
            DCHK(c->d_part.reserve(C * (size_t)a.ntiles * 2));
            a.partials = c->d_part.p;
            DCHK(c->d_env.reserve(C * (size_t)env_nchunk * 3));
            env_step = c->step_scheme != 1 && a.desc.Nx <= env_step_max_bins(I.model_id);
            if (env_step) DCHK(I.env_part.reserve(2 * C * (size_t)a.ntiles * 2));
        }
        I.f.qmargin = c->quick_decide == 1 ? (double)INFINITY : 1e-11;  // (TAMCMC_OPT_QUICK_DECIDE: a test facility)
        const size_t NS = (size_t)I.f.NS;
        I.f.bg = nullptr;
        if (c->precision == TAMCMC_PRECISION_FAST && !I.env) {
            // background series per (slot, tile).  (B): C slots in the context's scratch (rewritten every iteration).  (A): 2 x NS slots of
            // the sampler's OWN -- the candidates prepared by the last launch of a call are carried over to the next call, and anything else
            // that runs on the context in between (another sampler, a batched evaluation) rewrites the context's scratch
            DCHK(c->d_bg.reserve(C * (size_t)a.ntiles * 8));
            a.bg = c->d_bg.p;
            if (use_fused) {
                DCHK(I.fused_bg.reserve(3 * NS * (size_t)a.ntiles * 8));
                I.f.bg = I.fused_bg.p;
            }
        }
        if (use_fused) {  // (A): the tiles' partial sums by iteration parity (launch i writes one half and reads the other)
            DCHK(I.fused_part.reserve(2 * C * (size_t)a.ntiles * 2));
            I.f.part = I.fused_part.p;
        }
        // (two groups pay once one launch no longer fits the GPU's resident waves -- 20 chains x 196 tiles: 27.7 -> 23.9 us, x 782 tiles:
        // 59.8 -> 49.6 us -- and cost below that: 8 chains x 196 tiles 20.5 -> 23.7 us, 20 chains x 20 tiles 33.5 -> 35.6 us;
        // tools/groups_probe.py)
        split_ok = I.f.xsplit < a.C && c->step_scheme != 2 && (c->step_scheme == 3 || (long)a.C * a.ntiles >= 2500);
        // record buffers: at least 256 iterations' worth and grown geometrically, so that a caller that records in buffers of a fixed
        // length (the reference's Nbuffer) or a short call after a shorter one never pays an allocation -- nor, with it, new kernel
        // arguments -- in its steady state (older, smaller buffers are released with the sampler)
        auto grown = [](size_t need, size_t have, size_t unit) { const size_t floor_ = 256 * unit; return std::max(std::max(need, floor_), have * 2); };
        zc_smp = I.device_view(samples, (size_t)n_iter * C * Nv * 8);
        zc_st = I.device_view(stats, (size_t)n_iter * C * 3 * 8);
        if (samples && !zc_smp && I.smp_cap < (size_t)n_iter * C * Nv) {
            const size_t cap = grown((size_t)n_iter * C * Nv, I.smp_cap, C * Nv);
            DCHK(I.dalloc(&a.samples, cap));
            I.smp_cap = cap;
        }
        if (stats && !zc_st && I.stat_cap < (size_t)n_iter * C * 3) {
            const size_t cap = grown((size_t)n_iter * C * 3, I.stat_cap, C * 3);
            DCHK(I.dalloc(&a.stats, cap));
            I.stat_cap = cap;
        }
        args = a;
        args.samples = samples ? (zc_smp ? zc_smp : a.samples) : nullptr;
        args.stats = stats ? (zc_st ? zc_st : a.stats) : nullptr;
        const int G = I.G;
        for (int g = 0; g <= G; g++) goff[g] = (int)(((long)a.C * g) / G);
        auto fill_common = [&](LoglikeArgs &l, int B) {
            l.x = c->dx.p; l.y = c->dy.p; l.logx = c->dlogx.p; l.Nx = a.desc.Nx; l.B = B; l.ntiles = a.ntiles;
            l.x0 = a.desc.x_first; l.step = a.desc.step; l.noise_stride = a.desc.stride; l.model = nullptr; l.tile_rot = I.tile_rot;
        };
        for (int g = 0; g < G; g++) {
            LoglikeArgs &l = la[g];
            const int first = goff[g];
            fill_common(l, goff[g + 1] - goff[g]);
            l.mults = a.mults; l.offsets = a.pairs + 2 * first; l.noise = a.noise + (size_t)first * a.desc.stride;
            l.per = a.desc.per; l.slot0 = first;  // (chain m's table is rows [m per, (m+1) per) of a.mults: dev_unpack.h, rgb_prestep.hip)
            l.nharvey = a.nh + first; l.nnoise = a.nn + first; l.partials = a.partials + (size_t)first * a.ntiles * 2;
            l.bg_poly = a.bg ? a.bg + (size_t)first * a.ntiles * 8 : nullptr;
        }
        for (int e = 0; e < 3; e++) {  // (A): evaluation m = chain m, its table in a slot of candidate set e = iteration mod 3 (decide())
            LoglikeArgs &l = lf[e];
            const FusedArgs &f = I.f;
            fill_common(l, a.C);
            l.mults = f.mults + (size_t)e * NS * a.desc.per; l.offsets = f.pairs + (size_t)e * 2 * NS; l.noise = f.noise + (size_t)e * NS * a.desc.stride;
            l.nharvey = f.nh + (size_t)e * NS; l.nnoise = f.nn + (size_t)e * NS; l.partials = f.part;
            l.bg_poly = f.bg ? f.bg + (size_t)e * NS * a.ntiles * 8 : nullptr;
            l.per = a.desc.per; l.slot0 = 0;
        }
        return TAMCMC_OK;
    }

    int swap_pair_of(long it) const { return swap_pair(a.seed, a.C, a.dN_mixing, it, nullptr); }

    // ---- (B) one iteration per round over [ia, ib): k_iterate settles iteration it-1 and proposes iteration it
    int run_lockstep(long ia, long ib) {
        const int G = I.G;
        const size_t C = (size_t)a.C;
        I.armed_it = -1;
        I.it_lockstep += ib - ia;
        // the extra streams start after everything already enqueued on the context stream
        if (G > 1) {
            DCHK(hipEventRecord(I.ev_fork, st));
            for (int g = 1; g < G; g++) DCHK(hipStreamWaitEvent(I.gst[g], I.ev_fork, 0));
        }
        const long len = ib - ia;
        const long ev_every = len > 32 ? len / 32 : 1;
        int pending = 0, have_pre = 0;
        for (long i = ia; i <= ib; i++) {
            const long it = it0 + i;
            const int learn_p = (pending && learn && learn[i - 1]) ? 1 : 0;
            // L z of iteration it+1 can be computed by spare workgroups of THIS launch when no adaptation rewrites L in this
            // launch (learn_p) nor in the next one before its proposal (learn[i])
            const int make_pre = (i + 1 < ib && !learn_p && !(learn && learn[i])) ? 1 : 0;
            const int pre_flags = (have_pre ? 1 : 0) | (make_pre ? 2 : 0);
            const size_t lds = I.lds_base + ((learn_p && a.chol_in_lds) ? I.lds_adapt : 0);
            const long rec = (pending && (samples || stats)) ? i - 1 : (long)-1;
            // does settling iteration it-1 swap a pair that straddles two groups? (same draw as the kernel: Philox is host/device)
            int gA = -1, gB = -1;
            if (pending && G > 1) {
                const int A = swap_pair_of(it - 1);
                if (A >= 0 && group_of(A, goff, G) != group_of(A + 1, goff, G)) { gA = group_of(A, goff, G); gB = group_of(A + 1, goff, G); }
            }
            if (gA >= 0) {  // each of the two groups needs the other's k_loglike(it-1) before it settles the pair
                DCHK(hipEventRecord(I.ev_kb[gA], I.gst[gA]));
                DCHK(hipEventRecord(I.ev_kb[gB], I.gst[gB]));
                DCHK(hipStreamWaitEvent(I.gst[gA], I.ev_kb[gB], 0));
                DCHK(hipStreamWaitEvent(I.gst[gB], I.ev_kb[gA], 0));
            }
            for (int g = 0; g < G; g++) {
                const int cnt = goff[g + 1] - goff[g];
                if (i < ib)
                    hipLaunchKernelGGL(k_iterate<true>, dim3(make_pre ? 2 * cnt : cnt), dim3(TB), lds, I.gst[g], args, it, P, pending, rec, learn_p,
                                       I.adapt_scratch, goff[g], cnt, pre_flags, I.rgb ? rgb_device_slice(c, I.rgb_bmax, g) : rgb::Slice());
                else  // settle the last iteration of this stretch (MH test, swap, record, adaptation); nothing is proposed
                    hipLaunchKernelGGL(k_iterate<false>, dim3(cnt), dim3(TB), lds, I.gst[g], args, it, P, pending, rec, learn_p, I.adapt_scratch,
                                       goff[g], cnt, 0, rgb::Slice());
            }
            have_pre = make_pre;
            if (gA >= 0) {  // ... and must not overwrite (next iteration) what the other group's settle is still reading
                DCHK(hipEventRecord(I.ev_ki[gA], I.gst[gA]));
                DCHK(hipEventRecord(I.ev_ki[gB], I.gst[gB]));
                DCHK(hipStreamWaitEvent(I.gst[gA], I.ev_ki[gB], 0));
                DCHK(hipStreamWaitEvent(I.gst[gB], I.ev_ki[gA], 0));
            }
            P ^= 1;
            pending = 1;
            if (i < ib && I.rgb) {  // the proposals' tables: solver, then sort / zeta / rows (and the FAST background series)
                RgbDeviceTables R;
                R.mults = a.mults; R.pairs = a.pairs; R.nh = a.nh; R.nn = a.nn; R.noise = a.noise; R.stride = a.desc.stride;
                R.status = a.status_prop + (size_t)P * C;
                R.bg = a.bg; R.ntiles = a.ntiles; R.tile_bins = a.tile_bins;
                for (int g = 0; g < G; g++) {
                    int rc = rgb_device_stage(c, goff[g], goff[g + 1] - goff[g], I.rgb_bmax, g, a.desc.per, R, I.gst[g]);
                    if (rc) return rc;
                }
            }
            if (i < ib) {
                for (int g = 0; g < G; g++) {
                    hipEvent_t *pair = g == 0 ? T.lockstep_pair(i - ia, ev_every) : nullptr;
                    if (pair) DCHK(hipEventRecord(pair[0], I.gst[g]));
                    if (I.env) {  // the rows k_iterate has just written -> the partials the next k_iterate's accept_result sums
                        const size_t first = (size_t)goff[g];
                        if (int rc = envelope_stage_enqueue(c, I.model_id, goff[g + 1] - goff[g], a.env_rows + first, c->d_env.p + first * env_nchunk * 3,
                                                            a.partials + first * a.ntiles * 2, I.gst[g]))
                            return rc;
                    } else {
                        DCHK(launch_loglike(la[g], c->precision, c->wgs, c->K, false, I.gst[g]));
                    }
                    if (pair) DCHK(hipEventRecord(pair[1], I.gst[g]));
                }
            }
        }
        I.last_scheme = 1;
        I.last_prop_parity = P ^ 1;  // (the closing launch read the last proposals from parity P before the flip above)
        // join: the context stream continues after every group
        for (int g = 1; g < G; g++) {
            DCHK(hipEventRecord(I.ev_join[g], I.gst[g]));
            DCHK(hipStreamWaitEvent(st, I.ev_join[g], 0));
        }
        if (c->timing) {  // (with chain groups every launch carries C/G evaluations and overlaps the other groups' kernels)
            DCHK(hipStreamSynchronize(st));
            return T.drain_events((double)len * G, len * (long)a.C);
        }
        return TAMCMC_OK;
    }

    // Device-memory image of the two argument blocks, for the fused step's function calls (re-uploaded only when a pointer or size
    // changed since the last run; the candidates carried over from the last call were built for the old buffers then)
    int sync_arg_image() {
        const size_t n1 = (sizeof(DevSamplerArgs) + 15) & ~(size_t)15, n2 = sizeof(FusedArgs);
        std::vector<unsigned char> img(n1 + n2, 0);
        std::memcpy(img.data(), &args, sizeof(DevSamplerArgs));
        std::memcpy(img.data() + n1, &I.f, sizeof(FusedArgs));
        if (!I.d_argcopy) DCHK(I.dalloc(&I.d_argcopy, n1 + n2));
        if (img != I.h_argcopy) {
            DCHK(hipMemcpyAsync(I.d_argcopy, img.data(), n1 + n2, hipMemcpyHostToDevice, st));
            DCHK(hipStreamSynchronize(st));  // (img is a stack object)
            I.h_argcopy = img;
            I.armed_it = -1;
        }
        sc.ga = (const DevSamplerArgs *)I.d_argcopy;
        sc.gf = (const FusedArgs *)(I.d_argcopy + n1);
        return TAMCMC_OK;
    }

    // Entry of a fused stretch at iteration ia, unless the last call's final launch has prepared it (armed): L z of the first two
    // iterations, then the candidates of iteration ia built on the settled chains (state of parity q).  *launched: whether it was needed
    int fused_entry(long ia, bool *launched) {
        *launched = !(I.armed_it == it0 + ia && I.armed_q == q);
        if (!*launched) return TAMCMC_OK;
        const int nbr = 8 * I.f.NS;                // candidate roles, a multiple of 8 (keeps the tiles' XCD mapping)
        const int nlz2 = ((2 * a.C + 7) / 8) * 8;
        sc.it = it0 + ia; sc.rec = -1; sc.q = q; sc.flags = ST_LZ; sc.nbr = 0; sc.nlz = nlz2; sc.n_lz_live = 2 * a.C; sc.it_lz = it0 + ia; sc.q_lz = q;
        DCHK(launch_step(c->precision, c->K, nlz2, st, args, I.f, lf[0], sc));
        sc.flags = ST_ENTRY; sc.nbr = nbr; sc.nlz = 0; sc.n_lz_live = 0;
        DCHK(launch_step(c->precision, c->K, nbr, st, args, I.f, lf[0], sc));
        return TAMCMC_OK;
    }

    // Launch i of a stretch for chains [first, first + cnt): the tiles of iteration i (each decides iteration i-1 for its chain first),
    // the chains' commit workgroups (state, record and counters of iteration i-1), the candidates of iteration i+1, the L z of iteration
    // i+2.  A, A_prev: the swap pairs of iterations i and i-1; settled: the chains are settled (first launch of a stretch: nothing to
    // decide or commit).  ev: an event pair around the kernel, or null.
    int launch_group(int first, int cnt, int A, int A_prev, long i, bool settled, hipStream_t stream, hipEvent_t *ev = nullptr) {
        const bool owns_pair = A >= first && A + 1 < first + cnt;
        const int ntiles_pad = ((a.ntiles + 7) / 8) * 8;
        sc.it = it0 + i; sc.rec = ((samples || stats) && !settled) ? i - 1 : (long)-1; sc.q = q;
        sc.flags = ST_L | ST_BR | ST_LZ | ST_COMMIT | (settled ? ST_FIRST : 0);
#ifdef TAMCMC_PROBE  // timing experiments only (results are wrong): leave kinds of workgroups out of the launch
        if (const char *ep = getenv("TAMCMC_PROBE_STEP")) {
            const int pm = atoi(ep);
            if (pm & 1) sc.flags &= ~ST_BR;
            if (pm & 2) sc.flags &= ~ST_COMMIT;
            if (pm & 4) sc.flags &= ~ST_LZ;
            if (pm & 8) sc.flags |= ST_FIRST;
            if (pm & 16) sc.flags &= ~ST_L;
        }
#endif
        sc.first = first; sc.cnt = cnt; sc.extra = owns_pair ? 1 : 0; sc.pairA = settled ? -1 : A_prev;
        sc.nbr = 8 * (2 * cnt + (owns_pair ? 4 : 0)); sc.nlz = ((2 * cnt + 7) / 8) * 8; sc.n_lz_live = cnt; sc.it_lz = it0 + i + 2; sc.q_lz = q;
        LoglikeArgs lq = lf[(it0 + i) % 3];
        lq.B = cnt;
        lq.partials = I.f.part + ((size_t)q * a.C + first) * a.ntiles * 2;
        DCHK(launch_step(c->precision, c->K, sc.nbr + sc.nlz + ntiles_pad * cnt, stream, args, I.f, lq, sc, ev ? ev[0] : nullptr, ev ? ev[1] : nullptr));
        return TAMCMC_OK;
    }

    // After the last iteration ib-1 of a stretch: the commit workgroups alone (iteration ib-1 decided, the chains settled in parity q).
    int launch_close(int first, int cnt, long ib, hipStream_t stream) {
        sc.it = it0 + ib; sc.rec = (samples || stats) ? ib - 1 : (long)-1; sc.q = q;
        sc.flags = ST_COMMIT;
        sc.first = first; sc.cnt = cnt; sc.extra = 0;
        sc.nbr = 0; sc.nlz = ((cnt + 7) / 8) * 8; sc.n_lz_live = 0; sc.it_lz = 0; sc.q_lz = 0;
        DCHK(launch_step(c->precision, c->K, sc.nlz, stream, args, I.f, lf[0], sc));
        return TAMCMC_OK;
    }

    int s1_waits_for_st() {
        DCHK(hipEventRecord(I.ev_fork, st));
        DCHK(hipStreamWaitEvent(I.gst[1], I.ev_fork, 0));
        return TAMCMC_OK;
    }
    int st_waits_for_s1() {
        DCHK(hipEventRecord(I.ev_join[1], I.gst[1]));
        DCHK(hipStreamWaitEvent(st, I.ev_join[1], 0));
        return TAMCMC_OK;
    }

    // ---- (A) fused steps over [ia, ib) (no adaptation inside): one launch per iteration on the context stream, or two (one per chain group).
    // Two chain groups, each with its own launch per iteration on its own stream: a launch is a chain of dependent steps (sums ->
    // decision -> table rows -> tile, ~18 us even for five chains) that leaves most of the GPU idle at its two ends; the two groups'
    // launches fill each other's ends.  Nothing is shared between the groups' launches except at a swap whose pair (xsplit-1, xsplit)
    // straddles the groups.  For that iteration and the next (a window) the boundary moves by one chain -- [0, xsplit+1) on st,
    // [xsplit+1, C) on s1 -- so that the pair lies inside the first group's launch: st waits for s1 once on the way in (chain xsplit's
    // earlier launches are there), s1 waits for st once on the way out, and the rest of the second group keeps running through both
    // hops (profiles/r05_straddle_summary.md: the cost of the joint launches this replaces, and of what is left).  Only a window iteration whose own or previous pair is (xsplit, xsplit+1) is
    // still one joint launch over all chains, on st after both groups' earlier launches.  step_schedule.h (StepPlanner) decides all of
    // this, iteration by iteration, with every wait; here the plan is enqueued.  (Same chains bit for bit: the launches hold the same
    // workgroups, every buffer of the step is per chain, and a chain's cross candidates stay in the extra block named by f.xsplit.)
    int run_fused(long ia, long ib) {
        const long len = ib - ia;
        hipStream_t s1 = I.gst[1];
        I.it_fused += len;
        I.n_stretch += 1;
        q = P;
        sc = StepCtl{};
        if (int rc = sync_arg_image()) return rc;
        sc.first = 0; sc.cnt = a.C; sc.extra = 1;
        bool entered;
        if (int rc = fused_entry(ia, &entered)) return rc;
        StepPlanner plan(split_ok, a.C, I.f.xsplit);
        // does the context stream hold work of this call that the second group's stream has to wait for?  (Every entry point of the
        // library returns with its streams idle, so a call that starts on carried-over candidates has nothing to wait for: the event
        // hop would only delay the second group's first launch by 12-14 us, profiles/r05_straddle_summary.md.)
        plan.s1_must_wait = ia > 0 || entered;
        plan.s1_ahead = false;
        T.begin_fused(len);
        if (!split_ok && T.stretch_pair()) DCHK(hipEventRecord(T.stretch_pair()[0], st));
        long n_two = 0;
        int A_prev = -1;
        for (long i = ia; i < ib; i++) {
            const int A = swap_pair_of(it0 + i);
            const bool settled = i == ia;
            const StepPlan p = plan.next(A);
            if (p.st_waits_s1) if (int rc = st_waits_for_s1()) return rc;
            if (p.s1_waits_st) if (int rc = s1_waits_for_st()) return rc;
            if (int rc = launch_group(0, p.b, A, A_prev, i, settled, st)) return rc;
            if (p.b < a.C) {
                if (int rc = launch_group(p.b, a.C - p.b, A, A_prev, i, settled, s1, p.window ? nullptr : T.sampled_pair(i - ia))) return rc;
                n_two++;
                I.it_window += p.window ? 1 : 0;
            } else if (split_ok) I.it_joint += 1;
            A_prev = A;
            q ^= 1;
        }
        // the closing launches, over the ranges the last iteration's pair asks for (iteration ib-1's swap is decided by them)
        const StepPlan p = plan.next(-1);
        if (p.st_waits_s1) if (int rc = st_waits_for_s1()) return rc;
        if (p.s1_waits_st) if (int rc = s1_waits_for_st()) return rc;
        if (int rc = launch_close(0, p.b, ib, st)) return rc;
        if (p.b < a.C) {
            if (int rc = launch_close(p.b, a.C - p.b, ib, s1)) return rc;
            if (ib >= n_iter) s1_open = true;  // the call's last stretch: the host waits for both streams (no event hop on the GPU)
            else if (int rc = st_waits_for_s1()) return rc;
        }
        if (!split_ok && T.stretch_pair()) DCHK(hipEventRecord(T.stretch_pair()[1], st));  // (read after the call's final synchronisation)
        T.end_fused(len, split_ok, n_two);
        P = q;
        I.armed_it = it0 + ib;
        I.armed_q = q;
        I.last_scheme = 2;
        return TAMCMC_OK;
    }

    // ---- (C) k_env_step over [ia, ib) (no adaptation inside): one launch per iteration on the context stream, then a settle-only launch
    template <int KIND>
    int run_env_step_kind(long ia, long ib) {
        const long len = ib - ia;
        if (KIND == 0 && env_nchunk > ENV_STEP_MAX_CHUNKS) return TAMCMC_ERR_BAD_ARG;  // (k_env_step's chunk partials in LDS; prepare() never routes this here)
        I.armed_it = -1;
        I.it_fused += len;
        I.n_stretch += 1;
        const size_t half = (size_t)a.C * a.ntiles * 2;
        const size_t lds = env_step_lds_bytes((size_t)a.desc.Np, (size_t)a.Nv);
        EnvStepArgs e;
        e.x = c->dx.p; e.y = c->dy.p; e.logx = c->dlogx.p;
        e.h = c->hx[1] - c->hx[0]; e.xmax = c->xmax; e.nchunk = env_nchunk;
        T.begin_fused(len);
        if (T.stretch_pair()) DCHK(hipEventRecord(T.stretch_pair()[0], st));
        int pending = 0;
        for (long i = ia; i <= ib; i++) {
            const long rec = (pending && (samples || stats)) ? i - 1 : (long)-1;
            DevSamplerArgs la_ = args;
            la_.partials = I.env_part.p + (size_t)P * half;  // what the previous launch of the stretch wrote
            e.part_wr = I.env_part.p + (size_t)(P ^ 1) * half;
            if (i < ib) hipLaunchKernelGGL((k_env_step<KIND, true>), dim3(a.ntiles, a.C), dim3(TB), lds, st, la_, e, it0 + i, P, pending, rec);
            else hipLaunchKernelGGL((k_env_step<KIND, false>), dim3(1, a.C), dim3(TB), lds, st, la_, e, it0 + i, P, pending, rec);
            P ^= 1;
            pending = 1;
        }
        DCHK(hipGetLastError());
        if (T.stretch_pair()) DCHK(hipEventRecord(T.stretch_pair()[1], st));  // (read after the call's final synchronisation)
        T.end_fused(len, false, 0);
        I.last_scheme = 2;
        I.last_prop_parity = P ^ 1;  // (the closing launch read the last proposals from parity P before the flip above)
        return TAMCMC_OK;
    }
    int run_env_step(long ia, long ib) {
        return I.model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN ? run_env_step_kind<0>(ia, ib) : run_env_step_kind<1>(ia, ib);
    }

    // every launch is enqueued: the records, the wait for the streams, the kernel times
    int finish() {
        I.parity = P;
        DCHK(hipGetLastError());
        tl.mark();  // (every launch enqueued)
        double *const staged_smp = (samples && !zc_smp) ? samples : nullptr, *const staged_st = (stats && !zc_st) ? stats : nullptr;
        if (s1_open && (staged_smp || staged_st)) {  // (the copies below read what the second group's launches write)
            if (int rc = st_waits_for_s1()) return rc;
            s1_open = false;
        }
        DCHK(copy_records(staged_smp, staged_st, a, (size_t)n_iter, st));
        const bool poll = g_running_calls.load(std::memory_order_relaxed) == 1;
        if (s1_open) DCHK(Impl::wait_stream(I.gst[1], poll));
        DCHK(Impl::wait_stream(st, poll));
        tl.mark();  // (streams idle)
        return T.total();
    }
};

int DevSampler::run(long it0, long n_iter, const char *learn, double *samples, double *stats) {
    RunningCall running_call;
    CallTimeline tl;
    tl.mark();
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    if (n_iter <= 0) return TAMCMC_OK;
    if (I.use_drift) return run_mala(it0, n_iter, learn, samples, stats);
    DCHK(hipSetDevice(c->device));
    Impl::RunCall r(I, tl, it0, n_iter, learn, samples, stats);
    if (int rc = r.prepare()) return rc;
    tl.mark();  // (set-up of the call done: buffers, argument blocks)
    for (long i = 0, end = 0; i < n_iter; i = end) {
        bool is_fused;
        next_stretch(learn, n_iter, i, r.use_fused || r.env_step, &end, &is_fused);
        if (int rc = !is_fused ? r.run_lockstep(i, end) : r.env_step ? r.run_env_step(i, end) : r.run_fused(i, end)) return rc;
    }
    return r.finish();
}

// The Langevin engine (use_drift): per iteration k_mala_settle (settle it-1, propose it) -> the finite-difference batch of the proposals
// (k_fd_unpack -- red giants: k_fd_rgb_perturb and the pre-step --, base k_loglike with model rows, k_loglike<DELTA>, k_finalize x2)
// -> k_mala_test.  See dev_mala_impl.h.
int DevSampler::run_mala(long it0, long n_iter, const char *learn, double *samples, double *stats) {
    Impl &I = *impl;
    tamcmc_hip_ctx *c = I.ctx;
    DevSamplerArgs &a = I.a;
    DCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    I.armed_it = -1;
    const size_t C = (size_t)a.C, Nv = (size_t)a.Nv, Np = (size_t)a.desc.Np;
    const FdBatch::Buffers fd_ws{I.fd_part, I.fd_S, I.fd_model, I.fd_bg};
    // Red giants under STRICT: the batch would need the host's long-double unpack of every proposal (FdBatch::h_prep), and the proposals
    // exist on the device only.  Refused here, before anything is enqueued or counted: state, iteration and gradients stay as they are
    if (I.rgb && c->precision == TAMCMC_PRECISION_STRICT) return TAMCMC_ERR_BAD_ARG;
    {   // the batch's layout follows the context's options (arithmetic mode, geometry, windowed differences): re-laid out when they change
        // (red giants: layout() also re-reserves the context's pre-step workspace for the batch's chunk -- another sampler or a direct
        // gradient call may have been the last to size it; the slice is taken from the context at every enqueue, never kept.  A route
        // the model has not -- the adjoint -- is refused by layout() with the chains where they were)
        FdBatch nb;
        int rc = nb.layout(c, FdBatch::Request::FromOptions, I.model_id, I.prior_class, a.C, (int64_t)Np, I.h_plength.data(), a.Nv);
        if (rc) return rc;
        const bool need_bg = c->precision == TAMCMC_PRECISION_FAST && !I.fd_bg.p;  // (a switch to FAST between two calls keeps every size)
        if (nb.total_bytes != I.fd.total_bytes || nb.route != I.fd.route || nb.ntiles != I.fd.ntiles || nb.rgb != I.fd.rgb ||
            nb.chunk != I.fd.chunk || !I.fd_block.p || need_bg) {
            I.fd = nb;
            rc = ensure_poly(c);
            if (rc) return rc;
            DCHK(I.fd_block.reserve(nb.total_bytes));
            FdInputs in;  // the layout's constants; the vectors come from the device at every enqueue, the steps from k_mala_steps
            in.priors = I.h_priors.data(); in.extra_priors = I.h_extra.data(); in.priors_switch = I.h_sw.data();
            in.plength = I.h_plength.data(); in.index_to_relax = I.h_idx.data();
            std::vector<unsigned char> hb(nb.head.in_bytes);
            nb.head.stage(hb.data(), in);
            DCHK(hipMemcpyAsync(I.fd_block.p, hb.data(), nb.head.in_bytes, hipMemcpyHostToDevice, st));
            DCHK(hipStreamSynchronize(st));
            DCHK(nb.reserve(c, fd_ws));
            I.grad_valid = false;
        }
    }
    FdBatch &fd = I.fd;
    unsigned char *db = I.fd_block.p;
    fd.count_slots = c->timing && fd.hybrid();  // (hybrid red-giant batches: linearised / fallback slots of this call, counted on the device)
    if (fd.count_slots) DCHK(fd.zero_slot_counts(c, db));
    MalaArgs M = I.mala;
    const FdResults res = fd.head.results(db);  // (the device block: read by k_mala_test)
    M.S = I.fd_S.p; M.lpp = res.lpp; M.lpm = res.lpm; M.st = res.status;
    M.h = fd.head.hstep(db); M.E = fd.E; M.deltas = fd.deltas() ? 1 : 0; M.fd_step_rel = I.fd_step_rel; M.delta = I.delta;
    if (samples && I.smp_cap < (size_t)n_iter * C * Nv) {
        DCHK(I.dalloc(&a.samples, (size_t)n_iter * C * Nv));
        I.smp_cap = (size_t)n_iter * C * Nv;
    }
    if (stats && I.stat_cap < (size_t)n_iter * C * 3) {
        DCHK(I.dalloc(&a.stats, (size_t)n_iter * C * 3));
        I.stat_cap = (size_t)n_iter * C * 3;
    }
    DevSamplerArgs args = a;
    if (!samples) args.samples = nullptr;
    if (!stats) args.stats = nullptr;
    const size_t lds_settle = (4 * Nv + Np + 1 + 8) * sizeof(double) + 32;
    const size_t lds_test0 = (5 * Nv + 8) * sizeof(double) + 32, lds_adapt = (Nv * Nv + Nv) * sizeof(double);
    const bool chol_lds = lds_test0 + lds_adapt <= 156 * 1024;
    args.chol_in_lds = chol_lds ? 1 : 0;
    I.mala_chol_lds = args.chol_in_lds;
    I.it_lockstep += n_iter;
    if (!chol_lds && !I.adapt_scratch) DCHK(I.dalloc(&I.adapt_scratch, C * (Nv * Nv + Nv)));
    if (lds_test0 + lds_adapt > 64 * 1024 && chol_lds)
        DCHK(hipFuncSetAttribute((const void *)k_mala_test, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_test0 + lds_adapt)));
    int P = I.parity;
    auto batch = [&](const double *d_params, bool timed) -> int {
        return fd.enqueue(c, db, d_params, fd_ws, timed ? I.ev[0][0] : nullptr, timed ? I.ev[0][1] : nullptr);
    };
    if (!I.grad_valid) {  // gradient at the chains' current positions (start of a run, new positions from outside)
        hipLaunchKernelGGL(k_mala_steps, dim3(1), dim3(256), 0, st, args, M);
        int rc = batch(a.params_cur + (size_t)P * C * Np, false);
        if (rc) return rc;
        hipLaunchKernelGGL(k_mala_ginit, dim3(a.C), dim3(TB), 2 * Nv * sizeof(double), st, args, M, P);
        DCHK(hipGetLastError());
        I.grad_valid = true;
    }
    double kernel_ms = 0;
    long n_timed = 0, fd_bins_sampled = 0;
    int pending = 0;
    for (long i = 0; i <= n_iter; i++) {
        const long it = it0 + i;
        const long rec = (pending && (samples || stats)) ? i - 1 : (long)-1;
        if (i < n_iter) hipLaunchKernelGGL(k_mala_settle<true>, dim3(a.C), dim3(TB), lds_settle, st, args, M, it, P, pending, rec);
        else hipLaunchKernelGGL(k_mala_settle<false>, dim3(a.C), dim3(TB), lds_settle, st, args, M, it, P, pending, rec);
        P ^= 1;
        pending = 1;
        if (i == n_iter) break;
        const bool timed = c->timing && (i == 0 || i == n_iter / 2);  // two sampled batches per call (an event read needs a synchronisation)
        int rc = batch(a.params_prop, timed);
        if (rc) return rc;
        const int learn_i = (learn && learn[i]) ? 1 : 0;
        // (the adaptation's work area is reserved in every step when it fits: without adaptation the triangular solves keep the factor there)
        hipLaunchKernelGGL(k_mala_test, dim3(a.C), dim3(TB), lds_test0 + (chol_lds ? lds_adapt : 0), st, args, M, it, P, learn_i,
                           I.adapt_scratch);
        if (timed) {
            DCHK(hipStreamSynchronize(st));
            float ms = 0;
            DCHK(hipEventElapsedTime(&ms, I.ev[0][0], I.ev[0][1]));
            kernel_ms += ms;
            n_timed++;
            if (fd.route == FdBatch::Route::Windowed) {  // what the delta launch really touched (roofline bookkeeping, as fd_run does)
                long bins = 0;
                DCHK(fd.delta_stats(db, &bins, nullptr));
                fd_bins_sampled += bins;
            }
        }
    }
    I.parity = P;
    DCHK(hipGetLastError());
    DCHK(copy_records(samples, stats, a, (size_t)n_iter, st));
    DCHK(hipStreamSynchronize(st));
    if (fd.count_slots) {
        long lin = 0, fall = 0;
        DCHK(fd.hybrid_stats(c, db, &lin, &fall));
        c->rgb_adj_lin += lin;
        c->rgb_adj_fallback += fall;
    }
    if (n_timed) {  // (the sampled batches stand for all of them)
        c->kernel_ms += kernel_ms / n_timed * n_iter;
        c->launches += n_iter;
        c->evals += n_iter * (long)fd.B;
        c->fd_bins += fd_bins_sampled / n_timed * n_iter;
        c->fd_delta_evals += fd.route == FdBatch::Route::Windowed ? n_iter * (long)fd.B : 0;
    }
    return TAMCMC_OK;
}

}  // namespace tamcmc
