// ctx.h -- private definition of the opaque context of include/tamcmc_hip.h (shared by capi.hip and dev_sampler.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/tamcmc_hip.h"

namespace tamcmc {

template <typename T>
struct DevBuf {  // grow-only device buffer; released with its owner at the latest (the device must be current then)
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = n + n / 2 + 64;
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

template <typename T>
struct PinBuf {  // grow-only pinned host buffer; released with its owner at the latest
    T *p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { release(); }
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = n + n / 2 + 64;
        hipError_t e = hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace tamcmc

struct tamcmc_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_split[7] = {};  // stage boundaries of a hybrid red-giant batch (fd_batch.hip; created at the first timed one)
    std::string err;
    // options
    int precision = TAMCMC_PRECISION_STRICT;
    int timing = 0;
    int wgs = 256;  // workgroup size of k_loglike: 256 (4 waves per tile) or 64 (one wave per tile)
    int K = 4;      // bins per thread: tile = wgs*K bins
    bool geom_user_set = false;
    int fd_windowed = 1;  // FAST modes: finite differences through delta tables (changed multiplets on their windows only)
    int step_scheme = 0;  // device sampler: 0 = fused steps where possible (one or two launches per iteration: automatic), 1 = lockstep kernels only,
                          // 2 = fused, always one launch per iteration, 3 = fused, two chain groups whenever the chain count allows
    int quick_decide = 0; // device sampler, fused step (a test facility): 1 = every margin test of the decision shortcut answers "undecided"
    int armm_dense = 0;   // red-giant pre-step: 1 = dense grid walk
    int64_t fisher_ws_mb = 2048;  // tamcmc_hip_fisher: budget of the model rows kept on the device per pass, MiB (fd_rgb_chunk.h: fisher_chunk)
    int gradient = TAMCMC_GRADIENT_FD;  // gradient batches: finite differences, or the table-space adjoint with frozen windows (adjoint.h)
    int rgb_device_langevin = 0;  // 1: the device-resident engine builds its Langevin sampler for the red-giant ids (read at sampler creation)
    int rgb_adjoint = 0;  // 1: under TAMCMC_GRADIENT_ADJOINT the red-giant ids take the hybrid batch (fd_batch.hip; read at every call)
    int rgb_fisher = 0;  // 1: tamcmc_hip_fisher accepts the red-giant ids (fisher.hip: k_fisher_freeze_rgb; read at every call)
    int envelope_device_engine = 0;  // 1: the device-resident engine is built for the Gaussian-envelope ids 0 / 1 (read at sampler creation)
    int envelope_device_langevin = 0;  // 1: ... and its Langevin step (use_drift = 1) for ids 0 / 1; independent of envelope_device_engine (read at sampler creation)
    int factor_refresh = 0;  // R of TAMCMC_OPT_FACTOR_REFRESH: < 2 a full factorisation per adapting iteration, else rank-one steps (read at sampler creation)
    int envelope_gradient = 0;  // 1: the gradient batches of ids 0 / 1 take the analytic likelihood share (envelope.hip; read at every call)
    // resident spectrum
    int64_t Nx = 0;
    std::vector<double> hx;  // host copy of x (table builders need x[0], x[Nx-1], step)
    double xmax = 0;         // largest x (the leakage filter of the Kallinger model, envelope.hip)
    tamcmc::DevBuf<double> dx, dy, dlogx;
    // ONE pinned staging block and its device image per call (a single H2D copy):
    //   [int32 begin/end pairs 2B | int32 nharvey B | int32 nnoise B | pad] [double noise B*stride] [multiplets]
    tamcmc::PinBuf<unsigned char> h_stage;
    tamcmc::DevBuf<unsigned char> d_stage;
    tamcmc::DevBuf<double> d_part, d_S, d_model;
    tamcmc::DevBuf<unsigned char> d_rgb;  // red-giant pre-step workspace (rgb_prestep.hip)
    tamcmc::PinBuf<unsigned char> h_rgb;  // its pinned host image: [Prep B | RowIn B] going up, [int status B] coming back
    tamcmc::DevBuf<double> d_env;  // Gaussian-envelope fits: per (vector, chunk) trapezoid sums of the Kallinger normalisations
    tamcmc::DevBuf<double> d_envg;  // their analytic gradient: folded sums per vector, tile and chunk partials (envelope_grad_enqueue)
    tamcmc::DevBuf<double> d_bg;  // FAST far field: background series per (evaluation, tile) (bg_series.h)
    // finite-difference batches built on the device (fd_batch.hip)
    tamcmc::DevBuf<unsigned char> d_fd, d_poly;
    tamcmc::PinBuf<unsigned char> h_fd;
    bool poly_ready = false;
    tamcmc::DevBuf<double> d_fisher;  // Fisher information (fisher.hip): 1/h_applied, weights, slab partials, F
    double fisher_ms[3] = {0, 0, 0};  // last tamcmc_hip_fisher call with timing on: table build, row launches, Gram + fold (HIP events, summed over passes)
    int64_t rgb_fisher_forms[3] = {0, 0, 0};  // ... of a red giant: (chain, variable) pairs on the central, one-sided, unfrozen form (summed over passes)
    tamcmc::PinBuf<double> h_S;
    // samplers created on this context (they borrow its stream and buffers): tamcmc_hip_destroy with samplers still attached only
    // marks the context; the last tamcmc_sampler_destroy frees it -- any destruction order is safe
    int attached = 0;
    bool zombie = false;
    // stats
    double kernel_ms = 0;
    int64_t launches = 0, evals = 0;
    int64_t fd_full_evals = 0;                // ... of which "full table" evaluations (fd_batch.hip)
    int64_t fd_bins = 0, fd_delta_evals = 0;  // windowed finite differences (timing on): bins inside the affected ranges, delta evaluations
    int64_t rgb_adj_lin = 0, rgb_adj_fallback = 0;  // hybrid red-giant batches (timing on): perturbed slots contracted / sent through the DELTA launch
    double rgb_adj_ms[6] = {0, 0, 0, 0, 0, 0};  // last hybrid batch of a host entry with timing on: tables, base launch, row pass, noise pass + fold, fallback delta, contraction
};

namespace tamcmc {
struct StageLayout {
    size_t off_pairs, off_nh, off_nn, off_noise, off_mults, bytes;
    StageLayout(int B, int stride, size_t total_mults) {
        off_pairs = 0;
        off_nh = off_pairs + (size_t)2 * B * sizeof(int32_t);
        off_nn = off_nh + (size_t)B * sizeof(int32_t);
        off_noise = (off_nn + (size_t)B * sizeof(int32_t) + 15) & ~(size_t)15;
        off_mults = (off_noise + (size_t)B * stride * sizeof(double) + 15) & ~(size_t)15;
        bytes = off_mults + (total_mults + 1) * sizeof(tamcmc_multiplet);
    }
};
}  // namespace tamcmc

#define HIPCHK(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                   \
            return TAMCMC_ERR_HIP;                                                            \
        }                                                                                     \
    } while (0)

// Timing on: the likelihood launches a host entry bracketed with ev0 / ev1, into the totals of tamcmc_hip_get_kernel_stats -- their
// device time, one launch, `evals` evaluations.  Call after the stream is synchronised.
inline int account_kernel_time(tamcmc_hip_ctx *c, int64_t evals) {
    if (!c->timing) return TAMCMC_OK;
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->kernel_ms += ms;
    c->launches += 1;
    c->evals += evals;
    return TAMCMC_OK;
}
