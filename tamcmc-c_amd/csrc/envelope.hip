// envelope.hip -- Gaussian-envelope background fits on the device: model_Kallinger2014_Gaussian (id 0), model_Harvey_Gaussian (id 1).
//
// Both models are evaluated on every bin of the fitted range for every parameter vector: there is no window to skip.  Per bin they cost
// one exp for the Gaussian, one exp per active power law ((a x)^p = exp(p (ln a + ln x)) on the context's resident ln x), an IEEE
// reciprocal-by-divide per power law, the sinc^2 leakage filter (id 0) and the log of the likelihood term.
//
// Kernel sequence of one batch (stream order, no grid-wide barrier, no cooperative launch):
//   k_env_ksi   (id 0 only)  grid (chunks, B): per (vector, chunk of 4096 bins) the three trapezoid partial sums of get_ksinorm
//                            sum_i w_i / (1 + (x_i/b_k)^c_k), w = 1/2 on the first and last bin of the spectrum;
//   k_env_eval               grid (tiles, B): every workgroup of vector b first reduces b's chunk partials in a fixed order (so every tile
//                            of b sees the same xi_k bit for bit), then forms the model on its 1024 bins, writes the row (optional) and
//                            its partial sums of y/M and ln M;
//   k_finalize (kernels.hip) one workgroup per vector: the tile partials in a fixed order -> S[b].
// The chunk and tile sizes depend on Nx only, never on B, and every sum runs in a fixed order: a vector's logL is bit-identical whatever
// batch it sits in and whatever its position there.
//
// Who owns what.  envelope_row.h: the row builder, the xi term, the bodies of the two passes (the model of a bin, twice); the
// device-resident sampler's one-launch step (k_env_step, dev_env_step_impl.h) evaluates its tiles through the same bodies.  This file:
// the kernels around those bodies, and on the host ONE staging of rows (env_stage_rows), ONE statement of the evaluation's launches
// (env_launch_eval: the batch and the sampler's lockstep route both call it), ONE statement of the analytic gradient's launches
// (env_launch_grad: the gradient entries and the device-resident Langevin step both call it), ONE gradient run for the brute-force and the analytic
// likelihood share (envelope_gradient_run) behind ONE front door for the two gradient entries (envelope_gradient).  The tempered
// log-likelihood and the gradient's assembly are grad_assemble.h's, the timing totals ctx.h's (account_kernel_time).
//
// One arithmetic mode (TAMCMC_OPT_PRECISION does not apply): double, the reference's order of operations per bin except for the power laws
// taken through exp/log and the trapezoid sums taken as a tree instead of a left-to-right loop.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/tamcmc_hip.h"
#include "ctx.h"
#include "envelope.h"
#include "envelope_row.h"
#include "fd_batch.h"
#include "grad_assemble.h"
#include "kernels.h"
#include "priors_impl.h"

namespace tamcmc {

namespace {

__global__ void __launch_bounds__(EWG) k_env_ksi(const double *logx, int Nx, int nchunk, const EnvRow *rows, double *part) {
    __shared__ double s_red[3 * (EWG / 64)];
    const int chunk = blockIdx.x, b = blockIdx.y;
    double out[3];
    env_ksi_chunk(logx, Nx, chunk, rows[b], s_red, out);
    if (threadIdx.x == 0) {
        double *p = part + ((size_t)b * nchunk + chunk) * 3;
        p[0] = out[0];
        p[1] = out[1];
        p[2] = out[2];
    }
}

template <int KIND, bool WRITE_MODEL>  // KIND: model id (0 Kallinger, 1 Harvey)
__global__ void __launch_bounds__(EWG) k_env_eval(const double *x, const double *y, const double *logx, int Nx, int ntiles, int nchunk,
                                                  double h, double xmax, const EnvRow *rows, const double *ksi_part,
                                                  double *model, double *part) {
    __shared__ double s_red[3 * (EWG / 64)];
    __shared__ double s_coef[3];
    const int tile = blockIdx.x, b = blockIdx.y;
    const EnvRow &R = rows[b];
    if (KIND == 0) env_ksi_coef(ksi_part + (size_t)b * nchunk * 3, nchunk, h, R, s_red, s_coef);
    double out[2];
    env_tile<KIND, WRITE_MODEL>(x, y, logx, Nx, tile, xmax, R, s_coef, WRITE_MODEL ? model + (size_t)b * Nx : nullptr, s_red, out);
    if (threadIdx.x == 0) {
        double *p = part + ((size_t)b * ntiles + tile) * 2;
        p[0] = out[0];
        p[1] = out[1];
    }
}

// ---- analytic gradient (TAMCMC_OPT_ENVELOPE_GRADIENT = 1): the same geometry, one pass over the bins per vector ----
//   k_env_ksi_grad (id 0)  grid (chunks, C): k_env_ksi's three sums (same bits, same place: d_env) and the nine that carry the
//                          normalisation integrals' dependence on b_k and c_k;
//   k_env_grad             grid (tiles, C): env_ksi_coef as k_env_eval has it, then the tile's two sums of S (the layout k_finalize reads)
//                          and its 10 / 16 gradient sums, one partial per (vector, tile);
//   k_env_grad_fold        one workgroup per vector: the tile partials (and id 0's chunk partials) in a fixed order, no atomics; S[b] by
//                          k_finalize's statements (same strides, same tree), so the bits of the evaluation route.
__global__ void __launch_bounds__(EWG) k_env_ksi_grad(const double *logx, int Nx, int nchunk, const EnvRow *rows, double *part, double *gpart) {
    __shared__ double s_red[ENV_GRAD_NKRAW * (EWG / 64)];
    const int chunk = blockIdx.x, b = blockIdx.y;
    double out[ENV_GRAD_NKRAW];
    env_ksi_grad_chunk(logx, Nx, chunk, rows[b], s_red, out);
    if (threadIdx.x == 0) {
        double *p = part + ((size_t)b * nchunk + chunk) * 3, *g = gpart + ((size_t)b * nchunk + chunk) * (ENV_GRAD_NKRAW - 3);
        for (int k = 0; k < 3; k++) p[k] = out[k];
        for (int k = 0; k < ENV_GRAD_NKRAW - 3; k++) g[k] = out[3 + k];
    }
}

template <int KIND>
__global__ void __launch_bounds__(EWG) k_env_grad(const double *x, const double *y, const double *logx, int Nx, int ntiles, int nchunk, double h,
                                                  double xmax, const EnvRow *rows, const double *ksi_part, double *part, double *gpart) {
    constexpr int NG = KIND == 0 ? ENV_GRAD_NRAW0 : ENV_GRAD_NRAW1;
    __shared__ double s_red[(2 + NG) * (EWG / 64)];
    __shared__ double s_coef[3];
    const int tile = blockIdx.x, b = blockIdx.y;
    const EnvRow &R = rows[b];
    if (KIND == 0) env_ksi_coef(ksi_part + (size_t)b * nchunk * 3, nchunk, h, R, s_red, s_coef);
    double out[2 + NG];
    env_grad_tile<KIND>(x, y, logx, Nx, tile, xmax, R, s_coef, s_red, out);
    if (threadIdx.x == 0) {
        double *p = part + ((size_t)b * ntiles + tile) * 2, *g = gpart + ((size_t)b * ntiles + tile) * NG;
        p[0] = out[0];
        p[1] = out[1];
#pragma unroll
        for (int j = 0; j < NG; j++) g[j] = out[2 + j];
    }
}

// per vector: the NG tile sums -> gsum[b * ENV_GRAD_NRAWMAX ...]; id 0: the chunk sums -> ksum[b * ENV_GRAD_NKRAW ...], the first three summed as
// env_ksi_coef sums them (the I_k every tile used); S[b] from the tiles' two sums as k_finalize (kernels.hip) forms it
template <int NG>
__global__ void __launch_bounds__(EWG) k_env_grad_fold(const double *part, const double *gpart, int ntiles, const double *ksi_part,
                                                       const double *ksi_gpart, int nchunk, double *S, double *gsum, double *ksum) {
    __shared__ double s_red[(2 + NG) * (EWG / 64)];
    const int b = blockIdx.x;
    double s[2 + NG], out[2 + NG];
#pragma unroll
    for (int j = 0; j < 2 + NG; j++) s[j] = 0.0;
    for (int t = threadIdx.x; t < ntiles; t += EWG) {
        const double *q = part + ((size_t)b * ntiles + t) * 2, *p = gpart + ((size_t)b * ntiles + t) * NG;
        s[0] = s[0] + q[0];
        s[1] = s[1] + q[1];
#pragma unroll
        for (int j = 0; j < NG; j++) s[2 + j] = s[2 + j] + p[j];
    }
    env_block_reduce<2 + NG>(s, s_red, out);
    if (threadIdx.x == 0) {
        S[b] = out[0] + out[1];
        for (int j = 0; j < NG; j++) gsum[(size_t)b * ENV_GRAD_NRAWMAX + j] = out[2 + j];
        for (int j = NG; j < ENV_GRAD_NRAWMAX; j++) gsum[(size_t)b * ENV_GRAD_NRAWMAX + j] = 0.0;
    }
    if (NG != ENV_GRAD_NRAW0) return;
    __syncthreads();
    constexpr int NK = ENV_GRAD_NKRAW;
    double k9[NK], o9[NK];
#pragma unroll
    for (int j = 0; j < NK; j++) k9[j] = 0.0;
    for (int ch = threadIdx.x; ch < nchunk; ch += EWG) {
        const double *p = ksi_part + ((size_t)b * nchunk + ch) * 3, *g = ksi_gpart + ((size_t)b * nchunk + ch) * (NK - 3);
#pragma unroll
        for (int j = 0; j < 3; j++) k9[j] = k9[j] + p[j];
#pragma unroll
        for (int j = 0; j < NK - 3; j++) k9[3 + j] = k9[3 + j] + g[j];
    }
    env_block_reduce<NK>(k9, s_red, o9);
    if (threadIdx.x == 0)
        for (int j = 0; j < NK; j++) ksum[(size_t)b * NK + j] = o9[j];
}

// log-priors of n parameter vectors (rows of Np doubles): one thread each, the serial evaluation of priors_impl.h in double
__global__ void __launch_bounds__(64) k_env_prior(int prior_class, int n, const double *P, long Np, const double *pp, const int *sw, double *lp,
                                                  int *status) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= n) return;
    int st = TAMCMC_OK;
    lp[v] = (double)pr::prior_serial(prior_class, P + (size_t)v * Np, nullptr, Np, pp, sw, nullptr, &st);
    status[v] = st;
}

// Tiles and chunks of the resident spectrum (they depend on Nx only) and get_ksinorm's step
struct EnvGeom {
    int Nx, ntiles, nchunk;
    double h;  // x(1) - x(0), whatever the rest of the grid does
    explicit EnvGeom(const tamcmc_hip_ctx *c)
        : Nx((int)c->Nx), ntiles((Nx + ETILE - 1) / ETILE), nchunk((Nx + ECHUNK - 1) / ECHUNK), h(c->hx[1] - c->hx[0]) {}
};

// THE staging of rows: n vectors -> EnvRow each (host: h_stage, which keeps them until the next staging) and their upload to d_stage
// on the context stream.  Between the staging buffers' reservation and the upload it reserves what the kernels behind it write, the
// tile partials (d_part, n x ntiles x 2) and the caller's `sums`: the order in which the entries have always reserved them.
int env_stage_rows(tamcmc_hip_ctx *c, int model_id, int n, int ntiles, const double *params, int64_t Nparams, DevBuf<double> &sums,
                   size_t nsums) {
    const size_t row_bytes = (size_t)n * sizeof(EnvRow);
    HIPCHK(c, c->h_stage.reserve(row_bytes));
    HIPCHK(c, c->d_stage.reserve(row_bytes));
    HIPCHK(c, c->d_part.reserve((size_t)n * ntiles * 2));
    HIPCHK(c, sums.reserve(nsums));
    EnvRow *hr = (EnvRow *)c->h_stage.p;
    for (int b = 0; b < n; b++) env_row(model_id, params + (size_t)b * Nparams, hr[b]);
    HIPCHK(c, hipMemcpyAsync(c->d_stage.p, c->h_stage.p, row_bytes, hipMemcpyHostToDevice, c->stream));
    return TAMCMC_OK;
}
const EnvRow *staged_rows_host(const tamcmc_hip_ctx *c) { return (const EnvRow *)c->h_stage.p; }
const EnvRow *staged_rows_dev(const tamcmc_hip_ctx *c) { return (const EnvRow *)c->d_stage.p; }

// THE launches of the evaluation: k_env_ksi (id 0) into ksi_part, then k_env_eval for `cnt` rows into `partials` (and model_dev, if
// any).  check_each: the launch error is read after k_env_ksi too (the batch); otherwise once, after both (the sampler's lockstep route)
int env_launch_eval(tamcmc_hip_ctx *c, int model_id, int cnt, const EnvRow *rows, double *ksi_part, double *model_dev, double *partials,
                    hipStream_t st, bool check_each) {
    const EnvGeom g(c);
    const bool kal = model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN;
    if (kal) {
        hipLaunchKernelGGL(k_env_ksi, dim3(g.nchunk, cnt), dim3(EWG), 0, st, c->dlogx.p, g.Nx, g.nchunk, rows, ksi_part);
        if (check_each) HIPCHK(c, hipGetLastError());
    }
    const auto eval = kal ? (model_dev ? k_env_eval<0, true> : k_env_eval<0, false>) : (model_dev ? k_env_eval<1, true> : k_env_eval<1, false>);
    hipLaunchKernelGGL(eval, dim3(g.ntiles, cnt), dim3(EWG), 0, st, c->dx.p, c->dy.p, c->dlogx.p, g.Nx, g.ntiles, g.nchunk, g.h, c->xmax, rows,
                       kal ? ksi_part : nullptr, model_dev, partials);
    HIPCHK(c, hipGetLastError());
    return TAMCMC_OK;
}

// THE launches of the analytic gradient for `cnt` rows: k_env_ksi_grad (id 0), k_env_grad, k_env_grad_fold.  The gradient entries
// (envelope_grad_enqueue, the context's buffers) and the device-resident Langevin step (envelope_grad_stage_enqueue, the sampler's)
// both call it: the same statements in the same orders, so S[b] has the evaluation's bits on either
int env_launch_grad(tamcmc_hip_ctx *c, int model_id, int cnt, const EnvRow *rows, const EnvGradBuffers &b, hipStream_t st) {
    const EnvGeom g(c);
    const dim3 grid(g.ntiles, cnt);
    if (model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN) {
        hipLaunchKernelGGL(k_env_ksi_grad, dim3(g.nchunk, cnt), dim3(EWG), 0, st, c->dlogx.p, g.Nx, g.nchunk, rows, b.ksi_part, b.ksi_gpart);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL((k_env_grad<0>), grid, dim3(EWG), 0, st, c->dx.p, c->dy.p, c->dlogx.p, g.Nx, g.ntiles, g.nchunk, g.h, c->xmax, rows, b.ksi_part, b.part, b.gpart);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL((k_env_grad_fold<ENV_GRAD_NRAW0>), dim3(cnt), dim3(EWG), 0, st, b.part, b.gpart, g.ntiles, b.ksi_part, b.ksi_gpart, g.nchunk, b.S, b.gsum, b.ksum);
    } else {
        hipLaunchKernelGGL((k_env_grad<1>), grid, dim3(EWG), 0, st, c->dx.p, c->dy.p, c->dlogx.p, g.Nx, g.ntiles, g.nchunk, g.h, c->xmax, rows, nullptr, b.part, b.gpart);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL((k_env_grad_fold<ENV_GRAD_NRAW1>), dim3(cnt), dim3(EWG), 0, st, b.part, b.gpart, g.ntiles, nullptr, nullptr, 0, b.S, b.gsum, b.ksum);
    }
    HIPCHK(c, hipGetLastError());
    return TAMCMC_OK;
}

// the copy of n sums (d_S) behind the kernels
int env_fetch_sums(tamcmc_hip_ctx *c, const double *dev, size_t n) {
    HIPCHK(c, c->h_S.reserve(n));
    HIPCHK(c, hipMemcpyAsync(c->h_S.p, dev, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return TAMCMC_OK;
}

int env_check(tamcmc_hip_ctx *c, int model_id, int64_t Nparams) {
    if (Nparams < envelope_nparams(model_id)) return TAMCMC_ERR_BAD_ARG;
    if (c->Nx > 0x7fffffff / 2) return TAMCMC_ERR_BAD_ARG;
    return TAMCMC_OK;
}

}  // namespace

int envelope_enqueue(tamcmc_hip_ctx *c, int model_id, int B, const double *params, int64_t Nparams, double *model_dev) {
    const EnvGeom g(c);
    if (int rc = env_stage_rows(c, model_id, B, g.ntiles, params, Nparams, c->d_S, (size_t)B)) return rc;
    hipStream_t st = c->stream;
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev0, st));
    if (model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN) HIPCHK(c, c->d_env.reserve((size_t)B * g.nchunk * 3));
    if (int rc = env_launch_eval(c, model_id, B, staged_rows_dev(c), c->d_env.p, model_dev, c->d_part.p, st, true)) return rc;
    HIPCHK(c, launch_finalize(c->d_part.p, B, g.ntiles, c->d_S.p, st));
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev1, st));
    return TAMCMC_OK;
}

// The sampler's lockstep route: the rows are on the device already (written by k_iterate), one per chain
int envelope_stage_enqueue(tamcmc_hip_ctx *c, int model_id, int cnt, const void *rows_dev, double *ksi_part, double *partials, hipStream_t st) {
    return env_launch_eval(c, model_id, cnt, (const EnvRow *)rows_dev, ksi_part, nullptr, partials, st, false);
}

// The device-resident Langevin step: the analytic gradient's kernels on the rows k_env_mala_front has left on the device
int envelope_grad_stage_enqueue(tamcmc_hip_ctx *c, int model_id, int cnt, const void *rows_dev, const EnvGradBuffers &b, hipStream_t st) {
    return env_launch_grad(c, model_id, cnt, (const EnvRow *)rows_dev, b, st);
}

int envelope_loglike_params_batch(tamcmc_hip_ctx *c, int model_id, int B, const double *params, int64_t Nparams, const double *Tcoefs,
                                  double p, double *logL, double *model, int32_t *status) {
    int rc = env_check(c, model_id, Nparams);
    if (rc) return rc;
    const int64_t Nx = c->Nx;
    if (model) HIPCHK(c, c->d_model.reserve((size_t)B * Nx));
    rc = envelope_enqueue(c, model_id, B, params, Nparams, model ? c->d_model.p : nullptr);
    if (rc) return rc;
    hipStream_t st = c->stream;
    if ((rc = env_fetch_sums(c, c->d_S.p, (size_t)B))) return rc;
    if (model) HIPCHK(c, hipMemcpyAsync(model, c->d_model.p, (size_t)B * Nx * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if ((rc = account_kernel_time(c, B))) return rc;
    for (int b = 0; b < B; b++) {
        logL[b] = tempered_loglike(c->h_S.p[b], p, temperature_of(Tcoefs, b));
        if (status) status[b] = TAMCMC_OK;  // these models have no table that can fail: a non-finite vector gives a non-finite logL
    }
    return TAMCMC_OK;
}

// The points of a gradient batch, C x (Nvars + 1) rows per block: forward points theta + h e_k (the same double addition the
// gradient's divisor uses), then (backward) a second block with the backward points theta - h e_k
static std::vector<double> env_fd_points(int C, const double *params, int64_t Nparams, const int32_t *index_to_relax, int Nvars,
                                         const double *hstep, bool backward) {
    const int E = Nvars + 1;
    const size_t B = (size_t)C * E, Np = (size_t)Nparams;
    std::vector<double> P((backward ? 2 : 1) * B * Np);
    for (int ch = 0; ch < C; ch++)
        for (int e = 0; e < E; e++) {
            double *f = P.data() + ((size_t)ch * E + e) * Np;
            std::memcpy(f, params + (size_t)ch * Np, Np * 8);
            if (e > 0) f[index_to_relax[e - 1]] = params[(size_t)ch * Np + index_to_relax[e - 1]] + hstep[e - 1];
            if (backward) {
                double *g = P.data() + (B + (size_t)ch * E + e) * Np;
                std::memcpy(g, params + (size_t)ch * Np, Np * 8);
                if (e > 0) g[index_to_relax[e - 1]] = params[(size_t)ch * Np + index_to_relax[e - 1]] - hstep[e - 1];
            }
        }
    return P;
}

// Log-priors of the 2B points of env_fd_points on the device (k_env_prior), behind whatever the stream holds; synchronises.  lp: 2B
// values; *first_err: the first status that is not TAMCMC_OK
static int env_prior_points(tamcmc_hip_ctx *c, int prior_class, size_t B, const double *P, int64_t Nparams, const double *priors,
                            const int32_t *priors_switch, std::vector<double> &lp, int *first_err) {
    hipStream_t st = c->stream;
    const size_t Np = (size_t)Nparams;
    // one block: [vectors 2B x Np | priors 4 x Np | switch Np (int) ] in, [lp 2B | status 2B (int)] out
    const size_t nP = 2 * B * Np, o_pp = nP * 8, o_sw = o_pp + 4 * Np * 8, o_lp = (o_sw + Np * 4 + 15) & ~(size_t)15,
                 o_st = o_lp + 2 * B * 8, bytes = o_st + 2 * B * 4;
    HIPCHK(c, c->h_fd.reserve(bytes));
    HIPCHK(c, c->d_fd.reserve(bytes));
    unsigned char *hb = c->h_fd.p, *db = c->d_fd.p;
    std::memcpy(hb, P, nP * 8);
    std::memcpy(hb + o_pp, priors, 4 * Np * 8);
    std::memcpy(hb + o_sw, priors_switch, Np * 4);
    HIPCHK(c, hipMemcpyAsync(db, hb, o_lp, hipMemcpyHostToDevice, st));
    const int n = (int)(2 * B);
    hipLaunchKernelGGL(k_env_prior, dim3((n + 63) / 64), dim3(64), 0, st, prior_class, n, (const double *)db, (long)Np,
                       (const double *)(db + o_pp), (const int *)(db + o_sw), (double *)(db + o_lp), (int *)(db + o_st));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hb + o_lp, db + o_lp, bytes - o_lp, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    lp.assign((const double *)(hb + o_lp), (const double *)(hb + o_lp) + 2 * B);
    const int *lst = (const int *)(hb + o_st);
    for (size_t s = 0; s < 2 * B; s++)
        if (lst[s] != TAMCMC_OK && *first_err == TAMCMC_OK) *first_err = lst[s];
    return TAMCMC_OK;
}

// The analytic route's kernels for C vectors and the copy of what they fold: S (C), the tile sums (C x 16) and the xi sums (C x 12),
// one block of d_envg and then of h_S
static int envelope_grad_enqueue(tamcmc_hip_ctx *c, int model_id, int C, const double *params, int64_t Nparams) {
    const EnvGeom g(c);
    const bool kal = model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN;
    const int NG = env_grad_nraw(model_id);
    // d_envg: [S C | folded C x (16 + 12) | tile partials C x ntiles x NG | chunk partials C x nchunk x 9]; S sits in front of the
    // folded sums so that one copy brings both back
    const size_t o_tile = (size_t)C * (1 + ENV_GRAD_NRAWMAX + ENV_GRAD_NKRAW), o_chunk = o_tile + (size_t)C * g.ntiles * NG,
                 total = o_chunk + (kal ? (size_t)C * g.nchunk * (ENV_GRAD_NKRAW - 3) : 0);
    if (int rc = env_stage_rows(c, model_id, C, g.ntiles, params, Nparams, c->d_envg, total)) return rc;
    hipStream_t st = c->stream;
    EnvGradBuffers b;
    b.S = c->d_envg.p; b.gsum = b.S + C; b.ksum = b.gsum + (size_t)C * ENV_GRAD_NRAWMAX;
    b.gpart = c->d_envg.p + o_tile; b.ksi_gpart = c->d_envg.p + o_chunk;
    b.part = c->d_part.p;
    if (kal) HIPCHK(c, c->d_env.reserve((size_t)C * g.nchunk * 3));
    b.ksi_part = c->d_env.p;
    double *Sdev = b.S;
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev0, st));
    if (int rc = env_launch_grad(c, model_id, C, staged_rows_dev(c), b, st)) return rc;
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev1, st));
    return env_fetch_sums(c, Sdev, (size_t)C * (1 + ENV_GRAD_NRAWMAX + ENV_GRAD_NKRAW));
}

// What envelope_grad_enqueue brought back, once the stream is idle: S is h_S's first C values; dS / d(row quantity) (C x ENV_GRAD_N) and
// the xi sums (C x 9) in long double, which every caller goes on from
static void envelope_grad_unfold(const tamcmc_hip_ctx *c, int model_id, int C, std::vector<long double> &dS, std::vector<long double> &ksi) {
    const double h = EnvGeom(c).h;
    const EnvRow *hr = staged_rows_host(c);
    const double *raw = c->h_S.p + C, *kraw = raw + (size_t)C * ENV_GRAD_NRAWMAX;
    dS.assign((size_t)C * ENV_GRAD_N, 0.0L);
    ksi.assign((size_t)C * ENV_GRAD_NKSI, 0.0L);
    for (int b = 0; b < C; b++)
        env_grad_rows(model_id, hr[b], h, raw + (size_t)b * ENV_GRAD_NRAWMAX, kraw + (size_t)b * ENV_GRAD_NKRAW, dS.data() + (size_t)b * ENV_GRAD_N,
                      ksi.data() + (size_t)b * ENV_GRAD_NKSI);
}

int envelope_gradient_sums(tamcmc_hip_ctx *c, int model_id, int C, const double *params, int64_t Nparams, double *S, double *sums, double *ksi) {
    int rc = env_check(c, model_id, Nparams);
    if (rc) return rc;
    if (C > 65535) return TAMCMC_ERR_BAD_ARG;  // grid.y
    if ((rc = envelope_grad_enqueue(c, model_id, C, params, Nparams))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = account_kernel_time(c, C))) return rc;
    std::vector<long double> dS, ks;
    envelope_grad_unfold(c, model_id, C, dS, ks);
    for (int b = 0; b < C; b++) S[b] = c->h_S.p[b];
    for (size_t i = 0; i < dS.size(); i++) sums[i] = (double)dS[i];
    if (ksi && model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN)
        for (size_t i = 0; i < ks.size(); i++) ksi[i] = (double)ks[i];
    return TAMCMC_OK;
}

// Chain rule of the analytic route: dS / d(row quantity) of C vectors -> dlogL / dtheta_k (C x Nvars), tempered, in long double
static std::vector<double> envelope_chain_rule(int model_id, int C, const double *params, int64_t Nparams, const int32_t *index_to_relax, int Nvars,
                                               const double *Tcoefs, double p, const std::vector<long double> &dS) {
    const int NpJ = (int)envelope_nparams(model_id);
    std::vector<long double> J((size_t)ENV_GRAD_N * NpJ);
    std::vector<double> gL((size_t)C * Nvars);
    for (int ch = 0; ch < C; ch++) {
        env_row_jacobian(model_id, params + (size_t)ch * Nparams, J.data());
        for (int k = 0; k < Nvars; k++) {
            const int j = index_to_relax[k];
            const long double s = env_chain_contract(dS.data() + (size_t)ch * ENV_GRAD_N, J.data(), NpJ, j);  // (a parameter the model does not read: exactly 0)
            gL[(size_t)ch * Nvars + k] = s == 0.0L ? 0.0 : tempered_loglike(s, p, temperature_of(Tcoefs, ch));  // (+0, not -p * 0)
        }
    }
    return gL;
}

// THE gradient run of ids 0 and 1.  Shared: the checks, the forward (and, with a prior, backward) points, the prior's share -- the
// log-priors of those points on the device (k_env_prior, prior class 0 / 1 of priors_impl.h), one thread per point -- and the assembly.
// The likelihood's share: brute force, the C x (Nvars + 1) forward points evaluated in one batch; or (analytic,
// TAMCMC_OPT_ENVELOPE_GRADIENT = 1) one pass over the bins per chain and the chain rule on the host.  Stream order on either route:
// the likelihood's kernels, the copy of their sums, the prior's upload / kernel / download, one synchronise.
static int envelope_gradient_run(tamcmc_hip_ctx *c, int model_id, bool analytic, bool with_prior, int prior_class, int C, const double *params,
                                 int64_t Nparams, const int32_t *index_to_relax, int Nvars, const double *hstep, const double *Tcoefs, double p,
                                 const double *priors, const int32_t *priors_switch, double *logL0, double *logPr0, double *grad,
                                 double *grad_prior) {
    int rc = env_check(c, model_id, Nparams);
    if (rc) return rc;
    if (with_prior && prior_class != model_id) return TAMCMC_ERR_BAD_MODEL;  // priors_ctrl.list pairs class 0 with id 0, class 1 with id 1
    const size_t B = (size_t)C * (Nvars + 1);
    if (B > 65535) return TAMCMC_ERR_BAD_ARG;  // grid.y of the brute-force batch (the analytic route keeps the limit: the prior keeps the points)
    std::vector<double> P;
    if (!analytic || with_prior) P = env_fd_points(C, params, Nparams, index_to_relax, Nvars, hstep, with_prior);
    if (analytic) rc = envelope_grad_enqueue(c, model_id, C, params, Nparams);
    else if (!(rc = envelope_enqueue(c, model_id, (int)B, P.data(), Nparams, nullptr))) rc = env_fetch_sums(c, c->d_S.p, B);
    if (rc) return rc;
    std::vector<double> lp;
    int first_err = TAMCMC_OK;
    if (with_prior) {
        if ((rc = env_prior_points(c, prior_class, B, P.data(), Nparams, priors, priors_switch, lp, &first_err))) return rc;
    } else {
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if ((rc = account_kernel_time(c, analytic ? C : (int64_t)B))) return rc;
    std::vector<double> gL;
    if (analytic) {
        std::vector<long double> dS, ks;
        envelope_grad_unfold(c, model_id, C, dS, ks);
        gL = envelope_chain_rule(model_id, C, params, Nparams, index_to_relax, Nvars, Tcoefs, p, dS);
    }
    // (no status per evaluation: these models have no table that can fail)
    assemble_gradient(C, Nvars, params, Nparams, index_to_relax, hstep, Tcoefs, p, analytic ? LikelihoodShare::Derivative : LikelihoodShare::FullSums,
                      c->h_S.p, analytic ? gL.data() : nullptr, with_prior ? lp.data() : nullptr, with_prior ? lp.data() + B : nullptr, nullptr,
                      logL0, logPr0, grad, grad_prior);
    return first_err;
}

int envelope_gradient(tamcmc_hip_ctx *c, int model_id, bool with_prior, int prior_class, int C, const double *params, int64_t Nparams,
                      const int32_t *index_to_relax, int Nvars, const double *hstep, const double *Tcoefs, double p, const double *priors,
                      const int32_t *priors_switch, double *logL0, double *logPr0, double *grad, double *grad_prior) {
    if (!c) return TAMCMC_ERR_BAD_ARG;
    if (c->gradient == TAMCMC_GRADIENT_ADJOINT) return TAMCMC_ERR_BAD_MODEL;  // (no mode table: no table-space adjoint)
    const int rc = check_gradient_args(c, C, params, Nparams, nullptr, index_to_relax, Nvars, hstep,
                                       logL0 && grad && (!with_prior || (priors && priors_switch)), GA_VARS);
    if (rc) return rc;
    if (with_prior && prior_class != 0 && prior_class != 1) return TAMCMC_ERR_BAD_MODEL;
    if (C == 0) return TAMCMC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return envelope_gradient_run(c, model_id, c->envelope_gradient != 0, with_prior, prior_class, C, params, Nparams, index_to_relax, Nvars, hstep,
                                 Tcoefs, p, priors, priors_switch, logL0, logPr0, grad, grad_prior);
}

}  // namespace tamcmc
