// model_stats.hip -- posterior model spectrum: per-bin mean, spread, envelope and data/model ratio of the model M over a stream of
// parameter vectors, reduced over the SAMPLES axis on the device (what Diagnostics::gnuplt_model_diags of the reference plots from
// models it evaluates one by one on the host, diagnostics.cpp; include/tamcmc_hip.h states the law).
//
// k_model_stats: the loop nest of k_loglike turned inside out.  One workgroup = 256 threads = one tile of 256 consecutive bins, one bin
// per lane; it walks the staged tables of a chunk of vectors IN INDEX ORDER, compacts each vector's overlapping multiplets into LDS with
// the likelihood tile's staging pass (loglike_tile.h, table order), evaluates M at its bin with the STRICT per-bin operation order
// (strict_mult, then harvey_like: the bits k_loglike<STRICT, .., WRITE_MODEL> writes, whatever TAMCMC_OPT_PRECISION says) and updates
// seven accumulators held in registers; they are loaded once and stored once per launch.  No reduction over bins, no atomics, nothing
// crosses a workgroup: a bin's result depends on the sequence of vectors alone -- not on the tile size, the chunk size or the split of
// the stream over calls.  Nothing proportional to (vectors x bins) is stored or copied.
//
// Geometry: one bin per lane is all the parallelism the bins axis has (1e5 bins = 1563 waves, 1.5 per SIMD of 256 CUs); four waves share
// a tile so that one staging pass (64 rows by wave 0) serves 256 bins, and 1e5 bins give 391 workgroups for 256 CUs.  x, y and the
// seven planes are read and written coalesced (lane i -> bin base + i).
//
// This file is compiled with -ffp-contract=off and holds no fused multiply-add: every operation of the law is rounded on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/tamcmc_hip.h"
#include "kernels.h"
#include "loglike_tile.h"
#include "model_stats.h"
#include "mode_tables.h"
#include "rgb_prestep.h"
#include "envelope.h"
#include "ctx.h"

namespace tamcmc {

namespace {

using namespace tile;

__global__ void __launch_bounds__(MS_TILE) k_model_stats(const ModelStatsArgs m) {
    __shared__ TileLds<M_STRICT, MS_TILE> S;
    const LoglikeArgs &a = m.a;
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int t0 = tile * MS_TILE, t1 = min(t0 + MS_TILE, a.Nx);
    int bin[1] = {t0 + tid};
    const bool valid = bin[0] < a.Nx;
    const int bi = min(bin[0], a.Nx - 1);
    const double xv[1] = {a.x[bi]};
    const double y = a.y[bi];
    double *pl = m.planes + bi;
    bool have = m.have_ref != 0;  // (workgroup-uniform, like everything that steers the loop below)
    double R = 0.0, A1 = 0.0, A2 = 0.0, mn = INFINITY, mx = -INFINITY, Q = 0.0, G = 0.0;
    if (have) {
        R = pl[MS_R * m.plane]; A1 = pl[MS_A1 * m.plane]; A2 = pl[MS_A2 * m.plane]; mn = pl[MS_MIN * m.plane];
        mx = pl[MS_MAX * m.plane]; Q = pl[MS_Q * m.plane]; G = pl[MS_G * m.plane];
    }
    const Probe probe(a, 0, tile);
    tamcmc_multiplet g;
    for (int b = 0; b < a.B; b++) {
        const double w = m.weights[b];
        if (m.status[b] != 0 || !(w > 0.0)) continue;  // skipped vectors: a failed table, a zero weight
        const SlotWords sw = slot_words(a, b);
        double acc[1] = {0.0};
        for (int c0 = sw.mbeg; c0 < sw.mend; c0 += CHUNK) {
            __syncthreads();  // previous chunk fully consumed
            const int n = stage_chunk<M_STRICT, MS_TILE>(a, t0, t1, 0.0, 0.0, S, g, c0, sw.mbeg, sw.mend, probe);
            const LdsMult *s_m = (const LdsMult *)S.buf;
            for (int q = 0; q < n; q++) {
                const LdsMult &M = s_m[q];
                switch (M.l) {  // wave-uniform
                case 0: mult_dispatch<false, 1, 1>(M, xv, bin, acc, 0.0); break;
                case 1: mult_dispatch<false, 3, 1>(M, xv, bin, acc, 0.0); break;
                case 2: mult_dispatch<false, 5, 1>(M, xv, bin, acc, 0.0); break;
                default: mult_dispatch<false, 7, 1>(M, xv, bin, acc, 0.0); break;
                }
            }
        }
        // harvey_like, the statements of the STRICT likelihood terms (loglike_tile.h); Bg: the same terms summed before the modes are added
        const double *nz = a.noise + (size_t)b * a.noise_stride;
        double Mv = acc[0], Bg = 0.0;
        for (int hh = 0; hh < sw.nh; hh++) {
            const double tau = nz[3 * hh + 1];
            if (tau != 0.0) {
                double t = pow((1e-3 * tau) * xv[0], nz[3 * hh + 2]);
                t = nz[3 * hh] * (1.0 / (t + 1.0));
                Mv = Mv + t;
                Bg = Bg + t;
            }
        }
        const double white = nz[sw.nn - 1];
        Mv = Mv + white;
        Bg = Bg + white;
        if (!have) { R = Mv; have = true; }
        const double d = Mv - R;
        A1 = A1 + w * d;
        A2 = A2 + w * (d * d);
        mn = Mv < mn ? Mv : mn;
        mx = Mv > mx ? Mv : mx;
        Q = Q + w * (y / Mv);
        G = G + w * Bg;
    }
    if (valid && have) {
        pl[MS_R * m.plane] = R; pl[MS_A1 * m.plane] = A1; pl[MS_A2 * m.plane] = A2; pl[MS_MIN * m.plane] = mn;
        pl[MS_MAX * m.plane] = mx; pl[MS_Q * m.plane] = Q; pl[MS_G * m.plane] = G;
    }
}

}  // namespace

hipError_t launch_model_stats(const ModelStatsArgs &m, hipStream_t st) {
    if (m.a.B <= 0) return hipSuccess;
    if (m.a.Nx < 1 || !m.weights || !m.status || !m.planes || m.plane < (size_t)m.a.Nx) return hipErrorInvalidValue;
    const int ntiles = (m.a.Nx + MS_TILE - 1) / MS_TILE;
    hipLaunchKernelGGL(k_model_stats, dim3(ntiles), dim3(MS_TILE), 0, st, m);
    return hipGetLastError();
}

}  // namespace tamcmc

// ---- the handle of include/tamcmc_hip.h ----
struct tamcmc_model_stats {
    tamcmc_hip_ctx *ctx = nullptr;
    int model_id = 0;
    bool rgb = false;
    int64_t Nparams = 0, Nx = 0;
    int chunk = 0;
    std::vector<double> inputs;       // [Nparams] the vector add_vars scatters into
    std::vector<int32_t> free_index;  // indices with relax = 1, in order
    bool has_relax = false;
    int32_t plength[11];
    tamcmc::DevBuf<double> d_planes, d_w;
    tamcmc::DevBuf<int32_t> d_st;
    tamcmc::PinBuf<double> h_w;
    tamcmc::PinBuf<int32_t> h_st;
    std::vector<double> rows;  // add_vars: the scattered vectors of one chunk
    double W = 0.0;
    int64_t counts[3] = {0, 0, 0};  // accepted, skipped: table failed, skipped: weight 0
};

namespace {

constexpr int MS_DEFAULT_CHUNK = 1024;

// One chunk of B <= 65535 vectors (rows of Nparams doubles, contiguous): tables, launch, then W and the counts in vector order.
int add_chunk(tamcmc_model_stats *ms, int B, const double *params, const double *weights) {
    using namespace tamcmc;
    tamcmc_hip_ctx *c = ms->ctx;
    const int Nx = (int)ms->Nx;
    HIPCHK(c, ms->h_w.reserve((size_t)B));
    HIPCHK(c, ms->h_st.reserve((size_t)B));
    HIPCHK(c, ms->d_w.reserve((size_t)B));
    HIPCHK(c, ms->d_st.reserve((size_t)B));
    HIPCHK(c, ms->d_planes.reserve((size_t)MS_PLANES * Nx));
    int32_t *status = ms->h_st.p;
    for (int b = 0; b < B; b++) ms->h_w.p[b] = weights ? weights[b] : 1.0;
    int per = 0, stride = 1, first_err = TAMCMC_OK, rot = 0;
    const int rc = ms->rgb ? rgb_stage_params(c, ms->model_id, B, params, ms->Nparams, ms->plength, status, &per, &stride, &first_err, &rot)
                           : stage_params_host(c, ms->model_id, B, params, ms->Nparams, ms->plength, status, &per, &stride, &first_err);
    if (rc) return rc;
    const StageLayout L(B, stride, (size_t)B * per);
    hipStream_t st = c->stream;
    if (!ms->rgb) {  // host-built tables: one upload; their status goes up beside the weights (red giants: the pre-step left both on the device)
        HIPCHK(c, c->d_stage.reserve(L.bytes));
        HIPCHK(c, hipMemcpyAsync(c->d_stage.p, c->h_stage.p, L.bytes, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(ms->d_st.p, status, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    HIPCHK(c, hipMemcpyAsync(ms->d_w.p, ms->h_w.p, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
    ModelStatsArgs m;
    LoglikeArgs &a = m.a;
    a.x = c->dx.p; a.y = c->dy.p; a.logx = c->dlogx.p; a.Nx = Nx; a.B = B; a.ntiles = (Nx + MS_TILE - 1) / MS_TILE;
    a.x0 = c->hx[0]; a.step = c->hx[1] - c->hx[0];
    a.mults = (const tamcmc_multiplet *)(c->d_stage.p + L.off_mults);
    a.offsets = (const int32_t *)(c->d_stage.p + L.off_pairs);
    a.noise = (const double *)(c->d_stage.p + L.off_noise);
    a.noise_stride = stride;
    a.nharvey = (const int32_t *)(c->d_stage.p + L.off_nh);
    a.nnoise = (const int32_t *)(c->d_stage.p + L.off_nn);
    a.partials = nullptr;
    a.model = nullptr;
    m.weights = ms->d_w.p;
    m.status = ms->rgb ? (const int32_t *)rgb_status_device(c, B) : ms->d_st.p;
    m.planes = ms->d_planes.p;
    m.plane = (size_t)Nx;
    m.have_ref = ms->counts[0] > 0 ? 1 : 0;
    HIPCHK(c, launch_model_stats(m, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (ms->rgb) rgb_collect_status(c, B, status, &first_err);
    for (int b = 0; b < B; b++) {
        const double w = ms->h_w.p[b];
        if (status[b] != TAMCMC_OK) ms->counts[1]++;
        else if (!(w > 0.0)) ms->counts[2]++;
        else { ms->W = ms->W + w; ms->counts[0]++; }
    }
    return TAMCMC_OK;
}

int add_checks(const tamcmc_model_stats *ms, int64_t n, const double *rows, int64_t row_stride, int64_t min_stride, const double *weights) {
    if (!ms || n < 0 || (n > 0 && !rows) || row_stride < min_stride) return TAMCMC_ERR_BAD_ARG;
    if (ms->ctx->Nx != ms->Nx) return TAMCMC_ERR_BAD_ARG;  // the spectrum was replaced by one of another length: the planes mean nothing
    if (weights)
        for (int64_t i = 0; i < n; i++)
            if (!(weights[i] >= 0.0) || !std::isfinite(weights[i])) return TAMCMC_ERR_BAD_ARG;
    return TAMCMC_OK;
}

}  // namespace

extern "C" {

int tamcmc_hip_model_stats_create(tamcmc_model_stats **out, tamcmc_hip_ctx *c, int model_id, const double *inputs, int64_t Nparams,
                                  const int32_t *relax, const int32_t *plength, int32_t chunk) {
    if (!out) return TAMCMC_ERR_BAD_ARG;
    *out = nullptr;
    if (!c || !inputs || !plength || Nparams < 1 || chunk < 0 || chunk > 65535) return TAMCMC_ERR_BAD_ARG;
    if (tamcmc::is_envelope_model(model_id)) return TAMCMC_ERR_BAD_MODEL;  // ids 0, 1: no mode table
    if (c->Nx <= 0) return TAMCMC_ERR_NO_SPECTRUM;
    const bool rgb = tamcmc::is_rgb_model(model_id);
    if (!rgb && tamcmc::count_multiplets(model_id, plength) < 0) return TAMCMC_ERR_BAD_MODEL;
    tamcmc_model_stats *ms = new tamcmc_model_stats();
    ms->ctx = c;
    ms->model_id = model_id;
    ms->rgb = rgb;
    ms->Nparams = Nparams;
    ms->Nx = c->Nx;
    ms->chunk = chunk ? chunk : MS_DEFAULT_CHUNK;
    ms->inputs.assign(inputs, inputs + Nparams);
    std::memcpy(ms->plength, plength, sizeof ms->plength);
    if (relax) {
        ms->has_relax = true;
        for (int64_t i = 0; i < Nparams; i++)
            if (relax[i] == 1) ms->free_index.push_back((int32_t)i);
    }
    *out = ms;
    return TAMCMC_OK;
}

int tamcmc_hip_model_stats_add_params(tamcmc_model_stats *ms, int64_t n, const double *params, int64_t row_stride, const double *weights) {
    if (int rc = add_checks(ms, n, params, row_stride, ms ? ms->Nparams : 0, weights)) return rc;
    tamcmc_hip_ctx *c = ms->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t Np = ms->Nparams;
    for (int64_t i0 = 0; i0 < n; i0 += ms->chunk) {
        const int B = (int)((n - i0 < ms->chunk) ? n - i0 : ms->chunk);
        const double *rows = params + i0 * row_stride;
        if (row_stride != Np) {  // the table stages take contiguous rows
            ms->rows.resize((size_t)B * Np);
            for (int b = 0; b < B; b++) std::memcpy(&ms->rows[(size_t)b * Np], rows + (int64_t)b * row_stride, (size_t)Np * sizeof(double));
            rows = ms->rows.data();
        }
        if (int rc = add_chunk(ms, B, rows, weights ? weights + i0 : nullptr)) return rc;
    }
    return TAMCMC_OK;
}

int tamcmc_hip_model_stats_add_vars(tamcmc_model_stats *ms, int64_t n, const double *vars, int64_t row_stride, const double *weights) {
    if (ms && !ms->has_relax) return TAMCMC_ERR_BAD_ARG;
    const int64_t Nv = ms ? (int64_t)ms->free_index.size() : 0;
    if (int rc = add_checks(ms, n, vars, row_stride, Nv, weights)) return rc;
    tamcmc_hip_ctx *c = ms->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t Np = ms->Nparams;
    for (int64_t i0 = 0; i0 < n; i0 += ms->chunk) {
        const int B = (int)((n - i0 < ms->chunk) ? n - i0 : ms->chunk);
        ms->rows.resize((size_t)B * Np);
        for (int b = 0; b < B; b++) {
            double *row = &ms->rows[(size_t)b * Np];
            std::memcpy(row, ms->inputs.data(), (size_t)Np * sizeof(double));
            const double *v = vars + (i0 + b) * row_stride;
            for (int64_t k = 0; k < Nv; k++) row[ms->free_index[(size_t)k]] = v[k];
        }
        if (int rc = add_chunk(ms, B, ms->rows.data(), weights ? weights + i0 : nullptr)) return rc;
    }
    return TAMCMC_OK;
}

int tamcmc_hip_model_stats_get(const tamcmc_model_stats *ms, double *W, int64_t counts[3], double *mean, double *var, double *mn, double *mx,
                               double *ratio, double *background) {
    if (!ms) return TAMCMC_ERR_BAD_ARG;
    if (ms->counts[0] <= 0 || ms->ctx->Nx != ms->Nx) return TAMCMC_ERR_BAD_ARG;
    tamcmc_hip_ctx *c = ms->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t Nx = (size_t)ms->Nx;
    if (W) *W = ms->W;
    if (counts)
        for (int i = 0; i < 3; i++) counts[i] = ms->counts[i];
    if (!(mean || var || mn || mx || ratio || background)) return TAMCMC_OK;
    std::vector<double> h((size_t)tamcmc::MS_PLANES * Nx);
    HIPCHK(c, hipMemcpyAsync(h.data(), ms->d_planes.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double Wt = ms->W;
    const double *R = &h[tamcmc::MS_R * Nx], *A1 = &h[tamcmc::MS_A1 * Nx], *A2 = &h[tamcmc::MS_A2 * Nx];
    for (size_t i = 0; i < Nx; i++) {
        if (mean) mean[i] = R[i] + A1[i] / Wt;
        if (var) {
            const double v = (A2[i] - A1[i] * A1[i] / Wt) / Wt;
            var[i] = v < 0.0 ? 0.0 : v;  // (a NaN stays a NaN)
        }
        if (mn) mn[i] = h[tamcmc::MS_MIN * Nx + i];
        if (mx) mx[i] = h[tamcmc::MS_MAX * Nx + i];
        if (ratio) ratio[i] = h[tamcmc::MS_Q * Nx + i] / Wt;
        if (background) background[i] = h[tamcmc::MS_G * Nx + i] / Wt;
    }
    return TAMCMC_OK;
}

int tamcmc_hip_model_stats_reset(tamcmc_model_stats *ms) {
    if (!ms) return TAMCMC_ERR_BAD_ARG;
    ms->W = 0.0;
    ms->counts[0] = ms->counts[1] = ms->counts[2] = 0;  // nothing accepted: the next launch starts its planes in registers
    return TAMCMC_OK;
}

void tamcmc_hip_model_stats_destroy(tamcmc_model_stats *ms) {
    if (!ms) return;
    (void)hipSetDevice(ms->ctx->device);
    if (ms->ctx->stream) (void)hipStreamSynchronize(ms->ctx->stream);
    delete ms;
}

}  // extern "C"
