// fisher.hip -- expected (Fisher) information of the chi^2(2p) likelihood (fisher.h): k_fisher_freeze, k_fisher_freeze_rgb, k_fisher_gram,
// k_fisher_fold and the two C entries tamcmc_hip_fisher / tamcmc_hip_weighted_gram.  No atomics in anything that reaches F (the red giants'
// form counters are integers beside it): the bins of a slab are added in bin order (four per matrix
// instruction), the slabs in slab order, so two calls give the same bits and a chain's F does not depend on the chains around it, on its
// place in the batch or on the number of passes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "envelope.h"
#include "fd_batch.h"
#include "fisher.h"
#include "fisher_rgb_rule.h"
#include "kernels.h"

namespace tamcmc {
namespace {

constexpr int FG_WG = 256;  // four waves
constexpr int FG_SB = 64;   // rows of a panel: four 16-row blocks, one per wave
constexpr int FG_KT = 32;   // bins staged at a time
// LDS row stride in doubles.  A fragment read is lane -> X[row = lane & 15][bin = k + (lane >> 4)] (ds_read_b64, banks (a / 4) % 64, conflicts
// counted inside each half of the wave): with a stride = 2 (mod 32) doubles the 16 rows x 2 bins of a half fall on 32 different bank pairs
constexpr int FG_LD = FG_KT + 2;
static_assert(FISHER_SLAB % FG_KT == 0, "a slab is a whole number of staged chunks");

typedef double v4d __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(128) k_fisher_freeze(tamcmc_multiplet *mults, const int *pairs, const int *status, int per, int E) {
    const int slot = blockIdx.x, c = slot / E, e = slot - c * E, base = c * E;
    if (e == 0 || status[slot] != TAMCMC_OK || status[base] != TAMCMC_OK) return;
    const int n = min(min(pairs[2 * slot + 1] - pairs[2 * slot], pairs[2 * base + 1] - pairs[2 * base]), per);
    tamcmc_multiplet *t = mults + pairs[2 * slot];
    const tamcmc_multiplet *b = mults + pairs[2 * base];
    for (int j = threadIdx.x; j < n; j += 128) {
        t[j].i0 = b[j].i0;
        t[j].i1 = b[j].i1;
    }
}

// Red giants: one workgroup per (chain c, variable k).  Lanes over the rows of the base table compare both perturbed tables with it
// (adj_rgb_row_matches; an LDS flag per side, every writer stores the same value, as k_fd_compare under FdArgs::hybrid), the rule of
// fisher_rgb_rule.h chooses the form, and the workgroup writes what the form asks for.  Only this workgroup writes the two perturbed
// slots; the base slot is read by every workgroup of the chain and written by none.
__global__ void __launch_bounds__(128) k_fisher_freeze_rgb(const FisherRgbArgs a) {
    const int c = blockIdx.x / a.N, k = blockIdx.x - c * a.N, tid = threadIdx.x, E = 2 * a.N + 1;
    const int sb = c * E, sp = sb + 1 + k, sm = sb + 1 + a.N + k;
    __shared__ int s_moved[2];
    const int n_b = a.pairs[2 * sb + 1] - a.pairs[2 * sb], n_p = a.pairs[2 * sp + 1] - a.pairs[2 * sp], n_m = a.pairs[2 * sm + 1] - a.pairs[2 * sm];
    const tamcmc_multiplet *tb = a.mults + a.pairs[2 * sb];
    tamcmc_multiplet *tp = a.mults + a.pairs[2 * sp], *tm = a.mults + a.pairs[2 * sm];
    const bool ok_b = a.status[sb] == TAMCMC_OK, ok_p = ok_b && a.status[sp] == TAMCMC_OK, ok_m = ok_b && a.status[sm] == TAMCMC_OK;
    const bool same_p = ok_p && n_p == n_b, same_m = ok_m && n_m == n_b;  // (uniform)
    const int n = min(n_b, a.per);
    if (tid < 2) s_moved[tid] = 0;
    __syncthreads();
    for (int j = tid; j < n; j += 128) {
        if (same_p && !adj_rgb_row_matches(tb, tp, n_b, j)) s_moved[0] = 1;
        if (same_m && !adj_rgb_row_matches(tb, tm, n_b, j)) s_moved[1] = 1;
    }
    __syncthreads();
    const int cls_p = !ok_p ? ADJ_RGB_FAILED : (same_p && !s_moved[0] ? ADJ_RGB_LINEARISABLE : ADJ_RGB_FALLBACK);
    const int cls_m = !ok_m ? ADJ_RGB_FAILED : (same_m && !s_moved[1] ? ADJ_RGB_LINEARISABLE : ADJ_RGB_FALLBACK);
    const FisherRgbChoice ch = fisher_rgb_choose(cls_p, cls_m);
    if (tid == 0) {
        const size_t CN = (size_t)a.C * a.N, o = (size_t)c * a.N + k;
        a.rh[o] = a.rh3[(size_t)ch.rh * CN + o];
        if (a.counts && ch.form != FISHER_RGB_FAILED) atomicAdd(&a.counts[ch.form - 1], 1ULL);
    }
    for (int j = tid; j < n; j += 128) {
        if (ch.freeze_plus) { tp[j].i0 = tb[j].i0; tp[j].i1 = tb[j].i1; }
        if (ch.freeze_minus) { tm[j].i0 = tb[j].i0; tm[j].i1 = tb[j].i1; }
    }
    if (ch.substitute != FISHER_RGB_SIDE_NONE) {
        // the side that does not correspond becomes the base table: rows as 8-byte words, then the noise row and the counts
        const int ss = ch.substitute == FISHER_RGB_SIDE_PLUS ? sp : sm;
        constexpr int NW = (int)(sizeof(tamcmc_multiplet) / 8);
        const unsigned long long *src = (const unsigned long long *)tb;
        unsigned long long *dst = (unsigned long long *)(ch.substitute == FISHER_RGB_SIDE_PLUS ? tp : tm);
        for (int w = tid; w < n * NW; w += 128) dst[w] = src[w];
        for (int i = tid; i < a.stride; i += 128) a.noise[(size_t)ss * a.stride + i] = a.noise[(size_t)sb * a.stride + i];
        if (tid == 0) {
            a.pairs[2 * ss + 1] = a.pairs[2 * ss] + n;
            a.nh[ss] = a.nh[sb];
            a.nn[ss] = a.nn[sb];
        }
    }
}

// Grid (slabs, panel pairs SI <= SJ, chains).  The workgroup stages FG_KT bins of panel SI (and of panel SJ when it is another one) in LDS
// as X (fisher.h), zeros beyond N and beyond the slab, and wave v accumulates the four 16x16 blocks (4 SI + v, 4 SJ + 0..3) that lie in the
// upper block triangle: D += A B with A = X[16 rows of SI][4 bins] w, B = X[16 rows of SJ][4 bins]^T, lane -> A[lane & 15][lane >> 4],
// B[lane >> 4][lane & 15].  Result lane map of the f64 form: column = lane & 15, row = (lane >> 4) + 4 reg.
__global__ void __launch_bounds__(FG_WG, 2) k_fisher_gram(const GramArgs g) {
    __shared__ double sI[FG_SB * FG_LD], sJ[FG_SB * FG_LD], sw[FG_KT], srh[2 * FG_SB];
    const int slab = blockIdx.x, c = blockIdx.z, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nsb = (g.NP + FG_SB - 1) / FG_SB;
    int SI = 0, rem = blockIdx.y;
    while (rem >= nsb - SI) { rem -= nsb - SI; SI++; }
    const int SJ = SI + rem;
    const bool two = SJ != SI;
    const long k_lo = (long)slab * FISHER_SLAB, k_hi = min(g.K, k_lo + FISHER_SLAB);
    const double *P = g.P + (size_t)c * g.set, *Mn = g.Mn ? g.Mn + (size_t)c * g.set : nullptr, *M0 = g.M0 ? g.M0 + (size_t)c * g.set : nullptr;
    // staging: this thread's bin of the chunk and its eight rows of each panel
    const int kk = tid & (FG_KT - 1), r0 = tid >> 5;
    if (tid < 2 * FG_SB) {  // 1 / h_applied of the two panels' rows (0 beyond N: those rows of X are zero)
        const int j = (tid < FG_SB ? SI : SJ) * FG_SB + (tid & (FG_SB - 1));
        srh[tid] = j < g.N ? (g.rh ? g.rh[(size_t)c * g.N + j] : 1.0) : 0.0;
    }
    const int gi = SI * 4 + wave;  // this wave's block row
    bool act[4];
#pragma unroll
    for (int bj = 0; bj < 4; bj++) act[bj] = gi <= SJ * 4 + bj && gi * 16 < g.NP && (SJ * 4 + bj) * 16 < g.NP;
    v4d acc[4];
#pragma unroll
    for (int bj = 0; bj < 4; bj++) acc[bj] = (v4d){0.0, 0.0, 0.0, 0.0};
    const double *pJ = two ? sJ : sI;
    __syncthreads();  // (srh is read by every wave in the staging below)
    for (long k0 = k_lo; k0 < k_hi; k0 += FG_KT) {
        const long i = k0 + kk;
        const bool in = i < k_hi;
        const long ic = in ? i : k_hi - 1;  // (a lane beyond the slab loads the slab's last bin and stores zero: every load is unconditional)
        // all loads of the chunk first -- rows beyond N read row N - 1 and are masked by srh = 0 --, then the division, then the products
        double vI[8], vJ[8], mI[8], mJ[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const size_t o = (size_t)min(SI * FG_SB + r0 + 8 * q, g.N - 1) * g.K + ic;
            vI[q] = P[o];
            mI[q] = Mn ? Mn[o] : 0.0;
        }
        if (two) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const size_t o = (size_t)min(SJ * FG_SB + r0 + 8 * q, g.N - 1) * g.K + ic;
                vJ[q] = P[o];
                mJ[q] = Mn ? Mn[o] : 0.0;
            }
        }
        const double s = in ? (M0 ? 1.0 / M0[ic] : 1.0) : 0.0;
        if (tid < FG_KT) sw[kk] = in ? (g.w ? g.w[i] : 1.0) : 0.0;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int r = r0 + 8 * q;
            // (a row beyond N has srh = 0, a bin beyond the slab `in` = false: the select keeps what was loaded for them out)
            sI[r * FG_LD + kk] = (in && srh[r] != 0.0) ? ((vI[q] - mI[q]) * srh[r]) * s : 0.0;
            if (two)
                sJ[r * FG_LD + kk] = (in && srh[FG_SB + r] != 0.0) ? ((vJ[q] - mJ[q]) * srh[FG_SB + r]) * s : 0.0;
        }
        __syncthreads();
#pragma unroll 2  // (unrolled eight times the fragment reads of all steps are hoisted and the kernel takes 254 registers)
        for (int ks = 0; ks < FG_KT / 4; ks++) {
            const int kq = ks * 4 + (lane >> 4);
            const double a = sI[(wave * 16 + (lane & 15)) * FG_LD + kq] * sw[kq];
#pragma unroll
            for (int bj = 0; bj < 4; bj++)
                if (act[bj]) {  // (wave-uniform)
                    const double b = pJ[(bj * 16 + (lane & 15)) * FG_LD + kq];
                    acc[bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[bj], 0, 0, 0);
                }
        }
        __syncthreads();
    }
    double *out = g.part + ((size_t)c * g.nslab + slab) * g.NP * g.NP;
#pragma unroll
    for (int bj = 0; bj < 4; bj++)
        if (act[bj]) {
            const int col = (SJ * 4 + bj) * 16 + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = gi * 16 + (lane >> 4) + 4 * reg;
                out[(size_t)row * g.NP + col] = acc[bj][reg];
            }
        }
}

// Grid (ceil(N N / 256), chains), one thread per element of the upper triangle: the slabs in slab order, times p, over T, both halves written.
__global__ void __launch_bounds__(256) k_fisher_fold(const GramArgs g) {
    const int c = blockIdx.y;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)g.N * g.N) return;
    const int j = (int)(e / g.N), k = (int)(e - (long)j * g.N);
    if (j > k) return;
    const double *p = g.part + (size_t)c * g.nslab * g.NP * g.NP + (size_t)j * g.NP + k;
    double s = 0.0;
    for (int q = 0; q < g.nslab; q++) s += p[(size_t)q * g.NP * g.NP];
    double v = (s * g.p) / (g.T ? g.T[c] : 1.0);
    if (g.status) {
        const int *st = g.status + (size_t)c * g.E;
        if (st[0] != TAMCMC_OK || st[1 + j] != TAMCMC_OK || st[1 + g.N + j] != TAMCMC_OK || st[1 + k] != TAMCMC_OK || st[1 + g.N + k] != TAMCMC_OK) v = NAN;
    }
    double *F = g.F + (size_t)c * g.N * g.N;
    F[(size_t)j * g.N + k] = v;
    F[(size_t)k * g.N + j] = v;
}

}  // namespace

hipError_t launch_fisher_freeze(tamcmc_multiplet *mults, const int *pairs, const int *status, int per, int C, int E, hipStream_t st) {
    if (C <= 0 || E <= 0 || per <= 0 || !mults || !pairs || !status) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fisher_freeze, dim3(C * E), dim3(128), 0, st, mults, pairs, status, per, E);
    return hipGetLastError();
}

hipError_t launch_fisher_freeze_rgb(const FisherRgbArgs &a, hipStream_t st) {
    if (a.C <= 0 || a.N <= 0 || (long)a.C * a.N > 0x7fffffffL || a.per <= 0 || a.stride <= 0 || !a.mults || !a.pairs || !a.nh || !a.nn || !a.noise ||
        !a.status || !a.rh3 || !a.rh)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fisher_freeze_rgb, dim3(a.C * a.N), dim3(128), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_fisher_gram(const GramArgs &g, hipStream_t st) {
    const int nsb = (g.NP + FG_SB - 1) / FG_SB;
    const long pairs = (long)nsb * (nsb + 1) / 2, fold = ((long)g.N * g.N + 255) / 256;
    if (g.C <= 0 || g.C > 65535 || g.N <= 0 || g.NP != fisher_padded(g.N) || g.K <= 0 || g.nslab != fisher_slabs(g.K) || pairs > 65535 ||
        fold > 0x7fffffffL || !g.P || !g.part || !g.F || (g.status && g.E != 2 * g.N + 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fisher_gram, dim3(g.nslab, (unsigned)pairs, g.C), dim3(FG_WG), 0, st, g);
    hipLaunchKernelGGL(k_fisher_fold, dim3((unsigned)fold, g.C), dim3(256), 0, st, g);
    return hipGetLastError();
}

}  // namespace tamcmc

using namespace tamcmc;

extern "C" {

int tamcmc_hip_fisher(tamcmc_hip_ctx *c, int model_id, int C, const double *params, int64_t Nparams, const int32_t *plength,
                      const int32_t *index_to_relax, int Nvars, const double *hstep, const double *Tcoefs, double p, double *F) {
    if (!c) return TAMCMC_ERR_BAD_ARG;
    const bool rgb = is_rgb_model(model_id);
    if (is_envelope_model(model_id) || (rgb && !c->rgb_fisher)) return TAMCMC_ERR_BAD_MODEL;  // (no table / red giants: TAMCMC_OPT_RGB_FISHER)
    int rc = check_gradient_args(c, C, params, Nparams, plength, index_to_relax, Nvars, hstep, F != nullptr, GA_PLENGTH | GA_VARS | GA_FISHER);
    if (rc) return rc;
    if (c->precision == TAMCMC_PRECISION_STRICT) return TAMCMC_ERR_BAD_ARG;  // (as the adjoint route)
    if (C == 0) return TAMCMC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    rc = ensure_poly(c);
    if (rc) return rc;
    const size_t Np = (size_t)Nparams, N = (size_t)Nvars, Nx = (size_t)c->Nx;
    const int NP = fisher_padded(Nvars), nslab = fisher_slabs((long)c->Nx);
    // (red giants: the chains of a pass also have to go through the pre-step workspace slice, 2 Nvars + 1 vectors each)
    int chunk = rgb ? fisher_rgb_chunk(C, Nvars, (long)c->Nx, (size_t)c->fisher_ws_mb, rgb_device_workspace_bytes(1), FD_RGB_WORKSPACE)
                    : fisher_chunk(C, Nvars, (long)c->Nx, (size_t)c->fisher_ws_mb);
    {  // launch limits of a pass: chains on a grid axis of k_fisher_gram, (slots x tiles) workgroups of the row launch
        const long tiles = ((long)c->Nx + tile_bins(c->wgs, c->K) - 1) / tile_bins(c->wgs, c->K) + 8;
        const long cap = 0x7fffffffL / (tiles * (2 * Nvars + 1));
        if (cap < 1) return TAMCMC_ERR_BAD_ARG;
        if (chunk > cap) chunk = (int)cap;
        if (chunk > 65535) chunk = 65535;
    }
    struct Events {  // (destroyed on every way out)
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (hipEvent_t v : e)
                if (v) (void)hipEventDestroy(v);
        }
        hipEvent_t &operator[](int i) { return e[i]; }
    } ev;
    if (c->timing) {
        HIPCHK(c, hipEventCreate(&ev[0]));
        HIPCHK(c, hipEventCreate(&ev[1]));
        c->fisher_ms[0] = c->fisher_ms[1] = c->fisher_ms[2] = 0.0;
        c->rgb_fisher_forms[0] = c->rgb_fisher_forms[1] = c->rgb_fisher_forms[2] = 0;
    }
    int first_err = TAMCMC_OK;
    std::vector<double> h2(2 * N);  // [+h, -h]
    std::vector<int32_t> idx2(2 * N);  // [index_to_relax, index_to_relax]
    for (size_t k = 0; k < N; k++) {
        h2[k] = hstep[k]; h2[N + k] = -hstep[k];
        idx2[k] = idx2[N + k] = index_to_relax[k];
    }
    auto pass = [&](int c0, int cp) -> int {
        FdBatch fb;
        int r = fb.layout(c, FdBatch::Request::Rows, model_id, 0, cp, Nparams, plength, 2 * Nvars);
        if (r) return r;
        FdInputs in;  // (Route::Rows: the doubled arrays h2, idx2)
        in.params = params + (size_t)c0 * Np; in.hstep = h2.data(); in.index_to_relax = idx2.data(); in.plength = plength;
        unsigned char *db;
        if ((r = fb.begin(c, in, &db))) return r;
        // 1 / h_applied (the difference of the two perturbed doubles as stored; the device adds the same doubles) and the temperatures
        const size_t n_rh = (size_t)cp * N, n_F = (size_t)cp * N * N, n_part = (size_t)cp * nslab * NP * NP;
        // (red giants: the three candidates behind them, 1 / (x+ - x0) and 1 / (x0 - x-); k_fisher_freeze_rgb chooses on the device)
        HIPCHK(c, c->h_S.reserve((rgb ? 3 : 1) * n_rh + cp));
        for (int ch = 0; ch < cp; ch++) {
            for (size_t k = 0; k < N; k++) {
                const double x0 = params[(size_t)(c0 + ch) * Np + index_to_relax[k]];
                volatile double xp = x0 + hstep[k], xm = x0 + (-hstep[k]);
                c->h_S.p[(size_t)ch * N + k] = 1.0 / (xp - xm);
                if (rgb) {
                    c->h_S.p[n_rh + cp + (size_t)ch * N + k] = 1.0 / (xp - x0);
                    c->h_S.p[2 * n_rh + cp + (size_t)ch * N + k] = 1.0 / (x0 - xm);
                }
            }
            c->h_S.p[n_rh + ch] = Tcoefs ? Tcoefs[c0 + ch] : 1.0;
        }
        HIPCHK(c, c->d_fisher.reserve(n_rh + cp + n_F + n_part));
        double *d_rh = c->d_fisher.p, *d_T = d_rh + n_rh, *d_F = d_T + cp, *d_part = d_F + n_F;
        if (!rgb) HIPCHK(c, hipMemcpyAsync(d_rh, c->h_S.p, (n_rh + cp) * 8, hipMemcpyHostToDevice, st));
        if (rgb) {  // the temperatures alone; candidates [central | plus | minus] into the block, the chosen reciprocals come back in its o_frh
            HIPCHK(c, hipMemcpyAsync(d_T, c->h_S.p + n_rh, (size_t)cp * 8, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(db + fb.o_frh3, c->h_S.p, n_rh * 8, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(db + fb.o_frh3 + n_rh * 8, c->h_S.p + n_rh + cp, 2 * n_rh * 8, hipMemcpyHostToDevice, st));
            d_rh = (double *)(db + fb.o_frh);
            if (c->timing) {
                fb.count_forms = true;
                HIPCHK(c, hipMemsetAsync(db + fb.o_fcount, 0, 24, st));
            }
        }
        if (c->timing) HIPCHK(c, hipEventRecord(ev[0], st));
        r = fb.enqueue(c, db, c->timing ? c->ev0 : nullptr, c->timing ? c->ev1 : nullptr);
        if (r) return r;
        GramArgs g;
        g.M0 = c->d_model.p; g.P = g.M0 + Nx; g.Mn = g.M0 + (1 + N) * Nx; g.rh = d_rh;
        g.set = (size_t)fb.E * Nx;
        g.C = cp; g.N = Nvars; g.NP = NP; g.nslab = nslab; g.K = (long)c->Nx;
        g.part = d_part; g.T = d_T; g.p = (double)(long)p; g.status = fb.head.results(db).status; g.E = fb.E; g.F = d_F;
        HIPCHK(c, launch_fisher_gram(g, st));
        if (c->timing) HIPCHK(c, hipEventRecord(ev[1], st));
        HIPCHK(c, hipMemcpyAsync(F + (size_t)c0 * N * N, d_F, n_F * 8, hipMemcpyDeviceToHost, st));
        unsigned long long forms[3] = {0, 0, 0};
        if (fb.count_forms) HIPCHK(c, hipMemcpyAsync(forms, db + fb.o_fcount, sizeof forms, hipMemcpyDeviceToHost, st));
        FdResults res;
        if ((r = fb.finish(c, &res))) return r;
        if (c->timing) {
            float ms[3] = {0, 0, 0};
            HIPCHK(c, hipEventElapsedTime(&ms[0], ev[0], c->ev0));
            HIPCHK(c, hipEventElapsedTime(&ms[1], c->ev0, c->ev1));
            HIPCHK(c, hipEventElapsedTime(&ms[2], c->ev1, ev[1]));
            for (int i = 0; i < 3; i++) c->fisher_ms[i] += ms[i];
            for (int i = 0; i < 3; i++) c->rgb_fisher_forms[i] += (int64_t)forms[i];
        }
        if (first_err == TAMCMC_OK) first_err = res.first_status();
        return TAMCMC_OK;
    };
    for (int c0 = 0; c0 < C && rc == TAMCMC_OK; c0 += chunk) rc = pass(c0, C - c0 < chunk ? C - c0 : chunk);
    return rc ? rc : first_err;
}

int tamcmc_hip_weighted_gram(tamcmc_hip_ctx *c, int N, int64_t K, const double *A, const double *w, double *G) {
    if (!c || N < 1 || N > 16384 || K < 1 || K > 0x7fffffffLL * FISHER_SLAB / 2 || !A || !G) return TAMCMC_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int NP = fisher_padded(N), nslab = fisher_slabs((long)K);
    const size_t n_A = (size_t)N * K, n_w = w ? (size_t)K : 0, n_G = (size_t)N * N, n_part = (size_t)nslab * NP * NP;
    HIPCHK(c, c->d_model.reserve(n_A));
    HIPCHK(c, c->d_fisher.reserve(n_w + n_G + n_part));
    double *d_w = c->d_fisher.p, *d_G = d_w + n_w, *d_part = d_G + n_G;
    HIPCHK(c, hipMemcpyAsync(c->d_model.p, A, n_A * 8, hipMemcpyHostToDevice, st));
    if (w) HIPCHK(c, hipMemcpyAsync(d_w, w, n_w * 8, hipMemcpyHostToDevice, st));
    GramArgs g;
    g.P = c->d_model.p; g.w = w ? d_w : nullptr;
    g.C = 1; g.N = N; g.NP = NP; g.nslab = nslab; g.K = (long)K;
    g.part = d_part; g.F = d_G;
    HIPCHK(c, launch_fisher_gram(g, st));
    HIPCHK(c, hipMemcpyAsync(G, d_G, n_G * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return TAMCMC_OK;
}

int tamcmc_hip_get_rgb_fisher_stats(tamcmc_hip_ctx *c, int64_t *central, int64_t *one_sided, int64_t *unfrozen) {
    if (!c) return TAMCMC_ERR_BAD_ARG;
    if (central) *central = c->rgb_fisher_forms[0];
    if (one_sided) *one_sided = c->rgb_fisher_forms[1];
    if (unfrozen) *unfrozen = c->rgb_fisher_forms[2];
    return TAMCMC_OK;
}

int tamcmc_hip_get_fisher_times(tamcmc_hip_ctx *c, double *tables_ms, double *rows_ms, double *gram_ms) {
    if (!c) return TAMCMC_ERR_BAD_ARG;
    if (tables_ms) *tables_ms = c->fisher_ms[0];
    if (rows_ms) *rows_ms = c->fisher_ms[1];
    if (gram_ms) *gram_ms = c->fisher_ms[2];
    return TAMCMC_OK;
}

}  // extern "C"
