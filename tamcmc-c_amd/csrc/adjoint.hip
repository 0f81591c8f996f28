// adjoint.hip -- the three kernels of the adjoint gradient (adjoint.h): k_adj_rows, k_adj_noise (+ k_adj_fold, the ordered sum of their
// segments and tiles) and k_adj_contract.  No atomics: every sum has one fixed order (lane-strided bins, a wave64 __shfl_down tree, the waves in order
// through LDS, segments and tiles in order), so two calls give the same bits and a chain's result does not depend on the batch around it.
// (The one atomicAdd, in k_adj_contract, counts slots for the hybrid red-giant batch's statistics: integers, read by the host only.)
#include <hip/hip_runtime.h>

#include <cmath>

#include "adjoint.h"
#include "adj_rgb_match.h"

namespace tamcmc {
namespace {

constexpr int AB = 256;  // workgroup of k_adj_rows / k_adj_noise: four waves

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // (lane 0 holds the sum)
}

// v_rcp_f64 seed (2^-24.4) + one Newton-Raphson step: relative error <= 2.1e-15 (as the FAST likelihood tile's reciprocal)
__device__ __forceinline__ double rcp_nr1(double d) {
    const double r = __builtin_amdgcn_rcp(d);
    return fma(fma(-d, r, 1.0), r, r);
}

// One workgroup per (segment, table row, chain): the 17 sums of the row over segment s of its own window of the base table, bins
// [i0 + s ADJ_SEG, min(i1, i0 + (s + 1) ADJ_SEG)) -- counted from the row's i0, so what a chain's row adds up does not depend on anything
// outside the chain.  k_adj_fold adds the segments in order.
//   t = 2 (x - nu_m) / gamma, q = 1 + t^2, u = x / fc - 1, A = (1 + asym u)^2 + (gamma asym / (2 fc))^2 (A = 1, no derivative, when asym = 0)
//   dM/dhv_m = A / q                      dM/dnu_m = hv_m A (2 t / q^2) (2 / gamma)
//   dM/dgamma = sum_m hv_m [A 2 t^2 / (gamma q^2) + (gamma asym^2 / (2 fc^2)) / q]
//   dM/dasym  = sum_m (hv_m / q) [2 (1 + asym u) u + 2 (gamma / (2 fc))^2 asym]
//   dM/dfc    = sum_m (hv_m / q) [-2 (1 + asym u) asym x / fc^2 - gamma^2 asym^2 / (2 fc^3)]
// The row is workgroup-uniform (scalar registers); a lane keeps its 17 running sums in registers (the component loop is unrolled and
// predicated on the uniform 2l+1, so no accumulator is indexed dynamically).  One reciprocal (seed + Newton step) per component and bin;
// the sum over m of dM/dnu_m and dM/dhv_m leaves out the factors that do not depend on the bin's component (applied once at the end).
__global__ void __launch_bounds__(AB) k_adj_rows(const AdjArgs a) {
    __shared__ double s_w[AB / 64][ADJ_F];
    const int seg = blockIdx.x, row = blockIdx.y, c = blockIdx.z, tid = threadIdx.x, slot = c * a.E;
    const int n = a.pairs[2 * slot + 1] - a.pairs[2 * slot];
    if (row >= n || a.status[slot] != TAMCMC_OK) return;  // (no such row / a table that failed: k_adj_fold writes zeros)
    const tamcmc_multiplet &r = a.mults[(size_t)slot * a.per + row];
    const int w0 = max(r.i0, 0), w1 = min(r.i1, a.Nx);
    const int i0 = w0 + seg * ADJ_SEG, i1 = min(w1, i0 + ADJ_SEG);
    if (seg >= a.nseg || i0 >= i1) return;                // (beyond the row's window)
    const int nc = 2 * min(max(r.l, 0), 3) + 1;
    const double gamma = r.gamma, asym = r.asym, fc = r.fc;
    const bool asy = asym != 0.0;
    const double two_g = 2.0 / gamma, inv_fc = asy ? 1.0 / fc : 0.0;
    const double hgc = 0.5 * gamma * inv_fc;                 // gamma / (2 fc)
    const double c2sq = (hgc * asym) * (hgc * asym);         // (gamma asym / (2 fc))^2
    const double dA_dg = 0.5 * gamma * asym * asym * inv_fc * inv_fc;
    const double dA_da0 = 2.0 * hgc * hgc * asym;
    const double dA_dc0 = -0.5 * gamma * gamma * asym * asym * inv_fc * inv_fc * inv_fc;
    const double m2a = -2.0 * asym * inv_fc * inv_fc;
    double acc[ADJ_F];
#pragma unroll
    for (int f = 0; f < ADJ_F; f++) acc[f] = 0.0;
    const double *p0 = a.planes + (size_t)c * a.Nx, *p1 = p0 + a.plane;
    for (int i = i0 + tid; i < i1; i += AB) {
        const double x = a.x[i];
        const double ri = p0[i] * (1.0 - p1[i]);
        double u = 0.0, a1 = 1.0, A = 1.0;
        if (asy) {
            u = fma(x, inv_fc, -1.0);
            a1 = fma(asym, u, 1.0);
            A = fma(a1, a1, c2sq);
        }
        const double rA = ri * A;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int m = 0; m < 7; m++)
            if (m < nc) {
                const double t = (x - r.nu[m]) * two_g;
                const double iq = rcp_nr1(fma(t, t, 1.0));
                const double tiq = t * iq, h = r.hv[m];
                acc[7 + m] = fma(rA, iq, acc[7 + m]);        // r A / q
                acc[m] = fma(rA * tiq, iq, acc[m]);          // r A t / q^2        (x 2 hv_m 2/gamma below)
                s1 = fma(h, iq, s1);
                s2 = fma(h * tiq, tiq, s2);
            }
        acc[14] = fma(ri, fma(A * two_g, s2, dA_dg * s1), acc[14]);
        if (asy) {
            const double rs = ri * s1;
            acc[15] = fma(rs, fma(2.0 * a1, u, dA_da0), acc[15]);
            acc[16] = fma(rs, fma(m2a * a1, x, dA_dc0), acc[16]);
        }
    }
#pragma unroll
    for (int m = 0; m < 7; m++) acc[m] *= 2.0 * two_g * r.hv[m];
#pragma unroll
    for (int f = 0; f < ADJ_F; f++) {
        const double v = wave_sum(acc[f]);
        if ((tid & 63) == 0) s_w[tid >> 6][f] = v;
    }
    __syncthreads();
    double *out = a.Gpart + (((size_t)c * a.per + row) * a.nseg + seg) * ADJ_F;
    if (tid < ADJ_F) out[tid] = ((s_w[0][tid] + s_w[1][tid]) + s_w[2][tid]) + s_w[3][tid];
}

// Grid (tiles of ADJ_NTILE bins, chains): the tile's share of sum_i r_i dN_i/d|noise_j| for the base noise row [H, tau, p] x nharvey, N0.
// With z = exp(p (ln(1e-3 tau) + ln x)): d/dH = 1/(1+z), d/dtau = -H p z / (tau (1+z)^2), d/dp = -H z ln(1e-3 tau x) / (1+z)^2, d/dN0 = 1;
// a term with tau = 0 is skipped, as in the model.  One Harvey term at a time, so a lane holds three sums whatever nharvey is.
__global__ void __launch_bounds__(AB) k_adj_noise(const AdjArgs a) {
    __shared__ double s_w[AB / 64][3], s_out[3 * 16 + 4];
    const int tile = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, slot = c * a.E;
    const int stride = a.stride;
    const double *nz = a.noise + (size_t)slot * stride;
    const int nn = min(a.nn[slot], stride), nh = min(a.nh[slot], nn > 0 ? (nn - 1) / 3 : 0);
    const bool ok = a.status[slot] == TAMCMC_OK && nn > 0;
    for (int j = tid; j < stride; j += AB) s_out[j] = 0.0;
    const int b0 = tile * ADJ_NTILE, b1 = min(b0 + ADJ_NTILE, a.Nx);
    const double *p0 = a.planes + (size_t)c * a.Nx, *p1 = p0 + a.plane;
    auto wg3 = [&](double v0, double v1, double v2, int j, int cnt) {  // waves in order; lane 0 of the workgroup writes s_out[j .. j+cnt)
        v0 = wave_sum(v0); v1 = wave_sum(v1); v2 = wave_sum(v2);
        __syncthreads();
        if ((tid & 63) == 0) { s_w[tid >> 6][0] = v0; s_w[tid >> 6][1] = v1; s_w[tid >> 6][2] = v2; }
        __syncthreads();
        if (tid < cnt) s_out[j + tid] = ((s_w[0][tid] + s_w[1][tid]) + s_w[2][tid]) + s_w[3][tid];
    };
    if (ok) {
        for (int h = 0; h < nh; h++) {
            const double H = nz[3 * h], tau = nz[3 * h + 1], p = nz[3 * h + 2];
            if (tau == 0.0) continue;  // (uniform)
            const double lt = log(1e-3 * tau);
            double gH = 0.0, gT = 0.0, gP = 0.0;
            for (int i = b0 + tid; i < b1; i += AB) {
                const double ri = p0[i] * (1.0 - p1[i]);
                const double la = lt + a.logx[i];
                const double z = exp(p * la);
                const double w = 1.0 / (1.0 + z);
                const double zw2 = ri * (H * z * (w * w));
                gH += ri * w;
                gT -= zw2 * p / tau;
                gP -= zw2 * la;
            }
            wg3(gH, gT, gP, 3 * h, 3);
        }
        double g0 = 0.0;
        for (int i = b0 + tid; i < b1; i += AB) g0 += p0[i] * (1.0 - p1[i]);
        wg3(g0, 0.0, 0.0, nn - 1, 1);
    }
    __syncthreads();
    double *out = a.npart + ((size_t)c * a.ntn + tile) * stride;
    for (int j = tid; j < stride; j += AB) out[j] = s_out[j];
}

// The ordered second stage, one workgroup per chain: Gn[c][j] = the tiles' partials in tile order (as k_finalize sums the likelihood's
// tiles), G[c][row][f] = the row's segments in segment order (zeros for a row the table does not have or a table that failed).
__global__ void __launch_bounds__(AB) k_adj_fold(const AdjArgs a) {
    const int c = blockIdx.x, slot = c * a.E;
    for (int j = threadIdx.x; j < a.stride; j += AB) {
        double s = 0.0;
        for (int t = 0; t < a.ntn; t++) s += a.npart[((size_t)c * a.ntn + t) * a.stride + j];
        a.Gn[(size_t)c * a.stride + j] = s;
    }
    const int n = a.status[slot] == TAMCMC_OK ? a.pairs[2 * slot + 1] - a.pairs[2 * slot] : 0;
    for (int k = threadIdx.x; k < a.per * ADJ_F; k += AB) {
        const int row = k / ADJ_F, f = k - row * ADJ_F;
        double s = 0.0;
        if (row < n) {
            const tamcmc_multiplet &r = a.mults[(size_t)slot * a.per + row];
            const int len = min(r.i1, a.Nx) - max(r.i0, 0);
            const int ns = len > 0 ? min((len + ADJ_SEG - 1) / ADJ_SEG, a.nseg) : 0;
            const double *gp = a.Gpart + ((size_t)c * a.per + row) * a.nseg * ADJ_F + f;
            for (int q = 0; q < ns; q++) s += gp[(size_t)q * ADJ_F];
        }
        a.G[((size_t)c * a.per + row) * ADJ_F + f] = s;
    }
}

// One wave per slot (chain c, evaluation k): the first-order change of S from the base table to the slot's table.  Lane j takes rows j, j + 64, ...
// (fields in declaration order), the wave's tree adds the lanes, lane 0 adds the noise entries in order.  The windows of the slot's table are
// not read: frozen window.
__global__ void __launch_bounds__(64) k_adj_contract(const AdjArgs a, double *dS) {
    const int slot = blockIdx.x, c = slot / a.E, k = slot - c * a.E, base = c * a.E, lane = threadIdx.x;
    if (k == 0) {
        if (lane == 0) dS[slot] = 0.0;
        return;
    }
    if (a.status[slot] != TAMCMC_OK || a.status[base] != TAMCMC_OK) {
        if (lane == 0) dS[slot] = NAN;
        return;
    }
    if (a.cls) {
        const bool lin = a.cls[slot] & ADJ_RGB_FLAG_LINEAR;
        if (a.counts && lane == 0) atomicAdd(&a.counts[lin ? 0 : 1], 1ull);  // (integers: the order does not matter)
        if (!lin) {  // red giants, a fallback slot: the DELTA launch's difference, as it is
            if (lane == 0) dS[slot] = a.fall[slot];
            return;
        }
    }
    const int n = min(a.pairs[2 * base + 1] - a.pairs[2 * base], a.per);
    const tamcmc_multiplet *Te = a.mults + (size_t)slot * a.per, *T0 = a.mults + (size_t)base * a.per;
    double s = 0.0;
    for (int row = lane; row < n; row += 64) {
        const double *g = a.G + ((size_t)c * a.per + row) * ADJ_F;
        const tamcmc_multiplet &e = Te[row], &b = T0[row];
        const int nc = 2 * min(max(b.l, 0), 3) + 1;
        double v = 0.0;
        for (int m = 0; m < nc; m++) v += g[m] * (e.nu[m] - b.nu[m]);
        for (int m = 0; m < nc; m++) v += g[7 + m] * (e.hv[m] - b.hv[m]);
        v += g[14] * (e.gamma - b.gamma);
        if (b.asym != 0.0) {  // (asym = 0 at the base point: A = 1, no derivative)
            v += g[15] * (e.asym - b.asym);
            v += g[16] * (e.fc - b.fc);
        }
        s += v;
    }
    s = wave_sum(s);
    if (lane == 0) {
        const int nn = min(a.nn[base], a.stride);
        const double *ne = a.noise + (size_t)slot * a.stride, *n0 = a.noise + (size_t)base * a.stride, *gn = a.Gn + (size_t)c * a.stride;
        for (int j = 0; j < nn; j++) s += gn[j] * (ne[j] - n0[j]);
        dS[slot] = s;
    }
}

}  // namespace

hipError_t launch_adjoint(const AdjArgs &a, hipStream_t st, hipEvent_t *ev) {
    if (a.C <= 0 || a.C > 65535 || a.per <= 0 || a.per > 65535 || a.stride <= 0 || a.stride > 3 * 16 + 4 || a.ntn <= 0 || a.nseg <= 0 || !a.G ||
        !a.Gpart || !a.Gn || !a.npart || !a.planes)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_adj_rows, dim3(a.nseg, a.per, a.C), dim3(AB), 0, st, a);
    if (ev && hipEventRecord(ev[0], st) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_adj_noise, dim3(a.ntn, a.C), dim3(AB), 0, st, a);
    hipLaunchKernelGGL(k_adj_fold, dim3(a.C), dim3(AB), 0, st, a);
    if (ev && hipEventRecord(ev[1], st) != hipSuccess) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_adjoint_contract(const AdjArgs &a, double *dS, hipStream_t st) {
    if (a.C <= 0 || a.E <= 0 || !dS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_adj_contract, dim3(a.C * a.E), dim3(64), 0, st, a, dS);
    return hipGetLastError();
}

}  // namespace tamcmc
