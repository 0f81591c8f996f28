// envelope_row.h -- what the Gaussian-envelope models (ids 0 and 1) share between the batched evaluation (envelope.hip) and the
// device-resident sampler (dev_sampler.hip): the scalars formed once per parameter vector (EnvRow, env_row: one function for host and
// device), the tile geometry, and the device bodies of the two passes over the bins.  A kernel that evaluates a tile through these
// bodies gets the bits of k_env_ksi / k_env_eval: same statements, same reduction orders.
// Who owns what.  The xi pass's term and weight are env_ksi_term / env_ksi_weight, which env_ksi_chunk (k_env_ksi, k_env_step) and
// env_ksi_grad_chunk (k_env_ksi_grad) both sum.  The model of a bin still stands twice, in env_tile (k_env_eval, k_env_step) and in
// env_grad_tile (k_env_grad), each naming the other: a shared statement was measured and did not hold the parent's speed.  The tile
// and chunk bodies own their loops, their accumulators and the reduction (env_block_reduce); the kernels around them own grids and
// partial layouts.
#pragma once
#include <stdint.h>

#include <cmath>

#include "../../include/tamcmc_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TAMCMC_ENV_HD __host__ __device__ inline
#else
#define TAMCMC_ENV_HD inline
#endif

namespace tamcmc {

constexpr int EWG = 256;          // workgroup of both passes: four waves
constexpr int EK = 4;             // tile pass: bins per thread -> 1024-bin tiles
constexpr int EK1 = 16;           // xi pass: bins per thread -> 4096-bin chunks
constexpr int ETILE = EWG * EK;
constexpr int ECHUNK = EWG * EK1;
// The sampler's one-launch step (k_env_step) serves spectra up to this many bins.  Id 1: 32 768.  Id 0: every tile workgroup also walks
// the whole spectrum for the xi sums, and the step loses to the lockstep kernels from 7 tiles on (measured on the MI355X with 10 chains:
// 26.5 against 25.6 k iterations/s at 6 144 bins, 25.3 against 25.6 k at 7 168), so its limit is the measured crossover
constexpr int ENV_STEP_MAX_BINS = 32768;
constexpr int ENV_STEP_MAX_BINS_KSI = 6144;
constexpr int ENV_STEP_MAX_CHUNKS = (ENV_STEP_MAX_BINS_KSI + ECHUNK - 1) / ECHUNK;
TAMCMC_ENV_HD int env_step_max_bins(int model_id) {
    return model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN ? ENV_STEP_MAX_BINS_KSI : ENV_STEP_MAX_BINS;
}

// what is formed once per parameter vector (double, the reference's expressions)
struct EnvRow {
    double amp, numax, sig2;  // Gaussian: amp * exp((-0.5 (x - numax)^2) / sig2)       (id 0: amp * eta^2 first)
    double N0;                // white noise
    double H[2], lna[2], pw[2];  // id 1: H_k / (1 + exp(pw_k (lna_k + ln x))), lna_k = ln(1e-3 tc_k), term skipped when tc_k == 0
    double b[3], lnb[3], c[3], a2[3];  // id 0: (xi_k a_k^2 / b_k) / (1 + exp(c_k (ln x - ln b_k))), xi_k from the trapezoid sums
    int32_t hon[2];
    int32_t pad[2];
};

// EnvRow as the TAMCMC_ENVELOPE_ROW_N = 24 doubles of tamcmc_sampler.h (tamcmc_sampler_get_envelope_rows)
inline void env_row_as_doubles(const EnvRow &R, double *r) {
    r[0] = R.amp; r[1] = R.numax; r[2] = R.sig2; r[3] = R.N0;
    for (int k = 0; k < 2; k++) { r[4 + k] = R.H[k]; r[6 + k] = R.lna[k]; r[8 + k] = R.pw[k]; r[22 + k] = R.hon[k] ? 1.0 : 0.0; }
    for (int k = 0; k < 3; k++) { r[10 + k] = R.b[k]; r[13 + k] = R.lnb[k]; r[16 + k] = R.c[k]; r[19 + k] = R.a2[k]; }
}

// EnvRow of one vector: the scalar part of the model functions.  Host: libm's fabs / log / pow; device: the device library's.
TAMCMC_ENV_HD void env_row(int model_id, const double *p, EnvRow &R) {
    R = EnvRow{};
    if (model_id == TAMCMC_MODEL_HARVEY_GAUSSIAN) {
        R.amp = std::fabs(p[7]);
        R.numax = p[8];  // (not taken in absolute value by model_Harvey_Gaussian)
        R.sig2 = std::pow(std::fabs(p[9]), 2);
        for (int q = 0; q < 2; q++) {  // harvey_like(|params[0:7]|, ...): [H, tc, p] x 2, then B0
            const double H = std::fabs(p[3 * q]), tc = std::fabs(p[3 * q + 1]), pw = std::fabs(p[3 * q + 2]);
            R.hon[q] = (tc != 0) ? 1 : 0;
            R.H[q] = H;
            R.lna[q] = std::log((1e-3) * tc);
            R.pw[q] = pw;
        }
        R.N0 = std::fabs(p[6]);
        return;
    }
    // model_Kallinger2014_Gaussian + Kallinger2014(numax, mu_numax, params[0:14], ...)
    const double Amax = std::fabs(p[14]), numax = std::fabs(p[15]), sig = std::fabs(p[16]), mu_numax = p[17];
    R.amp = std::fabs(Amax);
    R.numax = numax;
    R.sig2 = std::pow(std::fabs(sig), 2);
    const double a0 = std::fabs(p[0] * std::pow(std::fabs(numax), p[1]));
    const double b0 = std::fabs(p[2] * std::pow(std::fabs(numax + mu_numax), p[3]));
    const double c0 = std::fabs(p[4]);
    const double a1 = p[5], a2 = p[6];
    const double b1 = std::fabs(p[7] * std::pow(std::fabs(numax + mu_numax), p[8]));
    const double b2 = std::fabs(p[10] * std::pow(std::fabs(numax + mu_numax), p[11]));
    const double c1 = std::fabs(p[9]), c2 = std::fabs(p[12]);
    R.N0 = std::fabs(p[13]);
    const double bb[3] = {b0, b1, b2}, cc[3] = {c0, c1, c2}, aa[3] = {a0, a1, a2};
    for (int k = 0; k < 3; k++) {
        R.b[k] = bb[k];
        R.lnb[k] = std::log(bb[k]);
        R.c[k] = cc[k];
        R.a2[k] = std::pow(aa[k], 2);
    }
}

// ---- analytic gradient of S = sum_i (y_i/M_i + ln M_i) (TAMCMC_OPT_ENVELOPE_GRADIENT; conventions in include/tamcmc_hip.h) ----
// The kernels sum r_i = 1/M_i - y_i/M_i^2 against what M's derivatives are made of, with L = 1/(1 + e^u), D = L (1 - L):
//   tile pass   [sum r G, sum r G d, sum r G d^2, sum r, sum r L_q (NQ), sum r D_q (NQ), sum r D_q u_q (NQ); id 0: sum r L_k^2 (3)]
//               G = g (id 1) / eta^2 g (id 0), d = x - numax; NQ = 2, u_q = lna_q + ln x (id 1); NQ = 3, u_q = ln x - ln b_q (id 0)
//   xi pass     (id 0) [sum w L_k, sum w D_k, sum w D_k u_k, sum w L_k^2] (3 each)
// A bin adds exactly 0 to the D and D u sums when D = 0 (a saturated term; a first bin at x = 0 is one) or when u is not finite.
// The sums of L^2 serve dS/dln b_k alone.  dM/dln b_k = C_k c_k L (Lbar - L), Lbar = sum w L^2 / sum w L: written with D it is
// c D - L I^b/I = c L ((1 - L) - (1 - Lbar)), which loses every digit where all of a spectrum's bins lie far above b_k (L << 1, a
// two-bin spectrum does it); written with L^2 it loses them where all lie far below (L close to 1).  The host takes the form whose
// terms are the smaller: L^2 where Lbar <= 1/2, D otherwise (env_grad_rows).
constexpr int ENV_GRAD_NRAW0 = 16, ENV_GRAD_NRAW1 = 10;  // tile sums of id 0 / id 1 (after S's own two)
constexpr int ENV_GRAD_NRAWMAX = 16;                     // stride of a vector's folded tile sums
constexpr int ENV_GRAD_NKRAW = 12;                       // xi sums of id 0 as the device leaves them
constexpr int ENV_GRAD_N = 13;                           // row quantities per vector: TAMCMC_ENVELOPE_GRAD_N
constexpr int ENV_GRAD_NKSI = 9;                         // xi sums per vector: TAMCMC_ENVELOPE_KSI_N
TAMCMC_ENV_HD int env_grad_nraw(int model_id) { return model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN ? ENV_GRAD_NRAW0 : ENV_GRAD_NRAW1; }

// Folded sums of one vector -> dS / d(row quantity), in the order of tamcmc_hip_envelope_gradient_sums:
//   id 1  [A, nu, sigma^2, N0, H_0, H_1, lna_0, lna_1, pw_0, pw_1, 0, 0, 0]
//   id 0  [A, nu (the Gaussian's), sigma^2, N0, a_k^2 (3), ln b_k (3), c_k (3)]
// and (id 0) the xi sums [I_k, I_k^b = c_k sum w D_k, I_k^c = -sum w D_k u_k] into ksi[9] (may be null).  h: the trapezoid step
// x(1) - x(0).  ONE text for the two arithmetics the chain rule runs in (as env_row is one text for host and device): T = long double
// on the host (the gradient entries, envelope.hip), T = double on the device (k_env_mala_chain, dev_mala_impl.h).
template <class T>
TAMCMC_ENV_HD void env_grad_rows(int model_id, const EnvRow &R, double h, const double *raw, const double *kraw, T *out, T *ksi) {
    for (int q = 0; q < ENV_GRAD_N; q++) out[q] = T(0);
    const T A = R.amp, s2 = R.sig2;
    out[0] = raw[0];
    out[1] = A * (T)raw[1] / s2;
    out[2] = A * (T)raw[2] / (T(2) * s2 * s2);
    out[3] = raw[3];
    if (model_id == TAMCMC_MODEL_HARVEY_GAUSSIAN) {
        for (int q = 0; q < 2; q++) {
            if (!R.hon[q]) continue;  // a switched-off term: 0 in its three places
            out[4 + q] = raw[4 + q];
            out[6 + q] = -(T)R.H[q] * (T)R.pw[q] * (T)raw[6 + q];
            out[8 + q] = -(T)R.H[q] * (T)raw[8 + q];
        }
        return;
    }
    for (int k = 0; k < 3; k++) {
        const T I = kraw[k], Ib = (T)R.c[k] * (T)kraw[3 + k], Ic = -(T)kraw[6 + k];
        const T hI = (T)h * I, Ck = (T)R.a2[k] / hI;
        const T rL = raw[4 + k], rD = raw[7 + k], rDu = raw[10 + k], rL2 = raw[13 + k];
        const T Kbar = (T)kraw[3 + k] / I, Lbar = (T)kraw[9 + k] / I;  // (Kbar + Lbar = 1)
        out[4 + k] = rL / hI;
        // the normalisation integral moves with b_k: c D - L I^b / I in whichever of its two forms keeps its digits ...
        out[7 + k] = Ck * (T)R.c[k] * (Lbar <= T(0.5) ? rL * Lbar - rL2 : rD - rL * Kbar);
        out[10 + k] = Ck * (-rDu - rL * Ic / I);                      // ... and with c_k
        if (ksi) { ksi[k] = I; ksi[3 + k] = Ib; ksi[6 + k] = Ic; }
    }
}

// d(row quantity) / d(parameter): J[q * Np + j], q in the order of env_grad_rows, j < Np = 10 (id 1) or 19 (id 0).  d|p|/dp =
// copysign(1, p); d ln(1e-3 |tc|)/dtc = 1/tc (not finite at tc = 0, where the model is not continuous).  T as for env_grad_rows.
template <class T>
TAMCMC_ENV_HD void env_row_jacobian(int model_id, const double *p, T *J) {
    const int Np = model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN ? 19 : 10;
    for (int i = 0; i < ENV_GRAD_N * Np; i++) J[i] = T(0);
    auto sgn = [](double v) { return (T)std::copysign(1.0, v); };
    auto at = [&](int q, int j) -> T & { return J[q * Np + j]; };
    if (model_id == TAMCMC_MODEL_HARVEY_GAUSSIAN) {
        at(0, 7) = sgn(p[7]);
        at(1, 8) = T(1);
        at(2, 9) = T(2) * (T)p[9];
        at(3, 6) = sgn(p[6]);
        for (int q = 0; q < 2; q++) {
            at(4 + q, 3 * q) = sgn(p[3 * q]);
            at(6 + q, 3 * q + 1) = T(1) / (T)p[3 * q + 1];
            at(8 + q, 3 * q + 2) = sgn(p[3 * q + 2]);
        }
        return;
    }
    const T s15 = sgn(p[15]), nu = std::fabs((T)p[15]), mu = p[17], nm = nu + mu, lnm = std::log(std::fabs(nm));
    at(0, 14) = sgn(p[14]);
    at(1, 15) = s15;
    at(2, 16) = T(2) * (T)p[16];
    at(3, 13) = sgn(p[13]);
    // a_0^2 = (p0 nu^p1)^2
    const T p0 = p[0], p1 = p[1], nup = std::pow(nu, T(2) * p1), a02 = p0 * p0 * nup;
    at(4, 0) = T(2) * p0 * nup;
    at(4, 1) = a02 * T(2) * std::log(nu);
    at(4, 15) = a02 * T(2) * p1 / nu * s15;
    at(5, 5) = T(2) * (T)p[5];
    at(6, 6) = T(2) * (T)p[6];
    // ln b_k = ln|p_i| + p_j ln|nu + mu|
    for (int k = 0; k < 3; k++) {
        const int bi = k == 0 ? 2 : k == 1 ? 7 : 10, bj = bi + 1, ci = bi + 2;
        const T pj = p[bj];
        at(7 + k, bi) = T(1) / (T)p[bi];
        at(7 + k, bj) = lnm;
        at(7 + k, 15) = pj / nm * s15;
        at(7 + k, 17) = pj / nm;
        at(10 + k, ci) = sgn(p[ci]);
    }
}

// dS / dtheta_j = sum_q dS/d(row quantity q) J[q][j], q ascending; a zero of the Jacobian adds nothing, so a parameter the model does
// not read (j >= NpJ, or a column of zeros) gives exactly +0.  T as for env_grad_rows.
template <class T>
TAMCMC_ENV_HD T env_chain_contract(const T *dS, const T *J, int NpJ, int j) {
    T s = T(0);
    if (j < NpJ)
        for (int q = 0; q < ENV_GRAD_N; q++) {
            const T Jq = J[q * NpJ + j];
            if (Jq != T(0)) s += dS[q] * Jq;
        }
    return s;
}

#if defined(__HIPCC__)

// t^p as the reference's pow(t, p) for t >= 0, from ln t: pow(t, 0) = 1 also at t = 0 (exp(0 * -inf) would be NaN)
__device__ __forceinline__ double pow_from_log(double p, double lt) { return p == 0.0 ? 1.0 : exp(p * lt); }

// Sums of a 256-thread workgroup: shuffle tree per wave, the four waves in order by thread 0, which alone gets the result.  Two calls
// that share s_red need a barrier between them.
template <int NV>
__device__ __forceinline__ void env_block_reduce(double (&v)[NV], double *s_red, double *out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; i++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[i] = v[i] + __shfl_down(v[i], off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; i++) s_red[wave * NV + i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; i++) {
            double s = s_red[i];
            for (int w = 1; w < EWG / 64; w++) s = s + s_red[w * NV + i];
            out[i] = s;
        }
    }
}

// L = 1 / (1 + t^c) at u = ln t, the xi pass's power-law term (env_ksi_term); e = t^c goes to a caller that wants the slope D too
__device__ __forceinline__ double env_logistic(double c, double u, double &e) {
    e = pow_from_log(c, u);
    return 1.0 / (e + 1.0);
}

// D = L (1 - L) with L = 1 / (1 + e): below e = 1 as L (e L), which has no cancellation where L is close to 1
__device__ __forceinline__ double env_logistic_slope(double L, double e) { return e < 1.0 ? L * (e * L) : L * (1.0 - L); }

// THE xi term of get_ksinorm's trapezoid sums (id 0) at bin i: L = 1 / (1 + (x_i/b)^c) with u = ln x_i - ln b, and its weight w = 1/2
// on the first and last bin of the spectrum.  env_ksi_chunk and env_ksi_grad_chunk both sum w L from here: the same bits.
__device__ __forceinline__ double env_ksi_weight(int i, int Nx) { return (i == 0 || i == Nx - 1) ? 0.5 : 1.0; }
__device__ __forceinline__ double env_ksi_term(double c, double lx, double lnb, double &u, double &e) {
    u = lx - lnb;
    return env_logistic(c, u, e);
}

// One chunk of get_ksinorm's three trapezoid sums (id 0): sum_i w_i L_i; thread 0 gets them in out[]
__device__ __forceinline__ void env_ksi_chunk(const double *logx, int Nx, int chunk, const EnvRow &R, double *s_red, double (&out)[3]) {
    const double lnb0 = R.lnb[0], lnb1 = R.lnb[1], lnb2 = R.lnb[2], c0 = R.c[0], c1 = R.c[1], c2 = R.c[2];
    double s[3] = {0.0, 0.0, 0.0};
    const int base = chunk * ECHUNK + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < EK1; k++) {
        const int i = base + k * EWG;
        if (i < Nx) {
            const double lx = logx[i], w = env_ksi_weight(i, Nx);
            double u, e;
            s[0] = s[0] + w * env_ksi_term(c0, lx, lnb0, u, e);
            s[1] = s[1] + w * env_ksi_term(c1, lx, lnb1, u, e);
            s[2] = s[2] + w * env_ksi_term(c2, lx, lnb2, u, e);
        }
    }
    env_block_reduce<3>(s, s_red, out);
}

// xi_k = b_k / (h * sum_k): get_ksinorm (noise_models.cpp:70-89), a vector's chunk partials summed in a fixed order; the three
// coefficients xi_k a_k^2 / b_k into s_coef.  Ends with a barrier.
__device__ __forceinline__ void env_ksi_coef(const double *ksi_part, int nchunk, double h, const EnvRow &R, double *s_red, double *s_coef) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int ch = threadIdx.x; ch < nchunk; ch += EWG) {
        const double *p = ksi_part + (size_t)ch * 3;
        s[0] = s[0] + p[0];
        s[1] = s[1] + p[1];
        s[2] = s[2] + p[2];
    }
    double out[3];
    env_block_reduce<3>(s, s_red, out);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double integral = out[k] * h;
            const double ksi = R.b[k] / integral;
            s_coef[k] = ksi * R.a2[k] / R.b[k];
        }
    }
    __syncthreads();
}

// The model of a bin is written twice, here and in env_grad_tile below: the two copies must stay equal statement for statement, for
// include/tamcmc_hip.h promises that the analytic route's logL0 is the evaluation's bit for bit.  One shared per-bin function was
// tried and measured: same bits, fewer instructions, but k_env_grad<1> came out 1 % slower at 10^6 bins and two
// more rows missed the parent's spread, so each body keeps its own statements.
// The model on one 1024-bin tile and the tile's sums of y/M and ln M (thread 0 gets them in out[]).  KIND: model id (0 Kallinger, 1
// Harvey); model_row (WRITE_MODEL): the vector's row of Nx model values
template <int KIND, bool WRITE_MODEL>
__device__ __forceinline__ void env_tile(const double *x, const double *y, const double *logx, int Nx, int tile, double xmax, const EnvRow &R,
                                         const double *s_coef, double *model_row, double *s_red, double (&out)[2]) {
    const double amp = R.amp, numax = R.numax, sig2 = R.sig2, N0 = R.N0;
    double acc[2] = {0.0, 0.0};
    const int base = tile * ETILE + threadIdx.x;
#pragma unroll
    for (int k = 0; k < EK; k++) {
        const int i = base + k * EWG;
        if (i < Nx) {
            const double xi = x[i], yi = y[i], lx = logx[i];
            const double d = xi - numax;
            const double g = exp((-0.5 * (d * d)) / sig2);
            double M;
            if (KIND == 0) {
                // eta^2 = sinc^2(pi x / (2 x_max)), 1 at a first bin x = 0 (eta_squared_Kallinger2014)
                double eta2 = 1.0;
                if (!(i == 0 && xi == 0.0)) {
                    const double a = 0.5 * M_PI * xi / xmax;  // ((0.5 pi) x) / x_max, the reference's grouping
                    const double sn = sin(a) / a;
                    eta2 = sn * sn;
                }
                M = (amp * eta2) * g;
                M = M + N0;  // Kallinger2014: Power = y + white noise, then the three super-Lorentzians, unfiltered (see tamcmc_hip.h)
#pragma unroll
                for (int q = 0; q < 3; q++) M = M + s_coef[q] * (1.0 / (pow_from_log(R.c[q], lx - R.lnb[q]) + 1.0));
            } else {
                M = amp * g;
#pragma unroll
                for (int q = 0; q < 2; q++)
                    if (R.hon[q]) M = M + R.H[q] * (1.0 / (pow_from_log(R.pw[q], R.lna[q] + lx) + 1.0));
                M = M + N0;
            }
            if (WRITE_MODEL) model_row[i] = M;
            acc[0] = acc[0] + yi / M;
            acc[1] = acc[1] + log(M);
        }
    }
    env_block_reduce<2>(acc, s_red, out);
}

// One chunk of the xi pass with the sums the gradient needs (id 0): per k the trapezoid sums of L_k (env_ksi_term, as env_ksi_chunk
// sums it), of D_k, of D_k (ln x - ln b_k) and of L_k^2; thread 0 gets them in out[]: [L (3), D (3), D u (3), L^2 (3)]
__device__ __forceinline__ void env_ksi_grad_chunk(const double *logx, int Nx, int chunk, const EnvRow &R, double *s_red, double (&out)[12]) {
    const double lnb[3] = {R.lnb[0], R.lnb[1], R.lnb[2]}, c[3] = {R.c[0], R.c[1], R.c[2]};
    double s[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int base = chunk * ECHUNK + threadIdx.x;
#pragma unroll 2
    for (int k = 0; k < EK1; k++) {
        const int i = base + k * EWG;
        if (i < Nx) {
            const double lx = logx[i], w = env_ksi_weight(i, Nx);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                double u, e;
                const double L = env_ksi_term(c[q], lx, lnb[q], u, e);
                s[q] = s[q] + w * L;
                s[9 + q] = s[9 + q] + w * (L * L);
                const double D = env_logistic_slope(L, e);
                if (D != 0.0 && isfinite(u)) {
                    s[3 + q] = s[3 + q] + w * D;
                    s[6 + q] = s[6 + q] + w * (D * u);
                }
            }
        }
    }
    env_block_reduce<12>(s, s_red, out);
}

// env_tile with the gradient's sums: M by env_tile's statements, kept equal to them by hand (see the note at env_tile; the two sums of
// S come out with the same bits), then r = (1 - y/M) / M
// against the pieces of dM; thread 0 gets [sum y/M, sum ln M, the tile sums listed above] in out[]
template <int KIND>
__device__ __forceinline__ void env_grad_tile(const double *x, const double *y, const double *logx, int Nx, int tile, double xmax, const EnvRow &R,
                                              const double *s_coef, double *s_red, double (&out)[2 + (KIND == 0 ? ENV_GRAD_NRAW0 : ENV_GRAD_NRAW1)]) {
    constexpr int NQ = KIND == 0 ? 3 : 2, NA = 2 + (KIND == 0 ? ENV_GRAD_NRAW0 : ENV_GRAD_NRAW1);
    const double amp = R.amp, numax = R.numax, sig2 = R.sig2, N0 = R.N0;
    double acc[NA];
#pragma unroll
    for (int j = 0; j < NA; j++) acc[j] = 0.0;
    const int base = tile * ETILE + threadIdx.x;
#pragma unroll
    for (int k = 0; k < EK; k++) {
        const int i = base + k * EWG;
        if (i < Nx) {
            const double xi = x[i], yi = y[i], lx = logx[i];
            const double d = xi - numax;
            const double g = exp((-0.5 * (d * d)) / sig2);
            double M, G = g, L[NQ], D[NQ], u[NQ];
            if (KIND == 0) {
                double eta2 = 1.0;
                if (!(i == 0 && xi == 0.0)) {
                    const double a = 0.5 * M_PI * xi / xmax;
                    const double sn = sin(a) / a;
                    eta2 = sn * sn;
                }
                G = eta2 * g;
                M = (amp * eta2) * g;
                M = M + N0;
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    u[q] = lx - R.lnb[q];
                    const double e = pow_from_log(R.c[q], u[q]);
                    L[q] = 1.0 / (e + 1.0);
                    D[q] = env_logistic_slope(L[q], e);
                    M = M + s_coef[q] * L[q];
                }
            } else {
                M = amp * g;
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    L[q] = 0.0; D[q] = 0.0; u[q] = 0.0;
                    if (R.hon[q]) {
                        u[q] = R.lna[q] + lx;
                        const double e = pow_from_log(R.pw[q], u[q]);
                        L[q] = 1.0 / (e + 1.0);
                        D[q] = env_logistic_slope(L[q], e);
                        M = M + R.H[q] * L[q];
                    }
                }
                M = M + N0;
            }
            const double t = yi / M;
            acc[0] = acc[0] + t;
            acc[1] = acc[1] + log(M);
            const double r = (1.0 - t) * (1.0 / M);
            const double rG = r * G;
            acc[2] = acc[2] + rG;
            acc[3] = acc[3] + rG * d;
            acc[4] = acc[4] + rG * (d * d);
            acc[5] = acc[5] + r;
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                acc[6 + q] = acc[6 + q] + r * L[q];
                if (KIND == 0) acc[6 + 3 * NQ + q] = acc[6 + 3 * NQ + q] + r * (L[q] * L[q]);
                if (D[q] != 0.0 && isfinite(u[q])) {
                    const double rD = r * D[q];
                    acc[6 + NQ + q] = acc[6 + NQ + q] + rD;
                    acc[6 + 2 * NQ + q] = acc[6 + 2 * NQ + q] + rD * u[q];
                }
            }
        }
    }
    env_block_reduce<NA>(acc, s_red, out);
}

#endif  // __HIPCC__

}  // namespace tamcmc
