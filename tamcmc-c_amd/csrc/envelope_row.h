// envelope_row.h -- what the Gaussian-envelope models (ids 0 and 1) share between the batched evaluation (envelope.hip) and the
// device-resident sampler (dev_sampler.hip): the scalars formed once per parameter vector (EnvRow, env_row: one function for host and
// device), the tile geometry, and the device bodies of the two passes over the bins.  A kernel that evaluates a tile through these
// bodies gets the bits of k_env_ksi / k_env_eval: same statements, same reduction orders.
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

// One chunk of get_ksinorm's three trapezoid sums (id 0): sum_i w_i / (1 + (x_i/b_k)^c_k), w = 1/2 on the first and last bin of the
// spectrum; thread 0 gets them in out[]
__device__ __forceinline__ void env_ksi_chunk(const double *logx, int Nx, int chunk, const EnvRow &R, double *s_red, double (&out)[3]) {
    const double lnb0 = R.lnb[0], lnb1 = R.lnb[1], lnb2 = R.lnb[2], c0 = R.c[0], c1 = R.c[1], c2 = R.c[2];
    double s[3] = {0.0, 0.0, 0.0};
    const int base = chunk * ECHUNK + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < EK1; k++) {
        const int i = base + k * EWG;
        if (i < Nx) {
            const double lx = logx[i];
            const double w = (i == 0 || i == Nx - 1) ? 0.5 : 1.0;
            s[0] = s[0] + w * (1.0 / (1.0 + pow_from_log(c0, lx - lnb0)));
            s[1] = s[1] + w * (1.0 / (1.0 + pow_from_log(c1, lx - lnb1)));
            s[2] = s[2] + w * (1.0 / (1.0 + pow_from_log(c2, lx - lnb2)));
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

#endif  // __HIPCC__

}  // namespace tamcmc
