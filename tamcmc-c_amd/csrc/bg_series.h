// bg_series.h -- Taylor series of the background (Harvey terms + white noise) on one tile of the likelihood kernel.
// H/(1+(a x)^p) with a = 1e-3 tau is analytic on a tile whose centre x_c is far from 0 (series_valid): with
// s = (x-x_c)/h,  u(s) = (a x_c)^p (1+eps s)^p  (binomial series, eps = h/x_c), then the reciprocal series of 1+u.
// The NH coefficients join the tile polynomial of the FAST far field (kernels.hip).  They depend on (evaluation, tile)
// only, so whoever builds an evaluation's table can build them once (dev_unpack.h, k_bg_poly) instead of every tile's
// workgroup; the arithmetic is this one function either way.   (noise_models.cpp:15-39 is the per-bin definition.)
#pragma once
#include <hip/hip_runtime.h>

namespace tamcmc {
namespace bg {

constexpr int NH = 8;             // Taylor coefficients of a Harvey term on a tile (x_c >> h)
constexpr double EPS_MAX = 0.02;  // ... used when eps = h/x_c <= EPS_MAX and the truncation of the steepest term fits SERIES_BUDGET:
// Truncation.  Deep in its decline (a x_c >> 1) a term is H (a x_c)^-p (1+eps s)^-p, the binomial series of a NEGATIVE power: its k-th
// coefficient is C(p+k-1,k) eps^k of the term, all of one sign at s = -1, so the NH = 8 kept coefficients leave
// C(p+7,8) eps^8 (1 + (p+8)/9 eps + ..) of the term (p = 2: 9 eps^8, p = 4: 330 eps^8, p = 8: 6435 eps^8; C(p,8) eps^8, the tail of
// u alone, is what this line claimed before and is 165 times less at p = 4).  For a x_c <~ 1 the term flattens and the tail shrinks.
// A tile takes the series when C(p_max+7,8) eps^8 <= SERIES_BUDGET, p_max the largest exponent among the evaluation's terms with
// tau != 0: every term then errs by <= 1.12 x 2e-13 of ITSELF (1.12 >= 1/(1 - (p+8)/9 eps): the tail beyond the 8th coefficient), the
// sum of the terms by <= 2.3e-13 M however many they are, which leaves three quarters of FAST's 1e-12 M to rounding.  eps <= 0.0194 at
// p = 2, 0.0137 at p = 4, 0.0086 at p = 8; a tile beyond it takes the per-bin exp/log path.  (tests/tile_series.py, test_tile_bounds.py)
constexpr double SERIES_BUDGET = 2e-13;

// v_rcp_f64 seed + two Newton-Raphson steps: ~1 ulp
__device__ __forceinline__ double rcp2(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    return fma(fma(-d, r, 1.0), r, r);
}

// centre and half-width of tile `tile` (tile_bins bins) on the regular grid x[i] = x0 + i*step
__device__ __forceinline__ void tile_geometry(int tile, int tile_bins, double x0, double step, double &xc, double &h) {
    const int t0 = tile * tile_bins;
    h = 0.5 * (double)tile_bins * step;
    xc = x0 + ((double)t0 + 0.5 * (double)tile_bins - 0.5) * step;
}
// largest exponent among the terms of a noise row that are switched on (0: none); a NaN exponent stays NaN and fails the gate
template <class NoiseAt>
__device__ __forceinline__ double max_exponent(NoiseAt nz, int nh) {
    double pm = 0.0;
    for (int t = 0; t < nh; t++) {
        const double pw = fabs(nz(3 * t + 2));
        if (nz(3 * t + 1) != 0.0 && !(pw <= pm)) pm = pw;
    }
    return pm;
}
// The gate of the series, in two parts: the tile's geometry alone, and with the steepest exponent.  A tile is series for all its users or
// for none: the three builders of prebuilt series (k_bg_poly in kernels.hip, dev_unpack.h, rgb_prestep.hip) apply the whole gate through
// prebuilt_series below; a tile workgroup (loglike_tile.h) that is handed a prebuilt series tests the geometry -- arithmetic on values it
// has, nothing to wait for -- and learns the exponent's verdict from the series itself (REFUSED); one that builds its own series applies
// the whole gate.
__device__ __forceinline__ bool series_geometry(double xc, double h) { return (fabs(h) <= EPS_MAX * fabs(xc)) && (xc > 0.0); }
// C(pmax+7, 8): once per evaluation
__device__ __forceinline__ double gate_coef(double pmax) {
    double c = pmax;
#pragma unroll
    for (int k = 1; k < NH; k++) c = c * ((pmax + (double)k) * (1.0 / (double)(k + 1)));
    return c;
}
// per tile: C eps^8 <= SERIES_BUDGET as C h^8 <= SERIES_BUDGET x_c^8 (x_c > 0: no division)
__device__ __forceinline__ bool series_valid(double xc, double h, double coef) {
    if (!series_geometry(xc, h)) return false;
    const double h2 = h * h, h4 = h2 * h2, x2 = xc * xc, x4 = x2 * x2;
    return coef * (h4 * h4) <= SERIES_BUDGET * (x4 * x4);  // (false for NaN)
}

// series of ONE term Hh/(1+(1e-3 tau x)^pw) about x_c; f[] = 0 when tau == 0 (noise_models.cpp:29)
__device__ __forceinline__ void harvey_term_series(double Hh, double tau, double pw, double xc, double h, double (&f)[NH]) {
#pragma unroll
    for (int k = 0; k < NH; k++) f[k] = 0.0;
    if (tau != 0.0) {
        const double eps = h / xc;
        double u[NH];
        u[0] = exp(pw * log(1e-3 * tau * xc));
#pragma unroll
        for (int k = 0; k < NH - 1; k++) u[k + 1] = u[k] * eps * (pw - (double)k) * (1.0 / (double)(k + 1));
        const double iv0 = rcp2(1.0 + u[0]);
        f[0] = Hh * iv0;
#pragma unroll
        for (int k = 1; k < NH; k++) {
            double acc2 = 0.0;
#pragma unroll
            for (int jj = 1; jj <= k; jj++) acc2 = fma(u[jj], f[k - jj], acc2);
            f[k] = -acc2 * iv0;
        }
    }
}

// all terms of one evaluation, summed in term order, + white noise (the LAST of the nn noise values)
template <class NoiseAt>
__device__ __forceinline__ void tile_series(NoiseAt nz, int nh, int nn, double xc, double h, double (&out)[NH]) {
#pragma unroll
    for (int k = 0; k < NH; k++) out[k] = 0.0;
    for (int t = 0; t < nh; t++) {
        double f[NH];
        harvey_term_series(nz(3 * t), nz(3 * t + 1), nz(3 * t + 2), xc, h, f);
#pragma unroll
        for (int k = 0; k < NH; k++) out[k] = out[k] + f[k];
    }
    out[0] = out[0] + nz(nn - 1);
}

// What a builder stores for one (evaluation, tile).  false: the geometry fails, nothing is stored (no tile looks).  Otherwise out[] is the
// series, or -- the geometry holds but the exponent's gate refuses -- NaN in every coefficient: the tile then takes the per-bin path.
__device__ __forceinline__ bool refused(double coef0) { return coef0 != coef0; }
template <class NoiseAt>
__device__ __forceinline__ bool prebuilt_series(NoiseAt nz, int nh, int nn, double xc, double h, double coef, double (&out)[NH]) {
    if (!series_geometry(xc, h)) return false;
    if (series_valid(xc, h, coef)) tile_series(nz, nh, nn, xc, h, out);
    else {
#pragma unroll
        for (int k = 0; k < NH; k++) out[k] = __builtin_nan("");
    }
    return true;
}

}  // namespace bg
}  // namespace tamcmc
