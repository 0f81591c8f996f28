// loglike_tile.h -- the tile body of the likelihood kernel, as a device function shared by k_loglike (kernels.hip) and the fused sampler
// step (dev_sampler.hip): one workgroup = one tile of WGS*K consecutive bins of ONE evaluation.  Here: the arithmetic modes and the
// per-bin bodies (strict_mult, fast_mult), the definition of the FAST far field (also k_fd_far's, kernels.hip), the phases of a tile
// (tile_compute) and the workgroup -> (tile, evaluation) mapping (loglike_tile).  kernels.hip has the kernels and the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "bg_series.h"

namespace tamcmc {
namespace tile {

constexpr int CHUNK = 64;  // multiplets staged per pass: one wave compacts one chunk

constexpr int F_FULL = 1;  // window covers every bin of the tile
constexpr int F_SAFE = 2;  // FAST: product of the 2l+1 denominators stays far below DBL_MAX on this tile
constexpr int F_ASYM = 4;  // asymmetry coefficient != 0
constexpr int F_FAR = 8;   // FAST far field: the multiplet joins the tile polynomial instead of the per-bin loop

// arithmetic modes of k_loglike (see include/tamcmc_hip.h)
constexpr int M_STRICT = 0, M_FAST_DIRECT = 2, M_FAST = 1;

// FAST far field: a multiplet whose window covers the whole tile and whose components all sit at least 1/RHO_MAX tile
// half-widths away from the tile centre is an analytic function of x on the tile; the sum of ALL such multiplets is ONE
// polynomial of degree NC-1 in s = (x - x_c)/h, evaluated per bin by Horner (NC-1 fma) instead of ~6 ops per component.
// Component: hv/(1+(beta s - A)^2) = sum_k c_k s^k, c_k = -hv Im(u q^k), u = 1/(A+i), q = beta u, |q| = rho, with the
// three-term recurrence c_{k+1} = 2 Re(q) c_k - |q|^2 c_{k-1}.
// Truncation.  Deep in the wing (A >> 1) the component is hv / (A^2 (1 - rho s)^2), a DOUBLE pole with c_k ~ (k+1) rho^k: after n
// coefficients the series lacks tau(rho, n) = rho^n (n + 1 + n rho) of the far term (at s = -1, the end of the tile away from the
// mode; n + 1 - n rho at s = +1), and for smaller A no more.  At the gate: tau_far = tau(1/6, 16) = 6.96e-12 of the far term -- which
// may be all of M on a tile in the wing of one tall, broad mode -- not the simple pole's rho^NC / (1 - rho) = 4e-13 this line quoted
// before.  FAST states |dM| <= 1e-12 M + tau_far F per bin, F the sum of the far components (include/tamcmc_hip.h); logL keeps 1e-11.
// The gate is not tightened: rho <= 1/7 would move about a sixth more components into the per-bin loop (estimated at C3, not measured).
// The early stop of far_coefs keeps every shorter loop inside tau_far: tau(sqrt(1.39e-2), 14) = 1.7e-12 .. tau(sqrt(4.6e-5), 6) = 6.9e-13.
// tests/test_tile_bounds.py pins NC, both radii and the early-stop table against a 50-digit reference.
constexpr int NC = 16;
constexpr double RHO_MAX2 = 1.0 / 36.0;  // rho <= 1/6 -> truncation <= tau_far = 6.96e-12 of the far term
constexpr double RHO_MAX2_ASYM = 1.0 / 64.0;  // asymmetric profiles: the far wing can dominate M and the quadratic factor feeds degree >= NC
                                              // terms back -> rho <= 1/8: truncation tau(1/8, 16) = 6.8e-14 of the term; where the factor
                                              // comes close to zero on the tile the coefficients' rounding counts more, measured
                                              // 6.9e-13 of the term at worst (3.6e-15 at A = 0); stated tau_asym = 2.8e-12
constexpr int NH = bg::NH;               // Taylor coefficients of the background on a tile (bg_series.h)
constexpr int ROW = NC + 2;  // LDS row stride of the coefficient reduction (16-byte aligned, conflict-free b128 writes)

// Timing instrumentation exists in the probe build only (-DTAMCMC_PROBE, tools/): the product library has no code path that can
// skip a phase or return a wrong log-likelihood.  stamp(k): phase stamps 0..6 of one workgroup; skip(bit): a.probe's phase-skip mask.
#ifdef TAMCMC_PROBE
struct Probe {
    const LoglikeArgs &a;
    const bool stamps;  // lane 0 of the middle tile of evaluation 0
    const long wg_t0;   // per-workgroup timeline
    __device__ __forceinline__ Probe(const LoglikeArgs &a_, int b, int tile)
        : a(a_), stamps(a_.dbg && b == 0 && tile == a_.ntiles / 2 && threadIdx.x == 0), wg_t0((a_.dbg && a_.dbg[7] == 77) ? (long)wall_clock64() : 0) {}
    __device__ __forceinline__ void stamp(int k) const { if (stamps) a.dbg[k] = (long)wall_clock64(); }
    __device__ __forceinline__ bool skip(int bit) const { return a.probe & bit; }
    __device__ __forceinline__ void timeline(int b, int tile) const {
        if (a.dbg && a.dbg[7] == 77 && threadIdx.x == 0) {
            long *w = a.dbg + 8 + 2 * ((size_t)b * a.ntiles + tile);
            w[0] = wg_t0;
            w[1] = (long)wall_clock64();
        }
    }
};
#else
struct Probe {
    __device__ __forceinline__ Probe(const LoglikeArgs &, int, int) {}
    __device__ __forceinline__ void stamp(int) const {}
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ void timeline(int, int) const {}
};
#endif

// LDS image of a multiplet (160 B, every field group 16-byte aligned for ds_read_b128).
struct __attribute__((aligned(16))) LdsMult {
    int i0, i1, l, flags;
    double g;     // STRICT: gamma^2          FAST: 2/gamma
    double asym;  // asymmetry coefficient
    double c2sq;  // (0.5*gamma*asym/fc)^2
    double fcx;   // STRICT: nu_c             FAST: asym/nu_c
    double2 nh[7];  // STRICT: {nu_nlm, H*V_m}   FAST: {A_m = (nu_nlm - x_c) 2/gamma, H*V_m}  (x_c = centre of the nominal tile)
};

// v_rcp_f64 seed (2^-24.4) + ONE Newton-Raphson step: relative error <= 2.1e-15
__device__ __forceinline__ double rcp_nr1(double d) {
    double r = __builtin_amdgcn_rcp(d);
    return fma(fma(-d, r, 1.0), r, r);
}
// two steps: ~1 ulp
__device__ __forceinline__ double rcp_nr2(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    return fma(fma(-d, r, 1.0), r, r);
}

template <int NV, int WGS = 256>
__device__ __forceinline__ void block_reduce(double (&v)[NV], double *s_red, double *out) {
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
            for (int w = 1; w < WGS / 64; w++) s = s + s_red[w * NV + i];
            out[i] = s;
        }
    }
}

// ---- STRICT: the reference's statement sequence per bin, one IEEE operation per statement ----
template <int NM, int K, bool FULL>
__device__ __forceinline__ void strict_mult(const LdsMult &M, const double (&xv)[K], const int (&bin)[K], double (&acc)[K]) {
    double nu[NM], hv[NM];
#pragma unroll
    for (int m = 0; m < NM; m++) {
        const double2 p = M.nh[m];
        nu[m] = p.x;
        hv[m] = p.y;
    }
    const double g2 = M.g;
    const int i0 = M.i0, i1 = M.i1;
    if (!(M.flags & F_ASYM)) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (FULL || (bin[k] >= i0 && bin[k] < i1)) {
                double res = 0.0;
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    const double d = xv[k] - nu[m];
                    double p = d * d;
                    p = 4.0 * p / g2;
                    const double inv = 1.0 / (1.0 + p);
                    res = res + hv[m] * inv;
                }
                acc[k] = acc[k] + res;
            }
        }
    } else {
        const double asym = M.asym, fc = M.fcx, c2sq = M.c2sq;
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (FULL || (bin[k] >= i0 && bin[k] < i1)) {
                const double t = 1.0 + asym * (xv[k] / fc - 1.0);
                const double asy = t * t + c2sq;
                double res = 0.0;
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    const double d = xv[k] - nu[m];
                    double p = d * d;
                    p = 4.0 * p / g2;
                    const double inv = 1.0 / (1.0 + p);
                    res = res + hv[m] * (asy * inv);
                }
                acc[k] = acc[k] + res;
            }
        }
    }
}

// ---- FAST: sum_m hv_m/q_m over a common denominator: 3 ops per component for q_m, 3 for (N,D),
//      ONE reciprocal (+1 Newton step) per multiplet per bin ----
//      The argument of component m is t = (x - nu_m) 2/gamma = (x - x_c) 2/gamma - A_m with A_m staged per tile: one fma per
//      component from the bin's offset to the tile centre (|x - x_c| <= half a tile, so the fma's rounding is ~1e-15 of t's scale).
template <int NM, int K, bool FULL>
__device__ __forceinline__ void fast_mult(const LdsMult &M, const double (&xv)[K], const int (&bin)[K], double (&acc)[K], double xc) {
    double nA[NM], hv[NM];
#pragma unroll
    for (int m = 0; m < NM; m++) {
        const double2 p = M.nh[m];
        nA[m] = -p.x;
        hv[m] = p.y;
    }
    const double g = M.g;
    const int i0 = M.i0, i1 = M.i1;
    const int flags = M.flags;
    if (flags & F_SAFE) {
        const bool has_asym = flags & F_ASYM;
        const double afc = M.fcx, c2sq = M.c2sq, one_m_asym = 1.0 - M.asym;
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (FULL || (bin[k] >= i0 && bin[k] < i1)) {
                const double xx = xv[k];
                const double dx = xx - xc;
                double t = fma(dx, g, nA[0]);
                double D = fma(t, t, 1.0);
                double N = hv[0];
#pragma unroll
                for (int m = 1; m < NM; m++) {
                    t = fma(dx, g, nA[m]);
                    const double q = fma(t, t, 1.0);
                    N = fma(N, q, hv[m] * D);
                    D = D * q;
                }
                double res = N * rcp_nr1(D);
                if (has_asym) {
                    const double ta = fma(afc, xx, one_m_asym);
                    res = res * fma(ta, ta, c2sq);
                }
                acc[k] = acc[k] + res;
            }
            if (K > 4 && (k & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // bound the live ranges: four bins in flight
        }
    } else {  // denominators too large to multiply on this tile: plain sum (never taken for sane widths)
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (FULL || (bin[k] >= i0 && bin[k] < i1)) {
                const double xx = xv[k];
                const double dx = xx - xc;
                double res = 0.0;
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    const double t = fma(dx, g, nA[m]);
                    res = res + hv[m] / fma(t, t, 1.0);
                }
                if (flags & F_ASYM) {
                    const double ta = fma(M.fcx, xx, 1.0 - M.asym);
                    res = res * fma(ta, ta, M.c2sq);
                }
                acc[k] = acc[k] + res;
            }
        }
    }
}

template <bool FAST, int NM, int K>
__device__ __forceinline__ void mult_dispatch(const LdsMult &M, const double (&xv)[K], const int (&bin)[K], double (&acc)[K], double xc) {
    if (M.flags & F_FULL) {
        if (FAST) fast_mult<NM, K, true>(M, xv, bin, acc, xc);
        else strict_mult<NM, K, true>(M, xv, bin, acc);
    } else {
        if (FAST) fast_mult<NM, K, false>(M, xv, bin, acc, xc);
        else strict_mult<NM, K, false>(M, xv, bin, acc);
    }
}


// ---- the FAST far field of one multiplet on one tile: ONE definition, shared by the tile's staging pass and coefficient phase below and
//      by k_fd_far (kernels.hip), which takes whole far-only tiles with one lane per tile.  A tile must be far for both or for neither ----
__device__ __forceinline__ double far_ig(const tamcmc_multiplet &g) { return 2.0 * rcp_nr2(g.gamma); }  // 2/gamma: t = (x - nu_m) 2/gamma
__device__ __forceinline__ double far_arg(double ig, double nu, double xc) { return ig * (nu - xc); }    // A_m = -t at the tile centre
__device__ __forceinline__ double far_rho2_max(bool asym) { return asym ? RHO_MAX2_ASYM : RHO_MAX2; }
// the far test of one component (of a row that has one: `live`): `far` falls unless rho^2 = beta^2/(A^2+1) <= r2, beta = h 2/gamma; also for NaN
// (a statement, not a predicate: as an expression the staging pass's seven branches become selects -- other code in the hot kernels)
__device__ __forceinline__ void far_component(bool &far, bool live, double beta2, double r2, double A) {
    if (live && !(beta2 <= r2 * fma(A, A, 1.0))) far = false;
}
// FAST asymmetry scalars: reciprocal + Newton steps instead of the two IEEE divides by nu_c (exact zeros when asym = 0 either way)
__device__ __forceinline__ void fast_asym_scalars(const tamcmc_multiplet &g, double &c2sq, double &fcx) {
    const double ifc = rcp_nr2(g.fc);
    const double c2 = 0.5 * g.gamma * g.asym * ifc;
    c2sq = c2 * c2;
    fcx = g.asym * ifc;
}
// the asymmetry factor (1+asym(x/nu_c-1))^2 + c2^2 = A0 + A1 s + A2 s^2 on the tile (fcx = asym/nu_c)
struct AsymPoly { double A0, A1, A2; };
__device__ __forceinline__ AsymPoly asym_poly(double fcx, double asym, double c2sq, double xc, double h) {
    const double p0 = fma(fcx, xc, 1.0 - asym), p1 = fcx * h;
    return {fma(p0, p0, c2sq), 2.0 * p0 * p1, p1 * p1};
}
// One component hv/(1+(beta s - A)^2) = sum_k c_k s^k: c_0 and the two constants of c_{k+1} = two_req c_k - q2 c_{k-1} (q2 = rho^2)
struct FarSeed { double c0, two_req, q2; };
__device__ __forceinline__ FarSeed far_seed(double hv, double A, double beta) {
    const double inv = rcp_nr2(fma(A, A, 1.0));
    return {hv * inv, 2.0 * beta * A * inv, beta * beta * inv};
}
// fc[k] += c_k.  EARLY_STOP (the caller's choice; the whole wave must be here): n coefficients where rho^n <= 1e-13, i.e. tau(rho, n) <= 1.7e-12 (above), the wave's longest loop runs
template <bool EARLY_STOP>
__device__ __forceinline__ void far_coefs(const FarSeed &f, double (&fc)[NC]) {
    double cm = f.c0, cc = cm * f.two_req;  // c_0, c_1
    fc[0] = fc[0] + cm;
    fc[1] = fc[1] + cc;
    const double q2 = f.q2;
    int nt = NC;
    if constexpr (EARLY_STOP) nt = (q2 > 1.39e-2) ? 16 : (q2 > 6.8e-3) ? 14 : (q2 > 2.5e-3) ? 12 : (q2 > 5.6e-4) ? 10 : (q2 > 4.6e-5) ? 8 : 6;
#pragma unroll
    for (int k = 2; k < NC; k++) {
        if (EARLY_STOP && (k & 1) == 0 && k >= 6 && !__any(k < nt)) break;  // wave-uniform
        const double cn = fma(f.two_req, cc, -q2 * cm);
        fc[k] = fc[k] + cn;
        cm = cc;
        cc = cn;
    }
}
// fc[k] += (c * (A0, A1, A2))_k, the component times the asymmetry factor
__device__ __forceinline__ void far_coefs_asym(const FarSeed &f, const AsymPoly &P, double (&fc)[NC]) {
    double c2 = 0.0, c1 = 0.0, c0k = f.c0;  // c_{k-2}, c_{k-1}, c_k
    const double nxt = f.c0 * f.two_req;
#pragma unroll
    for (int k = 0; k < NC; k++) {
        fc[k] = fc[k] + fma(P.A0, c0k, fma(P.A1, c1, P.A2 * c2));
        const double cn = (k == 0) ? nxt : fma(f.two_req, c0k, -f.q2 * c1);
        c2 = c1;
        c1 = c0k;
        c0k = cn;
    }
}

// Moment form of a far-only tile of a DELTA launch (see tile_compute): layout of a tile's FD_MOM moments and the gate.  The two
// users spend their lanes differently (a lane per coefficient with shuffles here, a lane per tile with a serial loop in k_fd_far); each
// keeps its own summation order.
constexpr int FD_W1 = 0, FD_W2 = NC, FD_RMAX = FD_MOM - 1;  // W1_k (k < NC), W2_m (m < 2 NC - 1), max 1/M0
static_assert(FD_MOM == NC + (2 * NC - 1) + 1, "moment layout");
// u^3 is omitted: below 1e-10 of the leading term when max|u| <= 1e-5, bounded by sum|c_k| max(1/M0)  (false for NaN)
__device__ __forceinline__ bool moment_form_holds(double sum_abs_c, double rmax) { return sum_abs_c * rmax <= 1e-5; }

// The workgroup's LDS (one object per workgroup, declared by the kernel: a fused kernel overlays it with its other roles' scratch).
template <int MODE, int WGS>
struct __attribute__((aligned(16))) TileLds {
    static constexpr bool FARFIELD = (MODE == M_FAST);
    // multiplet list and (after the multiplet loop) the coefficient-reduction rows share one region
    static constexpr int LDS_BYTES = FARFIELD ? (WGS * ROW * 8 > CHUNK * (int)sizeof(LdsMult) ? WGS * ROW * 8 : CHUNK * (int)sizeof(LdsMult))
                                              : CHUNK * (int)sizeof(LdsMult);
    unsigned char buf[LDS_BYTES];
    double coef[NC];               // FARFIELD: the tile's far-field polynomial
    double part[WGS / 16][NC];
    double red[2 * (WGS / 64)];
    double lt[TAMCMC_MAX_HARVEY];  // FAST: ln(1e-3*tau_k)
    double lto[TAMCMC_MAX_HARVEY]; // DELTA: ln(1e-3*tau_k) of the base point
    int n, nfar, anyfar;           // anyfar: bit 0 = the tile polynomial is in use, bit 1 = the prebuilt background series came refused (bg_series.h)
    unsigned short slot[CHUNK * 7];  // FARFIELD: this chunk's far COMPONENTS, packed: (position in the list) << 3 | m
};

// ---- staging of one chunk of the table (wave 0): every overlapping multiplet into LDS, near field first; returns the number of near ones ----
template <int MODE, int WGS>
__device__ __forceinline__ int stage_chunk(const LoglikeArgs &a, int t0, int t1, double xc, double h, TileLds<MODE, WGS> &S, tamcmc_multiplet &g, int c0, int mbeg,
                                           int mend, const Probe &probe) {
    constexpr bool FAST = (MODE != M_STRICT), FARFIELD = (MODE == M_FAST);
    const int tid = threadIdx.x;
    if (tid < 64) {
        const int idx = c0 + tid;
        // the whole row in ONE round trip (clamped index: lanes past the end stage nothing); with a.per its address does not wait for the range
        g = a.mults[a.per > 0 ? min(idx, mbeg + a.per - 1) : min(idx, mend - 1)];
        const int i0 = g.i0, i1 = g.i1;
        const bool ov = (idx < mend) && (i0 < t1) && (i1 > t0) && !probe.skip(16);
        // every overlapping multiplet is staged with its per-multiplet scalars hoisted: the NEAR ones first (in table order: the
        // per-bin loop below walks them without looking at a flag), the far ones -- they only feed the tile polynomial -- behind
        // them.  Pass 1 decides near / far (its temporaries die at the ballot), pass 2 builds the LDS image in place.
        const int l = g.l;
        const int nm = 2 * l + 1;
        const bool full = (i0 <= t0 && i1 >= t1);
        bool far = false;
        if (FARFIELD && ov && full) {
            const double ig = far_ig(g);
            const double beta2 = (ig * h) * (ig * h);
            const double r2 = far_rho2_max(g.asym != 0.0);
            far = true;
#pragma unroll
            for (int m = 0; m < 7; m++) {
                const double A = far_arg(ig, g.nu[m], xc);
                far_component(far, m < nm, beta2, r2, A);
            }
        }
        const unsigned long long mask = __ballot(ov);
        const unsigned long long fmask = FARFIELD ? __ballot(far) : 0ull;
        const unsigned long long lt = (1ull << tid) - 1ull;
        const int n_near = __popcll(mask & ~fmask);
        const int pos = far ? n_near + __popcll(fmask & lt) : __popcll(mask & ~fmask & lt);
        if (ov) {
            LdsMult &d = ((LdsMult *)S.buf)[pos];
            int flags = 0;
            if (full) flags |= F_FULL;
            if (g.asym != 0.0) flags |= F_ASYM;
            double c2sq, fcx;
            if (FAST) fast_asym_scalars(g, c2sq, fcx);
            else {
                const double c2 = 0.5 * g.gamma * g.asym / g.fc;
                c2sq = c2 * c2;
                fcx = g.fc;
            }
            d.c2sq = c2sq;
            d.asym = g.asym;
            double Am[7];
            if (FAST) {
                const double ig = far_ig(g);
                d.g = ig;
                d.fcx = fcx;
#pragma unroll
                for (int m = 0; m < 7; m++) Am[m] = far_arg(ig, g.nu[m], xc);  // constant trip count: g stays in registers
                if (far) flags |= F_FAR;
                else {
                    // prod_m (1 + ((x-nu_m) ig)^2) < (1e38)^7 = 1e266 on the whole tile?
                    const double bh = ig * h;  // |t| <= |A_m| + beta on the nominal tile (a coarse bound)
                    bool safe = true;
#pragma unroll
                    for (int m = 0; m < 7; m++) {
                        const double dm = fabs(Am[m]) + bh;
                        if (m < nm && !(fma(dm, dm, 1.0) < 1e38)) safe = false;  // also false for NaN/inf inputs
                    }
                    if (safe) flags |= F_SAFE;
                }
            } else {
                d.g = g.gamma * g.gamma;
                d.fcx = fcx;
            }
            d.i0 = i0; d.i1 = i1; d.l = l; d.flags = flags;
#pragma unroll
            for (int m = 0; m < 7; m++) d.nh[m] = make_double2(FAST ? Am[m] : g.nu[m], g.hv[m]);
        }
        if (FARFIELD) {
            // far components packed densely (no idle lanes for l < 3): offset = components of the far multiplets before this lane
            const int lv = ov ? g.l : 0;
            const unsigned long long f0 = __ballot(far && lv == 0), f1 = __ballot(far && lv == 1), f2 = __ballot(far && lv == 2),
                                     f3 = __ballot(far && lv >= 3);
            if (far) {
                const int off = __popcll(f0 & lt) + 3 * __popcll(f1 & lt) + 5 * __popcll(f2 & lt) + 7 * __popcll(f3 & lt);
                const int nmf = 2 * (lv > 3 ? 3 : lv) + 1;
                for (int m = 0; m < nmf; m++) S.slot[off + m] = (unsigned short)((pos << 3) | m);
            }
            if (tid == 0) {
                S.nfar = __popcll(f0) + 3 * __popcll(f1) + 5 * __popcll(f2) + 7 * __popcll(f3);  // far components of the chunk
                if (f0 | f1 | f2 | f3) S.anyfar = 1;
            }
        }
        if (tid == 0) S.n = n_near;
    }
    __syncthreads();
    return S.n;
}

// ---- background + likelihood terms of the lane's bins (STRICT, FAST, DELTA) into s[0], s[1]; WRITE_MODEL: the model / fd_rows stores ----
template <int MODE, int K, bool WRITE_MODEL, bool DELTA>
__device__ __forceinline__ void likelihood_terms(const LoglikeArgs &a, int b, int nh, int nn, const double *nz, const double *nzo, bool bg, bool harvey_poly,
                                                 bool dsub, bool fullnew, const double *s_lt, const double *s_lto, const double (&xv)[K],
                                                 const double (&yv)[K], const int (&bin)[K], const double (&acc)[K], const Probe &probe, double (&s)[2]) {
    constexpr bool FAST = (MODE != M_STRICT);
    const double white = nz[nn - 1];
    // FAST: the thread's K bins share ONE logarithm and ONE reciprocal: sum_k ln M_k = ln prod_k M_k and sum_k y_k/M_k = N / prod_k M_k with
    // N <- N M_k + y_k D built beside the product (three instructions per bin instead of a reciprocal with two Newton steps)
    double prod = 1.0, ynum = 0.0;
    double Mk[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        double Mv = acc[k];
        const int bi = min(bin[k], a.Nx - 1);
        const bool valid = bin[k] < a.Nx;
        if (!FAST) {
            for (int hh = 0; hh < nh; hh++) {
                const double tau = nz[3 * hh + 1];
                if (tau != 0.0) {
                    double t = pow((1e-3 * tau) * xv[k], nz[3 * hh + 2]);
                    t = nz[3 * hh] * (1.0 / (t + 1.0));
                    Mv = Mv + t;
                }
            }
            Mv = Mv + white;
            if (valid) {
                s[0] = s[0] + yv[k] * (1.0 / Mv);
                s[1] = s[1] + log(Mv);
            }
        } else {
            if (bg && !harvey_poly) {
                const double lx = a.logx[bi];
                for (int hh = 0; hh < nh; hh++) {
                    const double tau = nz[3 * hh + 1];
                    if (tau != 0.0) {
                        const double t = exp(nz[3 * hh + 2] * (s_lt[hh] + lx));
                        Mv = fma(nz[3 * hh], rcp_nr2(t + 1.0), Mv);
                    }
                    if (dsub) {
                        const double tauo = nzo[3 * hh + 1];
                        if (tauo != 0.0) {
                            const double t = exp(nzo[3 * hh + 2] * (s_lto[hh] + lx));
                            Mv = fma(-nzo[3 * hh], rcp_nr2(t + 1.0), Mv);
                        }
                    }
                }
                Mv = Mv + (dsub ? (white - nzo[nn - 1]) : white);
            }
            if (DELTA) {
                // Mv = dM; u = dM / M0.  Change of the bin's likelihood term y/M + ln M:
                //   y/(M0+dM) - y/M0 + ln(1 + dM/M0) = -(y/M0) u/(1+u) + log1p(u) = sum_n (-1)^n (y/M0 - 1/n) u^n.
                // The base launch left 1/M0 and y/M0 per bin (two planes); a forward-difference step gives |u| ~ 1e-7 .. 1e-3, where five terms
                // of the series are exact to rounding (omitted: u^6, < 1e-10 of the leading term for |u| <= 0.01) and cost a third of two
                // reciprocals and a log1p; a bin beyond that (a step of percent size) takes the closed form -- wave-uniform choice.
                const size_t o = (size_t)a.d_row[b] * a.Nx + (size_t)min(bin[k], a.Nx - 1);
                const double r0 = a.model0[o], yr = a.model0[a.fd_plane + o];
                const double u = (fullnew ? Mv - a.model0[2 * a.fd_plane + o] : Mv) * r0;
                double f;
                if (!__any(valid && !(fabs(u) <= 0.01))) {
                    double pz = fma(u, 0.2 - yr, yr - 0.25);
                    pz = fma(u, pz, (1.0 / 3.0) - yr);
                    pz = fma(u, pz, yr - 0.5);
                    pz = fma(u, pz, 1.0 - yr);
                    f = u * pz;
                } else f = fma(-yr * u, rcp_nr2(1.0 + u), log1p(u));
                if (valid) s[0] = s[0] + f;
            } else if (valid) {
                if (probe.skip(8)) s[0] = s[0] + yv[k] * Mv;
                else {
                    ynum = fma(ynum, Mv, yv[k] * prod);
                    prod = prod * Mv;
                }
            }
        }
        Mk[k] = Mv;
        if (WRITE_MODEL) {
            if (valid) {
                if (a.fd_rows) {  // base point of a finite-difference batch: what the DELTA launch needs of it (see there)
                    const double r0 = FAST ? rcp_nr2(Mv) : 1.0 / Mv;
                    a.fd_rows[(size_t)b * a.Nx + bin[k]] = r0;
                    a.fd_rows[a.fd_plane + (size_t)b * a.Nx + bin[k]] = yv[k] * r0;
                    a.fd_rows[2 * a.fd_plane + (size_t)b * a.Nx + bin[k]] = Mv;  // (for the "full table" evaluations of the DELTA launch)
                } else a.model[(size_t)b * a.Nx + bin[k]] = Mv;
            }
        }
    }
    if (FAST && !DELTA) {
        if (prod > 1e-280 && prod < 1e280) {
            s[1] = log(prod);
            s[0] = s[0] + ynum * rcp_nr2(prod);
        } else {  // product out of range (or NaN): bin by bin
#pragma unroll
            for (int k = 0; k < K; k++)
                if (bin[k] < a.Nx) {
                    s[1] = s[1] + log(Mk[k]);
                    s[0] = fma(yv[k], rcp_nr2(Mk[k]), s[0]);
                }
        }
    }
}

// ---- Horner evaluation of the tile polynomial (far multiplets and/or the background series) at the lane's bins ----
template <int K>
__device__ __forceinline__ void horner(const double *s_coef, double xc, double h, const double (&xv)[K], double (&acc)[K]) {
    const double inv_h = 1.0 / h;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double sx = (xv[k] - xc) * inv_h;
        double P = s_coef[NC - 1];
#pragma unroll
        for (int q = NC - 2; q >= 0; q--) P = fma(P, sx, s_coef[q]);
        acc[k] = acc[k] + P;
    }
}

// ---- reduction over the workgroup and the store of the tile's two sums (lane 0; the hook sees them too) ----
template <int WGS, class Hook>
__device__ __forceinline__ void reduce_and_store(const LoglikeArgs &a, double (&s)[2], double *s_red, int b, int tile, const Hook &hook) {
    double out[2];
    block_reduce<2, WGS>(s, s_red, out);
    if (threadIdx.x == 0) {
        double *p = a.partials + ((size_t)b * a.ntiles + tile) * 2;
        p[0] = out[0];
        p[1] = out[1];
        hook.store_sums(b, tile, out[0], out[1]);
    }
}

// ---- DELTA early exits: the tile is k_fd_far's, or it lies outside the affected range (workgroup-uniform, before any barrier) ----
__device__ __forceinline__ bool delta_tile_done(const LoglikeArgs &a, int t0, int t1, int b, int tile) {
    if (a.d_done && a.d_done[(size_t)b * a.ntiles + tile]) return true;  // a far-only tile of a light evaluation: k_fd_far (kernels.hip) did it
    const int lo = a.d_range[2 * b], hi = a.d_range[2 * b + 1];
    if (t1 <= lo || t0 >= hi) {  // tiles outside the affected bin range contribute exactly 0
        if (threadIdx.x == 0) {
            double *p = a.partials + ((size_t)b * a.ntiles + tile) * 2;
            p[0] = 0.0;
            p[1] = 0.0;
        }
        return true;
    }
    return false;
}

// ---- DELTA moment shortcut (one wave per tile).  A tile whose changed multiplets are ALL in its far field (most tiles of a perturbed
// frequency's window: the mode is near for three or four of a hundred) has dM = P(s), the tile polynomial, with |u| = |dM / M0| ~ 1e-7 of
// a far wing: the change of its likelihood terms, sum_b [(1 - y/M0) u - (1/2 - y/M0) u^2], is a dot product of the polynomial's
// coefficients (and of their self-convolution) with moments of the base point on this tile (k_fd_moments, kernels.hip) -- no bin is
// walked.  A tile beyond the gate (moment_form_holds) walks its bins: returns false.
__device__ __forceinline__ bool delta_moment_shortcut(const LoglikeArgs &a, const double *s_coef, int b, int tile) {
    const int tid = threadIdx.x;
    const double *mm = a.fd_mom + ((size_t)a.d_row[b] * a.ntiles + tile) * FD_MOM;
    const double w1 = (tid < NC) ? mm[FD_W1 + tid] : 0.0, w2 = (tid < 2 * NC - 1) ? mm[FD_W2 + tid] : 0.0, rmax = mm[FD_RMAX];
    const double ck = (tid < NC) ? s_coef[tid] : 0.0;
    double ab = fabs(ck);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ab = ab + __shfl_xor(ab, off, 64);
    if (!moment_form_holds(ab, rmax)) return false;
    double cv = 0.0;  // (c * c)_tid
    if (tid < 2 * NC - 1) {
        const int j0 = tid < NC ? 0 : tid - (NC - 1), j1 = tid < NC ? tid : NC - 1;
        for (int j = j0; j <= j1; j++) cv = fma(s_coef[j], s_coef[tid - j], cv);
    }
    double tot = fma(ck, w1, cv * w2);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) tot = tot + __shfl_xor(tot, off, 64);
    if (tid == 0) {
        double *p = a.partials + ((size_t)b * a.ntiles + tile) * 2;
        p[0] = tot;
        p[1] = 0.0;
    }
    return true;
}

// (rare, and out of line: inlined, the logarithm's temporaries would count against the tile's register budget)
__device__ __attribute__((noinline)) inline void refused_logs(double *s_lt, const double *nz, int nh, int tid) {
    for (int hh = tid; hh < nh; hh += NH) s_lt[hh] = log(1e-3 * nz[3 * hh + 1]);
}

// One tile of one evaluation: table slot `sb` (its multiplets, noise row, background series), result row `b` (partials / model).
// xpre (may be null): the lane's K values of x, requested by a caller that had something to wait for first (loglike_tile).
template <int MODE, int WGS, int K, bool WRITE_MODEL, bool DELTA, class Hook>
__device__ __forceinline__ void tile_compute(const LoglikeArgs &a, const int tile, const int b, const int sb, TileLds<MODE, WGS> &S, const int mbeg,
                                             const int mend, const int nh, const int nn, const Hook &hook, const double *xpre) {
    constexpr bool FAST = (MODE != M_STRICT);
    static_assert(!DELTA || (FAST && !WRITE_MODEL), "DELTA launches are FAST-mode, logL-only");
    constexpr bool FARFIELD = (MODE == M_FAST);
    LdsMult *s_m = (LdsMult *)S.buf;
    double *s_rows = (double *)S.buf;
    int &s_nfar = S.nfar, &s_anyfar = S.anyfar;
    unsigned short *s_slot = S.slot;
    double *s_coef = S.coef;
    double(*s_part)[NC] = S.part;
    double *s_red = S.red;
    double *s_lt = S.lt, *s_lto = S.lto;
    const int tid = threadIdx.x;
    const Probe probe(a, b, tile);
    probe.stamp(0);
    constexpr int TILE = WGS * K;
    const int t0 = tile * TILE;
    const int t1 = min(t0 + TILE, a.Nx);
    if (DELTA && delta_tile_done(a, t0, t1, b, tile)) return;

    tamcmc_multiplet g;
    // DELTA, bit 1 of the evaluation's flags ("full table"): a perturbation that moves most multiplets (a splitting coefficient, the
    // asymmetry) is cheaper as the WHOLE perturbed model minus the base model row M0 (third plane of model0) than as +new / -old row
    // pairs -- per rows instead of up to 2 per.  The table then holds every row of the perturbed point, the background is the base
    // point's (the noise parameters did not change: its prebuilt series, a.bg_poly rows by base point), and dM = M - M0 per bin.  The
    // unchanged rows and the background are summed by the same code in the same order as in the base launch: they cancel exactly.
    const bool fullnew = DELTA && (a.d_flags[b] & 2);
    const bool dsub = DELTA && !fullnew;  // the evaluation carries -old rows / the old noise row: differences are formed term by term
    // prebuilt background series of this (evaluation, tile), one coefficient per lane: it stays in those lanes' registers and enters the
    // tile polynomial where the far-field sums are closed (no wait for it here, no trip through LDS)
    const bool bg_prebuilt = FARFIELD && a.bg_poly && (!DELTA || fullnew);
    double bg_pre = 0.0;
    if (bg_prebuilt && tid < NH) bg_pre = a.bg_poly[((size_t)(DELTA ? a.d_row[b] : sb) * a.ntiles + tile) * NH + tid];
    double xv[K], yv[K], acc[K];
    int bin[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        bin[k] = t0 + k * WGS + tid;
        const int bi = min(bin[k], a.Nx - 1);
        xv[k] = xpre ? xpre[k] : a.x[bi];
        acc[k] = 0.0;
    }

    const double *nz = a.noise + (size_t)sb * a.noise_stride;
    // DELTA: background difference only when the noise parameters changed (same Harvey count on both sides)
    const bool bg = !DELTA || fullnew || (a.d_flags[b] & 1);
    const double *nzo = DELTA ? a.d_noise_old + (size_t)b * a.noise_stride : nz;
    // tile geometry for the far field: centre and half-width of the nominal tile on the regular grid
    double xc, h;
    bg::tile_geometry(tile, TILE, a.x0, a.step, xc, h);
    // FARFIELD: the background H/(1+(a x)^p) + N0 is analytic on the tile with its singularities ~x_c away, so it joins the
    // tile polynomial: u(s) = (a x_c)^p (1+eps s)^p (binomial series), then the reciprocal series of 1+u.
    // The gate also looks at the steepest exponent of the evaluation's terms (of both noise rows where a DELTA evaluation subtracts the
    // old one).  With a prebuilt series its builder has applied that part -- here only the geometry, nothing to wait for -- and a tile it
    // refused comes marked: the polynomial then takes zeros for it (bg_mark) and the likelihood terms add the background per bin (series_on).
    bool harvey_poly = false;
    if (FARFIELD && bg) {
        if (bg_prebuilt) harvey_poly = bg::series_geometry(xc, h);
        else {
            double pmax = bg::max_exponent([nz](int i) { return nz[i]; }, nh);
            if (dsub) pmax = fmax(pmax, bg::max_exponent([nzo](int i) { return nzo[i]; }, nh));
            harvey_poly = bg::series_valid(xc, h, bg::gate_coef(pmax));
        }
    }
    if (FAST && bg && !harvey_poly) {
        if (tid < nh) {
            s_lt[tid] = log(1e-3 * nz[3 * tid + 1]);
            if (dsub) s_lto[tid] = log(1e-3 * nzo[3 * tid + 1]);
        }
    }
    if (FARFIELD) {
        if (tid < NC) s_coef[tid] = 0.0;
        if (tid == 0) s_anyfar = harvey_poly ? 1 : 0;
        __syncthreads();
        if (harvey_poly && !bg_prebuilt) {
            // lane = Harvey term (wave 1 when there are four waves: wave 0 is about to compact the first chunk); the NH
            // series coefficients of the terms are added to the tile polynomial in term order by the last of these lanes
            const int hl = (WGS > 64) ? tid - 64 : tid;
            double f[NH];
#pragma unroll
            for (int k = 0; k < NH; k++) f[k] = 0.0;
            const bool lane_new = (hl >= 0 && hl < nh), lane_old = dsub && (hl >= 32 && hl < 32 + nh);
            if (lane_new || lane_old) {
                const double *nq = lane_new ? nz : nzo;
                const int ht = lane_new ? hl : hl - 32;
                bg::harvey_term_series(lane_new ? nq[3 * ht] : -nq[3 * ht], nq[3 * ht + 1], nq[3 * ht + 2], xc, h, f);
            }
            // lanes hl = 0..nh-1 live in ONE wave: sum their series in lane order with shuffles, lane 0 adds the white noise
            if (hl >= 0 && hl < 64) {
#pragma unroll
                for (int k = 0; k < NH; k++) {
                    double v = f[k];
                    double tot = 0.0;
                    for (int t = 0; t < nh; t++) tot = tot + __shfl(v, t, 64);
                    if (dsub)
                        for (int t = 0; t < nh; t++) tot = tot + __shfl(v, 32 + t, 64);
                    const double wn = dsub ? (nz[nn - 1] - nzo[nn - 1]) : nz[nn - 1];
                    if (hl == 0) s_coef[k] = tot + (k == 0 ? wn : 0.0);
                }
            }
        }
    }

    // the table builder already summed the series of this (evaluation, tile) (bg_series.h, same arithmetic): still in registers
    bool bg_in_regs = harvey_poly && bg_prebuilt;
    // a series its builder refused (bg_series.h, NaN in every coefficient): the polynomial takes zeros for the background
    const auto bg_mark = [](double c) { return bg::refused(c) ? 0.0 : c; };
    bool any_near = false;  // (workgroup-uniform) a chunk held a multiplet of the near field
    probe.stamp(1);
    for (int c0 = mbeg; c0 < mend; c0 += CHUNK) {
        __syncthreads();  // previous chunk fully consumed
        const int n_near = stage_chunk(a, t0, t1, xc, h, S, g, c0, mbeg, mend, probe);
        probe.stamp(2);
        const int n = probe.skip(1) ? 0 : n_near;
        any_near = any_near || (n_near > 0);
        for (int q = 0; q < n; q++) {
            const LdsMult &M = s_m[q];  // (near multiplets only: the staging pass put them first)
            switch (M.l) {  // wave-uniform
            case 0: mult_dispatch<FAST, 1, K>(M, xv, bin, acc, xc); break;
            case 1: mult_dispatch<FAST, 3, K>(M, xv, bin, acc, xc); break;
            case 2: mult_dispatch<FAST, 5, K>(M, xv, bin, acc, xc); break;
            default: mult_dispatch<FAST, 7, K>(M, xv, bin, acc, xc); break;
            }
        }
        probe.stamp(3);
        if (FARFIELD && s_nfar > 0 && !probe.skip(2)) {  // workgroup-uniform
            // AFTER the near-field loop (its registers are dead): one lane per (far multiplet, m) slot computes the NC Taylor
            // coefficients of its component; the lanes' vectors are summed in a fixed order into the tile polynomial
            double fcoef[NC];
#pragma unroll
            for (int k = 0; k < NC; k++) fcoef[k] = 0.0;
            const int nslots = s_nfar;
            for (int slot = tid; slot < nslots; slot += WGS) {
                const int e = s_slot[slot];
                const LdsMult &M = s_m[e >> 3];
                const double2 nhm = M.nh[e & 7];
                const FarSeed f = far_seed(nhm.y, nhm.x, M.g * h);
                if (!(M.flags & F_ASYM)) far_coefs<true>(f, fcoef);
                else far_coefs_asym(f, asym_poly(M.fcx, M.asym, M.c2sq, xc, h), fcoef);
            }
            __syncthreads();  // every lane is done with the multiplet list: its LDS region now holds the reduction rows
#pragma unroll
            for (int k = 0; k < NC; k += 2) *(double2 *)&s_rows[tid * ROW + k] = make_double2(fcoef[k], fcoef[k + 1]);
            __syncthreads();
            {
                const int k = tid & 15, part = tid >> 4;
                double sum = 0.0;
#pragma unroll
                for (int r = 0; r < 16; r++) sum = sum + s_rows[(part * 16 + r) * ROW + k];
                s_part[part][k] = sum;
            }
            __syncthreads();
            if (tid < NC) {
                double sum = (bg_in_regs && tid < NH) ? bg_mark(bg_pre) : s_coef[tid];  // background first, then the parts: the order of the sum
#pragma unroll
                for (int p = 0; p < WGS / 16; p++) sum = sum + s_part[p][tid];
                s_coef[tid] = sum;
            }
            bg_in_regs = false;
        }
    }
    if (bg_in_regs && tid < NH) s_coef[tid] = bg_mark(bg_pre);  // (no far multiplet on this tile: the polynomial is the background alone)
    if (FARFIELD && bg_prebuilt && harvey_poly && tid < NH && bg::refused(bg_pre)) {  // rare: the per-bin background after all -- the lanes
        if (tid == 0) s_anyfar = 3;                                                    // that hold the series mark the tile and set up its logs
        refused_logs(s_lt, nz, nh, tid);
    }
    probe.stamp(4);
    // the power values: issued before the polynomial evaluation, consumed after it
#pragma unroll
    for (int k = 0; k < K; k++) yv[k] = DELTA ? 0.0 : a.y[min(bin[k], a.Nx - 1)];  // (DELTA: y enters through the base point's y/M0 plane)
    if (FAST) __syncthreads();  // s_lt / s_coef visible (also when the evaluation has no multiplet chunk)
    const bool series_on = harvey_poly && !(FARFIELD && (s_anyfar & 2));  // (workgroup-uniform)
    if constexpr (DELTA && FARFIELD && WGS == 64) {
        // A tile whose changed multiplets are ALL in its far field (most tiles of a perturbed frequency's window: the mode is near for
        // three or four of a hundred) has dM = P(s), the tile polynomial, with |u| = |dM / M0| ~ 1e-7 of a far wing: the change of its
        // likelihood terms, sum_b [(1 - y/M0) u - (1/2 - y/M0) u^2], is a dot product of the polynomial's coefficients (and of their
        // self-convolution) with moments of the base point on this tile (k_fd_moments, kernels.hip) -- no bin is walked.  A tile beyond
        // the gate (moment_form_holds) walks its bins.
        // (a perturbed noise parameter has no rows: its dM is the difference of two background series, a polynomial wherever the series is valid)
        if (a.fd_mom && (!bg || harvey_poly) && !fullnew && !any_near) {  // workgroup-uniform
            if (delta_moment_shortcut(a, s_coef, b, tile)) return;
        }
    }
    if (FARFIELD && s_anyfar && !probe.skip(4)) horner(s_coef, xc, h, xv, acc);  // workgroup-uniform: far multiplets and/or the background series

    probe.stamp(5);
    // ---- background + likelihood terms ----
    double s[2] = {0.0, 0.0};
    likelihood_terms<MODE, K, WRITE_MODEL, DELTA>(a, b, nh, nn, nz, nzo, bg, series_on, dsub, fullnew, s_lt, s_lto, xv, yv, bin, acc, probe, s);
    __syncthreads();
    reduce_and_store<WGS>(a, s, s_red, b, tile, hook);
    probe.stamp(6);
    probe.timeline(b, tile);
}

// What a table slot leads to: its multiplet range and the lengths of its noise row.
struct SlotWords { int sb, nn, nh, mbeg, mend; };
// everything the slot index leads to is requested at once (one memory round trip, not one per dependent step): the table's range,
// the noise row's lengths; a.per > 0 (device-built tables in fixed-size slots): the range begins at (slot0 + sb) * per
__device__ __forceinline__ SlotWords slot_words(const LoglikeArgs &a, int sb) {
    SlotWords w;
    w.sb = sb; w.nn = a.nnoise[sb]; w.nh = a.nharvey[sb];
    w.mend = a.offsets[2 * sb + 1];
    w.mbeg = a.per > 0 ? (a.slot0 + sb) * a.per : a.offsets[2 * sb];
    return w;
}

// Hook of loglike_tile: which table slot evaluation b reads, and what lane 0 does with the tile's two sums beside storing them.
// early_loads: the slot takes the hook a memory round trip or more to name (head(), in place of slot(): the slot AND its words) -- the
// tile's x, which depends on the tile alone, is requested before it and consumed after it.  (Not y: held from here to the likelihood terms,
// its K values per lane would not fit the 168 registers of the fused step's three waves per SIMD.)
struct DirectSlots {
    static constexpr bool early_loads = false;
    __device__ __forceinline__ int slot(const LoglikeArgs &, int b, int /*tile*/) const { return b; }  // evaluation b reads table slot b
    __device__ __forceinline__ void store_sums(int /*b*/, int /*tile*/, double, double) const {}
};

// Workgroup `id` of a launch over ntiles x B (tile, evaluation) pairs, XCD-aware: ids id, id+8, id+16, .. share an XCD (round-robin
// dispatch), so all evaluations of one tile are placed on the XCD whose L2 holds that tile's x/y.
// The hook names the table slot of evaluation b (fused sampler step: decided on the device from the previous launch's sums).
template <int MODE, int WGS, int K, bool WRITE_MODEL, bool DELTA, class Hook>
__device__ __forceinline__ void loglike_tile(const LoglikeArgs &a, const int id, TileLds<MODE, WGS> &S, const Hook &hook) {
    const int xcd = id & 7, j = id >> 3;
    // launch order = tile_rot, tile_rot+1, ..., wrapping: the caller points tile_rot at the first tile of the mode region so
    // that the long-running tiles (near field) are dispatched first and the cheap far-field-only tiles fill the tail
    const int b = j % a.B;
    int tile = (j / a.B) * 8 + xcd;
    if (tile >= a.ntiles) return;  // padding workgroup: leaves before any barrier
    tile += a.tile_rot;
    if (tile >= a.ntiles) tile -= a.ntiles;
    SlotWords w;
    double xpre[Hook::early_loads ? K : 1];
    if constexpr (Hook::early_loads) {
#pragma unroll
        for (int k = 0; k < K; k++) xpre[k] = a.x[min(tile * (WGS * K) + k * WGS + (int)threadIdx.x, a.Nx - 1)];
        w = hook.head(a, b, tile);
    } else w = slot_words(a, hook.slot(a, b, tile));
    if (w.nn > 0)  // else: empty evaluation slot (a candidate that was not built, or whose table failed)
        tile_compute<MODE, WGS, K, WRITE_MODEL, DELTA, Hook>(a, tile, b, w.sb, S, w.mbeg, w.mend, w.nh, w.nn, hook, Hook::early_loads ? xpre : nullptr);
}

}  // namespace tile
}  // namespace tamcmc
