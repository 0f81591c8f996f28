// dev_iterate_impl.h -- device code of the lockstep scheme (included by dev_sampler.hip, inside its anonymous namespace, before
// dev_step_impl.h and dev_mala_impl.h, which use what is defined here).
//
// The pieces every scheme shares -- the Metropolis-Hastings outcome of one chain (mh_outcome), the sums of a chain's per-tile partials in
// k_finalize's order, the Robbins-Monro adaptation with its blocked Cholesky factorisation (adapt_chain), the proposal x' = x + L z with
// its log-prior and multiplet table (propose_common), the parallel-tempering swap (resolve_swap) -- and k_iterate, the lockstep
// scheme's one kernel per iteration besides the likelihood kernel.

// value of x in lane LANE (a compile-time constant) for every lane: v_readlane, no LDS round trip like __shfl
template <int LANE>
__device__ __forceinline__ double lane_value(double x) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), LANE), hi = __builtin_amdgcn_readlane((int)(b >> 32), LANE);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>): a loop whose index is a compile-time constant in every copy of its body,
// so that small register arrays indexed by it stay in registers (`#pragma unroll` is a request the optimiser may turn down)
// (the body's call is inlined whatever the caller's size: left as a call, the arrays its lambda captures by reference live in scratch)
template <int I, int N, class F>
__device__ __forceinline__ void static_for_from(F &f) {
    if constexpr (I < N) {
        [[clang::always_inline]] f(std::integral_constant<int, I>{});
        static_for_from<I + 1, N>(f);
    }
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    static_for_from<0, N>(f);
}

constexpr int TB = 256;  // threads of k_iterate (one workgroup per chain)

// Outcome of the Metropolis-Hastings test of chain j for the pending iteration (MALA.cpp:490-551): the values the
// chain holds AFTER the test.
struct AcceptOut {
    int acc;
    double r, logL, logPr, logPost;
};

// MALA.cpp:490-551 for one chain, by ONE lane: S = sum of the chain's per-tile partials, (logPr, status) = the proposal's prior and
// table status, logPost_cur / logL_cur / logPr_cur = what the chain holds.  The same statement sequence serves both launch schemes.
template <class AT>  // AT: DevSamplerArgs, or the same block read through a constant-memory reference (fused settle)
__device__ __forceinline__ AcceptOut mh_outcome(const AT &a, int j, long itp, double S, double logPr, int status, double logL_cur,
                                                double logPr_cur, double logPost_cur, double Tcoef, double init_logL) {
    double logL = (-(double)a.pl * S) / Tcoef;  // call_likelihood, model_def.cpp:399-401
    double logPost;
    if (status != TAMCMC_OK) logL = NAN;
    if (logPr == -INFINITY || isnan(logPr)) { logL = init_logL; logPost = -INFINITY; }  // model_def.cpp:476-480
    else logPost = logL + logPr;
    double u, u1;
    rng_uniform2(a.seed, RNG_ACCEPT, (uint32_t)j, (uint64_t)itp, 0, u, u1);
    double r;
    if (!isnan(logL)) {
        if (logPost == -INFINITY) r = 0.;
        else {
            const double e = exp(logPost - logPost_cur);
            r = fmin(1.0, e);
            if (isnan(r)) r = 0.;
        }
    } else r = 0.;
    AcceptOut o;
    o.acc = (u <= r) ? 1 : 0;
    o.r = r;
    if (o.acc) { o.logL = logL; o.logPr = logPr; o.logPost = logPost; }
    else { o.logL = logL_cur; o.logPr = logPr_cur; o.logPost = logPost_cur; }
    return o;
}

// (B): computed by a whole 256-thread workgroup; every workgroup that needs chain j's outcome (the chain's own workgroup and, in a
// swap step, its partner's) recomputes it from the same inputs -> identical results.
__device__ __forceinline__ void accept_result(const DevSamplerArgs &a, int j, long itp, int P, double *s_red, AcceptOut *s_out) {
    const int tid = threadIdx.x;
    // same reduction order as k_finalize (kernels.hip): strided per-thread sums, shuffle tree, waves in order
    double s1 = 0, s2 = 0;
    for (int t = tid; t < a.ntiles; t += TB) {
        const double *p = a.partials + ((size_t)j * a.ntiles + t) * 2;
        s1 = s1 + p[0];
        s2 = s2 + p[1];
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s1 = s1 + __shfl_down(s1, off, 64);
        s2 = s2 + __shfl_down(s2, off, 64);
    }
    __syncthreads();
    if (lane == 0) { s_red[2 * wave] = s1; s_red[2 * wave + 1] = s2; }
    __syncthreads();
    if (tid == 0) {
        double t1 = s_red[0], t2 = s_red[1];
        for (int w = 1; w < TB / 64; w++) { t1 = t1 + s_red[2 * w]; t2 = t2 + s_red[2 * w + 1]; }
        const int C = a.C;
        *s_out = mh_outcome(a, j, itp, t1 + t2, a.logPr_prop[P * C + j], a.status_prop[P * C + j], a.logL_cur[P * C + j], a.logPr_cur[P * C + j],
                            a.logPost_cur[P * C + j], a.Tcoefs[j], a.init_logL[j]);
    }
    __syncthreads();
}

// Sum of a chain's per-tile partials by ONE wave in k_finalize's order (kernels.hip): 256 strided per-thread sums (four per lane here),
// a shuffle tree per 64, the four in order.  Every lane returns the total.
__device__ __forceinline__ double wave_sum_in_order(const double (&s1)[TB / 64], const double (&s2)[TB / 64]) {
    double t1 = 0, t2 = 0;
#pragma unroll
    for (int q = 0; q < TB / 64; q++) {
        double a1 = s1[q], a2 = s2[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            a1 = a1 + __shfl_down(a1, off, 64);
            a2 = a2 + __shfl_down(a2, off, 64);
        }
        if (q == 0) { t1 = a1; t2 = a2; }
        else { t1 = t1 + a1; t2 = t2 + a2; }
    }
    return __shfl(t1 + t2, 0, 64);
}
__device__ __forceinline__ double wave_partial_sum(const double *base, int ntiles) {
    const int lane = threadIdx.x & 63;
    double s1[TB / 64], s2[TB / 64];
#pragma unroll
    for (int q = 0; q < TB / 64; q++) { s1[q] = 0; s2[q] = 0; }
    for (int t0 = 0; t0 < ntiles; t0 += TB) {  // virtual thread q*64+lane of k_finalize adds tile t0 + q*64 + lane in this round
        double v1[TB / 64], v2[TB / 64];
#pragma unroll
        for (int q = 0; q < TB / 64; q++) {  // the round's loads first: one memory round trip instead of four
            const int t = t0 + q * 64 + lane;
            v1[q] = t < ntiles ? base[2 * t] : 0.0;
            v2[q] = t < ntiles ? base[2 * t + 1] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < TB / 64; q++)
            if (t0 + q * 64 + lane < ntiles) { s1[q] = s1[q] + v1[q]; s2[q] = s2[q] + v2[q]; }
    }
    return wave_sum_in_order(s1, s2);
}

// value of x in lane `lane` (wave-uniform, a run-time value) for every lane
__device__ __forceinline__ double lane_value_at(double x, int lane) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// The rank-one step of chain m's factor (factor_update.h: solve, then scale): LT <- the transposed Cholesky factor of
// beta2 L L^T + w w^T, w = wscale x d.  false: refused (a pivot or a coefficient not finite and positive), LT untouched.
//   IN_LDS   A [Nv x Nv] receives LT as it is stored (row k = column k of L: the substitution reads a column as one run, the sweep's
//            lanes read a row of L across a run); va, vb [Nv] are LDS vectors of the caller.  Up to 128 variables the substitution runs
//            in the registers of ONE wave (lane i: rows i and i + 64; p_k handed on by a lane read: no barrier and no memory round trip
//            per column, reciprocal pivots taken beforehand, all at a time) -- the pattern of k_mala_test's solves.
//   else     A IS LT (device memory, updated in place: the sweep's lane reads an element, then writes it); va, vb in the scratch.
// The sweep: lane i owns row i of L, columns i down to 0, with the suffix sum of L_ij p_j; rows are independent, no barrier inside, and
// every element is written straight to LT (lanes along a run).  d [Nv]: the deviation on entry, p = L^-1 w on exit.
// Called by all TB threads after a barrier; s_scal[2] is its refusal flag.  Ends with a barrier.
template <class WP, bool IN_LDS>
__device__ bool factor_rank_one_as(const DevSamplerArgs &a, int m, double beta2, double wscale, WP A, WP d, WP va, WP vb, double *s_scal) {
    const int tid = threadIdx.x, Nv = a.Nv;
    double *LT = a.LT + (size_t)m * Nv * Nv;
    const double beta = sqrt(beta2);
    const bool one_wave = IN_LDS && Nv <= 128;
    if constexpr (!IN_LDS) A = (WP)LT;
    if (tid == 0) s_scal[2] = (beta2 > 0.0 && beta2 <= 1.7976931348623157e308) ? 0.0 : 1.0;
    if constexpr (IN_LDS) {
        for (int e = tid; e < Nv * Nv; e += TB) A[e] = LT[e];
        if (one_wave)
            for (int k = tid; k < Nv; k += TB) va[k] = 1.0 / LT[(size_t)k * Nv + k];
    }
    for (int k = tid; k < Nv; k += TB) d[k] = d[k] * wscale;
    __syncthreads();
    if (one_wave) {
        if (tid < 64) {
            const int lane = tid, hi = lane + 64;
            double f0 = lane < Nv ? d[lane] : 0.0, f1 = hi < Nv ? d[hi] : 0.0;
            double alpha = beta2, ap0 = beta2, al0 = beta2, ap1 = beta2, al1 = beta2;
#pragma clang loop unroll(disable)
            for (int k = 0; k < Nv; k++) {
                const size_t row = (size_t)k * Nv;
                const double id = va[k];
                const double l0 = (lane > k && lane < Nv) ? A[row + lane] : 0.0, l1 = (hi > k && hi < Nv) ? A[row + hi] : 0.0;
                const double pk = lane_value_at(k < 64 ? f0 : f1, k & 63) * id;
                const double an = alpha + pk * pk;
                if (lane == (k & 63)) {
                    if (k < 64) { f0 = pk; ap0 = alpha; al0 = an; }
                    else { f1 = pk; ap1 = alpha; al1 = an; }
                }
                alpha = an;
                f0 = f0 - l0 * pk;  // (rows above the column: l = 0, the value stays)
                f1 = f1 - l1 * pk;
            }
            bool ok = true;
            if (lane < Nv) {
                double ca, cb;
                ok = factor_column(beta, ap0, al0, f0, &ca, &cb) && ok;
                d[lane] = f0; va[lane] = ca; vb[lane] = cb;
            }
            if (hi < Nv) {
                double ca, cb;
                ok = factor_column(beta, ap1, al1, f1, &ca, &cb) && ok;
                d[hi] = f1; va[hi] = ca; vb[hi] = cb;
            }
            if (!ok) s_scal[2] = 1.0;
        }
        __syncthreads();
    } else {
        // wide proposals: a column per step -- p_k and its coefficients by one lane, then every row below loses L_ik p_k
        double alpha = beta2;  // (lane 0's)
#pragma clang loop unroll(disable)
        for (int k = 0; k < Nv; k++) {
            if (tid == 0) {
                const double pk = d[k] * (1.0 / A[(size_t)k * Nv + k]);
                const double an = alpha + pk * pk;
                double ca, cb;
                if (!factor_column(beta, alpha, an, pk, &ca, &cb)) s_scal[2] = 1.0;
                alpha = an;
                d[k] = pk; va[k] = ca; vb[k] = cb;
            }
            __syncthreads();
            const double pk = d[k];
            for (int i = k + 1 + tid; i < Nv; i += TB) d[i] = d[i] - A[(size_t)k * Nv + i] * pk;
            __syncthreads();
        }
    }
    if (s_scal[2] != 0.0) {  // every lane leaves together, LT is not touched
        __syncthreads();
        return false;
    }
#pragma clang loop unroll(disable)
    for (int i = tid; i < Nv; i += TB) {
        double s = 0.0;
#pragma unroll 4
        for (int k = i; k >= 0; k--) {
            const size_t e = (size_t)k * Nv + i;
            const double v = A[e];
            LT[e] = v * va[k] + s * vb[k];
            s = s + v * d[k];
        }
    }
    __syncthreads();
    return true;
}

// Robbins-Monro adaptation of chain m's proposal law (MALA.cpp:296-319) and Cholesky of (Sigma+eps2 I) sigma
// (MALA.cpp:348-350); `vars` = the chain's position after the MH test, `Pm` = its move probability.
// WP: pointer type of the work matrix A and the vector d in their address space (LDS when the matrix fits there: ds_read/ds_write
// instead of flat accesses, whose latency is several times higher; device memory otherwise); PANELS: the blocked factorisation.
// fmode: what the factor does (step_schedule.h::factor_step_mode): 1 = today's full factorisation, 2 = a rank-one step of the factor
// in force where factor_update.h's rule allows it (va, vb: its two coefficient vectors [Nv], in A's address space); s_scal [4].
template <class WP, bool PANELS>
__device__ void adapt_chain_as(const DevSamplerArgs &a, int m, long itp, const double *vars, double Pm, WP A, WP d, double *s_red, double *s_scal,
                               int fmode, WP va, WP vb) {
    const int tid = threadIdx.x, Nv = a.Nv;
    const double g = a.c0 / (1. + (double)itp);
    double *mu = a.mu + (size_t)m * Nv;
    double *cov = a.cov + (size_t)m * Nv * Nv;
    double n2 = 0;
    for (int k = tid; k < Nv; k += TB) {
        const double v = mu[k] + g * (vars[k] - mu[k]);
        d[k] = v;
        n2 += v * v;
    }
    n2 = wg_sum(n2, s_red);
    {
        const double nrm = sqrt(n2);
        const double sc = (nrm <= a.A1) ? 1.0 : a.A1 / nrm;  // p3_fct
        for (int k = tid; k < Nv; k += TB) {
            const double v = (sc == 1.0) ? d[k] : d[k] * sc;
            mu[k] = v;
            d[k] = vars[k] - v;  // deviation from the UPDATED mu (MALA.cpp:311)
        }
    }
    __syncthreads();
#ifdef TAMCMC_PROBE
    if (a.probe == 1) return;
#endif
    // covariance update (MALA.cpp:313-316) and the matrix to factor, A = (Sigma + eps2 I) sigma, in one sweep over Sigma (device memory,
    // read and written once); lanes as a 16 x 16 grid over (row, column): no index arithmetic per element, 128-byte runs per row
    const int gi = tid >> 4, gk = tid & 15;
    n2 = 0;
    constexpr int CB = 8;  // columns of a lane per batch: two rows x CB device-memory reads are in flight before the first use
#pragma clang loop unroll(disable)
    for (int i = gi; i < Nv; i += 32) {
        const int i2 = i + 16;
        const bool two = i2 < Nv;
        const double di = d[i], di2 = two ? d[i2] : 0.0;
#pragma clang loop unroll(disable)
        for (int jb = gk; jb < Nv; jb += 16 * CB) {
            double c0[CB], c1[CB];
            static_for<CB>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                const int j = jb + 16 * q;
                c0[q] = (j < Nv) ? cov[(size_t)i * Nv + j] : 0.0;
                c1[q] = (two && j < Nv) ? cov[(size_t)i2 * Nv + j] : 0.0;
            });
            static_for<CB>([&](auto qc) {  // row i (the sum of squares keeps the element order of a plain row-by-row sweep per lane)
                constexpr int q = decltype(qc)::value;
                const int j = jb + 16 * q;
                if (j < Nv) {
                    const size_t e = (size_t)i * Nv + j;
                    const double v = c0[q] + g * (di * d[j] - c0[q]);
                    cov[e] = v;
                    A[e] = v;
                    n2 += v * v;
                }
            });
            static_for<CB>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                const int j = jb + 16 * q;
                if (two && j < Nv) {
                    const size_t e = (size_t)i2 * Nv + j;
                    const double v = c1[q] + g * (di2 * d[j] - c1[q]);
                    cov[e] = v;
                    A[e] = v;
                    n2 += v * v;
                }
            });
        }
    }
#ifdef TAMCMC_PROBE
    if (a.probe == 2) return;
#endif
    n2 = wg_sum(n2, s_red);
    if (tid == 0) {
        const double nrm = sqrt(n2);
        s_scal[0] = (nrm <= a.A1) ? 1.0 : a.A1 / nrm;  // p2_fct
        const double sig_old = a.sigma[m];
        double v1 = sig_old + g * (Pm - a.target_acceptance);
        if (v1 < a.epsilon1) v1 = a.epsilon1;  // p1_fct
        if (v1 > a.A1) v1 = a.A1;
        a.sigma[m] = v1;
        s_scal[1] = v1;
        const bool r1 = factor_takes_rank_one(fmode, g, s_scal[0] != 1.0, a.fvalid[m] != 0);
        s_scal[3] = r1 ? factor_beta2(g, sig_old, v1) : -1.0;
    }
    __syncthreads();
    const double sc = s_scal[0], sig = s_scal[1];
    if (s_scal[3] >= 0.0) {  // (workgroup-uniform) the rank-one step: Sigma is final (not rescaled), d still holds x - mu'
        const double beta2 = s_scal[3];
        const bool done = factor_rank_one_as<WP, PANELS>(a, m, beta2, factor_w_scale(g, sig), A, d, va, vb, s_scal);
        if (tid == 0) {
            if (!done) a.fvalid[m] = 0;  // the old factor stays in force; the next adapting iteration is full
            atomicAdd((unsigned long long *)&a.fcount[done ? 0 : 3], 1ull);
        }
        return;
    }
    for (int i = gi; i < Nv; i += 16)
        for (int j = gk; j < Nv; j += 16) {
            const size_t e = (size_t)i * Nv + j;
            double v = A[e];
            if (sc != 1.0) { v = v * sc; cov[e] = v; }  // (a covariance of norm > A1 = 1e14: never with sane inputs)
            A[e] = (v + (i == j ? a.epsi2 : 0.0)) * sig;
        }
    __syncthreads();
#ifdef TAMCMC_PROBE
    if (a.probe == 3) return;
#endif
    // Cholesky in place (lower triangle of A).  A matrix that is not positive definite (possible only while gamma = c0/(1+i) > 1,
    // i.e. adaptation before iteration c0) keeps the PREVIOUS factor -- the host engine does the same (host_mala.cpp::factor); the
    // reference hands Eigen's partial result on.  Every element sees the operations of the right-looking algorithm in its order
    // (A_ik -= L_ij L_kj for j ascending, then scaled by 1/d_kk), the host engine's factor to 1-2 ulp (round 3: reciprocal square roots
    // in the panels' diagonal blocks; the sqrt / divide sequence of the host engine was the factorisation's serial chain):
    //   * panels of NB columns: the NB x NB diagonal block is factored by NB lanes of one wave (rows in registers, pivots by
    //     shuffles, no workgroup barrier inside); the panel's columns below it are one forward substitution per row, a row per lane;
    //     then all lanes apply the NB columns to the trailing block in one sweep (a 16 x 16 grid over rows x columns, L_i,panel in
    //     registers along a row).  3 barriers per panel instead of 3 per column; the serial chain is sqrt -> divide per column.
    constexpr int NB = 8;
    bool pd = true;  // positive definite so far
    int j0 = 0;      // columns done by panels
    const int ti = tid >> 4, tk = tid & 15;
    if constexpr (PANELS) {
        if (tid == 0) s_scal[0] = 0.0;  // "not positive definite" flag
        __syncthreads();
        // (1) a panel's NB x NB diagonal block, by the first NB lanes of wave 0 (lane r = row p0+r in registers; pivots by readlane);
        //     called by the whole of wave 0
        auto diag_block = [&](const int p0) __attribute__((always_inline)) {
            double r[NB];
            const int row = p0 + tid;
            static_for<NB>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                r[c] = (tid < NB) ? A[(size_t)row * Nv + p0 + c] : 0.0;
            });
            bool bad = false;
            static_for<NB>([&](auto jc) {
                constexpr int jj = decltype(jc)::value;
                if (!bad) {  // wave-uniform
                    const double ajj = lane_value<jj>(r[jj]);
                    if (!(ajj > 0.0)) bad = true;
                    else {
                        // 1/sqrt(a_jj): v_rsq_f64 seed + two Newton steps (the serial chain of the factorisation is this step, once per
                        // column: an IEEE sqrt followed by an IEEE divide is ~5x as long); the column is scaled by it, the diagonal is
                        // a_jj / sqrt(a_jj) with one correction step.  1-2 ulp from the sqrt / divide factor of the host engine
                        double y = __builtin_amdgcn_rsq(ajj);
                        y = fma(y, fma(-ajj * y, 0.5 * y, 0.5), y);
                        y = fma(y, fma(-ajj * y, 0.5 * y, 0.5), y);
                        double djj = ajj * y;
                        djj = fma(fma(-djj, djj, ajj), 0.5 * y, djj);
                        if (tid > jj) r[jj] = r[jj] * y;
                        else if (tid == jj) { r[jj] = djj; d[p0 + jj] = y; }  // (d[] is free since the covariance update: reciprocal pivots)
                        static_for<NB - 1 - jj>([&](auto kc) {
                            constexpr int kk = jj + 1 + decltype(kc)::value;
                            const double lk = lane_value<kk>(r[jj]);  // L_(p0+kk),jj
                            if (tid >= kk) r[kk] = r[kk] - r[jj] * lk;
                        });
                    }
                }
            });
            if (bad) { if (tid == 0) s_scal[0] = 1.0; }
            else if (tid < NB)
                static_for<NB>([&](auto cc) {
                    constexpr int c = decltype(cc)::value;
                    if (c <= tid) A[(size_t)row * Nv + p0 + c] = r[c];
                });
        };
        // (2) the panel's columns below the block, one row per lane: L_i,jj = (A_i,jj - sum_{j' < jj} L_i,j' L_jj,j') / d_jj
        auto below_block = [&](const int p0) __attribute__((always_inline)) {
#pragma clang loop unroll(disable)
            for (int i = p0 + NB + tid; i < Nv; i += TB) {
                double li[NB], Ld[NB][NB];  // the row's panel entries and the diagonal block: every LDS read is requested before the first use
                static_for<NB>([&](auto cc) {
                    constexpr int c = decltype(cc)::value;
                    li[c] = A[(size_t)i * Nv + p0 + c];
                    static_for<c>([&](auto qc) {
                        constexpr int q = decltype(qc)::value;
                        Ld[c][q] = A[(size_t)(p0 + c) * Nv + p0 + q];
                    });
                    Ld[c][c] = d[p0 + c];  // reciprocal pivot (diag_block)
                });
                static_for<NB>([&](auto jc) {
                    constexpr int jj = decltype(jc)::value;
                    static_for<jj>([&](auto qc) {
                        constexpr int q = decltype(qc)::value;
                        li[jj] = li[jj] - li[q] * Ld[jj][q];
                    });
                    li[jj] = li[jj] * Ld[jj][jj];
                });
                static_for<NB>([&](auto cc) {
                    constexpr int c = decltype(cc)::value;
                    A[(size_t)i * Nv + p0 + c] = li[c];
                });
            }
        };
        // (3) the panel's NB columns applied to columns kb..ke-1 of the trailing block (rows i >= kb, columns <= i); the calling lanes
        //     form an RS x CS grid (ri, rk)
        auto trailing = [&](const int p0, const int kb, const int ke, const int ri, const int rk, auto rs_c, auto cs_c) __attribute__((always_inline)) {
            constexpr int RS = decltype(rs_c)::value, CS = decltype(cs_c)::value;
#pragma clang loop unroll(disable)
            for (int i = kb + ri; i < Nv; i += RS) {
                double li[NB];
                static_for<NB>([&](auto cc) {
                    constexpr int c = decltype(cc)::value;
                    li[c] = A[(size_t)i * Nv + p0 + c];
                });
                const int kend = i < ke - 1 ? i : ke - 1;  // last column of the row
                int k = kb + rk;
#pragma clang loop unroll(disable)
                for (; k + CS <= kend; k += 2 * CS) {  // two columns per trip: their LDS reads are in flight together (one wave per SIMD here)
                    double v0 = A[(size_t)i * Nv + k], v1 = A[(size_t)i * Nv + k + CS], l0[NB], l1[NB];
                    static_for<NB>([&](auto cc) {
                        constexpr int c = decltype(cc)::value;
                        l0[c] = A[(size_t)k * Nv + p0 + c];
                        l1[c] = A[(size_t)(k + CS) * Nv + p0 + c];
                    });
                    static_for<NB>([&](auto cc) {
                        constexpr int c = decltype(cc)::value;
                        v0 = v0 - li[c] * l0[c];
                        v1 = v1 - li[c] * l1[c];
                    });
                    A[(size_t)i * Nv + k] = v0;
                    A[(size_t)i * Nv + k + CS] = v1;
                }
                if (k <= kend) {
                    double v = A[(size_t)i * Nv + k];
                    static_for<NB>([&](auto cc) {
                        constexpr int c = decltype(cc)::value;
                        v = v - li[c] * A[(size_t)k * Nv + p0 + c];
                    });
                    A[(size_t)i * Nv + k] = v;
                }
            }
        };
        // Schedule: the next panel's diagonal block (the serial sqrt -> divide chain) is factored by wave 0 WHILE waves 1-3 apply the
        // current panel to the rest of the trailing block; only the next panel's own NB columns are updated ahead of it by all lanes.
#pragma clang loop unroll(disable)
        for (int p = -NB;;) {  // p: the panel being applied (none yet on the first trip, which only factors block 0)
            const int c0 = p + NB;
#ifdef TAMCMC_PROBE
            long pt0 = (long)wall_clock64(), pt1 = pt0;
#endif
            if (p >= 0) {
                below_block(p);
                __syncthreads();
#ifdef TAMCMC_PROBE
                pt1 = (long)wall_clock64();
#endif
                trailing(p, c0, c0 + NB, tid >> 3, tid & 7, std::integral_constant<int, TB / 8>{}, std::integral_constant<int, 8>{});
                __syncthreads();
            }
            j0 = c0;
            if (c0 + NB > Nv) break;  // fewer than NB columns left: the slice above was the whole trailing block
#ifdef TAMCMC_PROBE
            long pt2 = (long)wall_clock64();
#endif
            if (tid < 64) diag_block(c0);
            else if (p >= 0)
                trailing(p, c0 + NB, Nv, (tid - 64) >> 4, tid & 15, std::integral_constant<int, (TB - 64) / 16>{}, std::integral_constant<int, 16>{});
            __syncthreads();
#ifdef TAMCMC_PROBE
            if (m == 0 && tid == 0) {
                const long pt3 = (long)wall_clock64();
                a.counters[4] += pt1 - pt0; a.counters[5] += pt2 - pt1; a.counters[6] += pt3 - pt2; a.counters[7] += 1;
            }
#endif
            if (s_scal[0] != 0.0) { pd = false; break; }  // every lane leaves together, L is not touched
            p = c0;
        }
    }
    // the columns the panels leave (fewer than NB; all of them for wide proposals, whose work matrix is in device memory): one per step
#pragma clang loop unroll(disable)
    for (int j = j0; j < Nv && pd; j++) {
        const double ajj = A[(size_t)j * Nv + j];  // workgroup-uniform (its last update was before the previous step's closing barrier)
        if (!(ajj > 0.0)) { pd = false; break; }   // every lane leaves together, L is not touched
        const double djj = sqrt(ajj);
        if (tid == 0) d[j] = djj;                  // the new diagonal is parked in d[] (free since the covariance update)
        for (int i = j + 1 + tid; i < Nv; i += TB) A[(size_t)i * Nv + j] = A[(size_t)i * Nv + j] / djj;
        __syncthreads();
        for (int i = j + 1 + ti; i < Nv; i += 16) {
            const double lij = A[(size_t)i * Nv + j];
            for (int k = j + 1 + tk; k <= i; k += 16) A[(size_t)i * Nv + k] = A[(size_t)i * Nv + k] - lij * A[(size_t)k * Nv + j];
        }
        __syncthreads();
    }
    if (pd)
        for (int j = j0 + tid; j < Nv; j += TB) A[(size_t)j * Nv + j] = d[j];
    __syncthreads();
#ifdef TAMCMC_PROBE
    if (a.probe == 4) return;
#endif
    double *LT = a.LT + (size_t)m * Nv * Nv;  // the factor transposed (row k of LT = column k of L), written in 128-byte runs
    if (pd)
        for (int k = gi; k < Nv; k += 16)
            for (int i = gk; i < Nv; i += 16) LT[(size_t)k * Nv + i] = (k <= i) ? A[(size_t)i * Nv + k] : 0.0;
    if (tid == 0) {  // marked valid iff the matrix was positive definite; a full step in a rank-one slot of the schedule was forced
        a.fvalid[m] = pd ? 1 : 0;
        atomicAdd((unsigned long long *)&a.fcount[fmode == 2 ? 2 : 1], 1ull);
    }
    __syncthreads();
}
// A, d: the work matrix [Nv x Nv] and vector [Nv] -- in LDS when a.chol_in_lds (then va, vb are two more LDS vectors [Nv] of the caller),
// else the chain's slice of the scratch, [Nv^2 + 3 Nv] (va, vb are its tail).
__device__ __forceinline__ void adapt_chain(const DevSamplerArgs &a, int m, long itp, const double *vars, double Pm, double *A, double *d, double *s_red,
                            double *s_scal, int fmode, double *va, double *vb) {
    typedef double __attribute__((address_space(3))) *lds_dp_t;
    typedef double __attribute__((address_space(1))) *dev_dp_t;
    if (a.chol_in_lds) adapt_chain_as<lds_dp_t, true>(a, m, itp, vars, Pm, (lds_dp_t)A, (lds_dp_t)d, s_red, s_scal, fmode, (lds_dp_t)va, (lds_dp_t)vb);
    else adapt_chain_as<dev_dp_t, false>(a, m, itp, vars, Pm, (dev_dp_t)A, (dev_dp_t)d, s_red, s_scal, fmode, (dev_dp_t)(d + a.Nv), (dev_dp_t)(d + 2 * a.Nv));
}

// z ~ N(0, I) of (chain, iteration) into LDS (ends without a barrier) and row i of L z (MALA.cpp:348-355)
__device__ __forceinline__ void normals_into(const DevSamplerArgs &a, int chain, long it, double *s_z) {
    for (int k2 = threadIdx.x; 2 * k2 < a.Nv; k2 += (int)blockDim.x) {
        double z0, z1;
        rng_normal2(a.seed, RNG_PROPOSAL, (uint32_t)chain, (uint64_t)it, (uint32_t)k2, z0, z1);
        s_z[2 * k2] = z0;
        s_z[2 * k2 + 1] = z1;
    }
}
__device__ __forceinline__ double Lz_row(const DevSamplerArgs &a, int chain, int i, const double *s_z) {
    const double *LT = a.LT + (size_t)chain * a.Nv * a.Nv;
    double s = 0;
    for (int k = 0; k <= i; k++) s = s + LT[(size_t)k * a.Nv + i] * s_z[k];
    return s;
}

// The same rows of L z with the loads of a batch issued before the first use (a row's sum stays in ascending k, the order of Lz_row):
// lane i owns rows i and i+64.  A wave on its own has no other wave's loads to hide behind.
__device__ __forceinline__ void Lz_rows_wave(const DevSamplerArgs &a, int chain, const double *s_z, double *out) {
    constexpr int NB = 8;
    const int Nv = a.Nv, lane = threadIdx.x;
    const double *LT = a.LT + (size_t)chain * Nv * Nv;
#pragma clang loop unroll(disable)
    for (int i = lane; i < Nv; i += 64) {
        double s = 0;
        int k0 = 0;
#pragma clang loop unroll(disable)
        for (; k0 + NB <= i + 1; k0 += NB) {  // full batches: NB independent loads, then the NB terms in order
            double l[NB];
#pragma unroll
            for (int u = 0; u < NB; u++) l[u] = LT[(size_t)(k0 + u) * Nv + i];
#pragma unroll
            for (int u = 0; u < NB; u++) s = s + l[u] * s_z[k0 + u];
        }
#pragma clang loop unroll(disable)
        for (; k0 <= i; k0++) s = s + LT[(size_t)k0 * Nv + i] * s_z[k0];
        out[i] = s;
    }
}

// x' = x + L z from the state in LDS (s_vars/s_params) and the normals in s_z (or the rows lz computed ahead), scattered into the
// parameter vector (update_params_with_vars); both also written to pv / pp.  Called after a barrier; ends without one.
__device__ __forceinline__ void propose_position(const DevSamplerArgs &a, int chain, double *pv, double *pp, double *s_vars, double *s_params,
                                                 const double *s_z, const double *lz) {
    const int Np = a.desc.Np, Nv = a.Nv, tid = threadIdx.x;
    for (int i = tid; i < Nv; i += TB) {  // lane i owns row i: reads s_vars[i] only, every s_z[k]
        const double s = lz ? lz[i] : Lz_row(a, chain, i, s_z);
        const double v = s_vars[i] + 0.0 + s;
        s_vars[i] = v;
        pv[i] = v;
    }
    __syncthreads();
    for (int k = tid; k < Nv; k += TB) s_params[a.index_to_relax[k]] = s_vars[k];  // update_params_with_vars
    __syncthreads();
    for (int i = tid; i < Np; i += TB) pp[i] = s_params[i];
}

// Gaussian-envelope models (ids 0 / 1): the front end of a proposal -- its log-prior by lane 0 (pr::prior_serial in double, what the
// gradient batch's k_env_prior runs) while the first lane of wave 1 forms the row the evaluation reads (env_row, envelope_row.h).  No
// table and no unpack; a dead prior or a status that is not OK is mh_outcome's business, whatever the row then holds.  s_params
// complete (a barrier) before the call; ends without a barrier.
__device__ __forceinline__ void env_front(const ModelDesc &d, const double *s_params, EnvRow *row, double *logPr_out, int *status_out) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        int st = TAMCMC_OK;
        *logPr_out = (double)pr::prior_serial(d.prior_class, s_params, nullptr, (long)d.Np, d.priors, d.priors_switch, nullptr, &st);
        *status_out = st;
    } else if (tid == 64) env_row(d.model_id, s_params, *row);
}

// Proposal of iteration `it` for `chain` from the state in LDS (s_vars/s_params): x' = x + L z (MALA.cpp:348-355), L =
// chol((Sigma+eps2) sigma) stored transposed, same Philox streams as the host engine; log-prior; params' -> multiplet table
// written into slot `slot` of the likelihood kernel's input block.  Ends without a barrier.  (B): 256 threads.
__device__ __forceinline__ void propose_common(const DevSamplerArgs &a, const UnpackLds &U, int chain, long it, int slot, double *pv, double *pp,
                               double *logPr_out, int *status_out, double *s_vars, double *s_params, double *s_z, const double *lz = nullptr,
                               const rgb::Slice *rs = nullptr, int rb = 0) {
    const int Np = a.desc.Np, tid = threadIdx.x;
    const bool rgb = is_rgb_model(a.desc.model_id), env = is_envelope_model(a.desc.model_id);
    if (!lz) normals_into(a, chain, it, s_z);
    if (!rgb && !env) unpack_begin(a.desc, U);
    else __syncthreads();
    propose_position(a, chain, pv, pp, s_vars, s_params, s_z, lz);
    if (env) {  // ids 0 / 1: the kernels enqueued right behind this launch (envelope_stage_enqueue) evaluate the row
        env_front(a.desc, s_params, a.env_rows + slot, logPr_out, status_out);
        return;
    }
    if (rgb) {
        // red-giant models (ids 25 / 27): the table needs the mixed-mode solver -- the kernels enqueued right behind this launch
        // (rgb_device_stage) build it.  Here: the red-giant front end (rgb_front.h, shared with the gradient batch's k_fd_rgb_perturb) on
        // this kernel's schedule: the generic prior terms by all 256 lanes, then the serial tail on lane 0 while wave 1 runs the scalar
        // unpack of the proposal, published into the group's workspace slice.
        __shared__ rgb::FrontLds F;
        mt::xreal *terms = (mt::xreal *)U.poly;  // (the polynomial tables' LDS is not used by these models; xreal = double on the device)
        const bool spread = a.desc.prior_class == 4 && (size_t)Np * sizeof(mt::xreal) <= sizeof(mt::PolyTab);
        if (tid == 0) *U.status = TAMCMC_OK;
        __syncthreads();
        if (spread)
            for (int i = tid; i < Np; i += TB) {
                int st = TAMCMC_OK;
                terms[i] = pr::generic_prior_term(s_params, Np, a.desc.priors, a.desc.priors_switch, i, &st);
                if (st != TAMCMC_OK) *U.status = st;
            }
        __syncthreads();
        if (tid == 0) rgb::front_prior_serial(a.desc, s_params, spread ? terms : nullptr, *U.status, F);
        else if ((tid >> 6) == 1) rgb::front_unpack(a.desc, s_params, *rs, F);
        __syncthreads();
        const double lp = F.lp;
        const int stp = F.stp;
        if (tid == 0 && (stp != TAMCMC_OK || lp == -INFINITY || isnan(lp))) {  // model_def.cpp:472,476-480 skips the model: nothing to solve
            F.P.Lp = 0; F.P.Lg = 0; F.P.status = stp != TAMCMC_OK ? stp : TAMCMC_ERR_BAD_ARG;
            F.R.status = F.P.status; F.R.Nfl0 = F.R.Nfl2 = F.R.Nfl3 = 0; F.R.bias_n = 0;
            F.noise[0] = 1.0;
            F.hn[0] = 0; F.hn[1] = 1;
        }
        __syncthreads();
        rgb::front_publish<TB>(F, *rs, rb, slot, a.desc.stride, a.noise, a.nh, a.nn);
        if (tid == 0) {
            *logPr_out = lp;
            *status_out = stp;
        }
        return;
    }

    // ---- log-prior, then params' -> multiplet table written into the likelihood kernel's input block ----
    TablePtrs T;
    T.mults = a.mults; T.pairs = a.pairs; T.nh = a.nh; T.nn = a.nn; T.noise = a.noise;
    T.bg = a.bg; T.ntiles = a.ntiles; T.tile_bins = a.tile_bins;
    // four roles beside each other (dev_unpack.h): prior terms + background tiles | table rows | shared scalars + m-visibilities
    const double logPr = wg_log_prior(a.desc, s_params, U, true, true, &T, slot);
    const bool live = (logPr != -INFINITY) && !isnan(logPr);  // model_def.cpp:472,476-480
    wg_unpack(a.desc, s_params, U, slot, T, live, true, true);
    if (tid == 0) {
        *logPr_out = logPr;
        *status_out = *U.status;
    }
}

// the swap pair of iteration i (step_schedule.h) from an argument block in either address space
template <class AT>
__device__ __forceinline__ bool is_swap_iter(const AT &a, long i) {
    return is_swap_iteration(a.C, a.dN_mixing, i);
}
template <class AT>
__device__ __forceinline__ int swap_first(const AT &a, long i, double *u_out) {
    return swap_draw(a.seed, a.C, i, u_out);
}

// Parallel tempering (MALA.cpp:397-461) on the pair's outcomes AFTER their MH tests: does the pair swap, and what does each side
// then hold as tempered logL / prior / posterior.  oA, oB are updated in place; returns 1 when swapped.
template <class AT>
__device__ __forceinline__ int resolve_swap(const AT &a, int A, double u, AcceptOut &oA, AcceptOut &oB) {
    const int B = A + 1;
    const double LA = oA.logL, LB = oB.logL;
    const double LA_TB = LA * a.Tcoefs[A] / a.Tcoefs[B];
    const double LB_TA = LB * a.Tcoefs[B] / a.Tcoefs[A];
    const double e = exp(LA_TB + LB_TA - LA - LB);
    const double rT = fmin(1.0, e);
    if (!(u <= rT)) return 0;
    const double prA = oA.logPr, prB = oB.logPr;
    oA.logL = LB_TA; oA.logPr = prB; oA.logPost = LB_TA + prB;      // A <- B, re-tempered (MALA.cpp:431-435)
    // swap_rule 1 (MALA.cpp:433,444 as executed): B's stored posterior carries B's own old prior
    oB.logL = LA_TB; oB.logPr = prA; oB.logPost = LA_TB + (a.swap_rule == 1 ? prB : prA);
    return 1;
}

// (0) of the lockstep scheme for chain m, by a whole 256-thread workgroup: the MH test of the pending iteration it-1 (own chain; the
// swap partner's too when chain m is in the swap pair), the adjacent-pair parallel-tempering swap, the chain's new current state into
// the OTHER parity buffer and into LDS (s_vars / s_params; with learn_pending the chain's own position after the test into s_z), the
// record.  pending = 0: the state is carried over as it is.  `writer`: this workgroup writes the chain's state, counters and records --
// every workgroup of k_iterate; of the workgroups that k_env_step (dev_env_step_impl.h) runs per chain, the first tile's only.
__device__ __forceinline__ void settle_chain(const DevSamplerArgs &a, int m, long it, int P, int pending, long rec, int learn_pending, bool writer,
                                             double *s_vars, double *s_params, double *s_z, double *s_red, AcceptOut *s_own_p, AcceptOut *s_partner_p) {
    const int Np = a.desc.Np, Nv = a.Nv, C = a.C, tid = threadIdx.x;
    const int Q = P ^ 1;
    AcceptOut &s_own = *s_own_p, &s_partner = *s_partner_p;
    const double *curv = a.vars_cur + (size_t)P * C * Nv, *curp = a.params_cur + (size_t)P * C * Np;
    const double *prpv = a.vars_prop + (size_t)P * C * Nv, *prpp = a.params_prop + (size_t)P * C * Np;
    double *newv = a.vars_cur + (size_t)Q * C * Nv, *newp = a.params_cur + (size_t)Q * C * Np;
    if (pending) {
        const long itp = it - 1;
        accept_result(a, m, itp, P, s_red, &s_own);
        int src = m;
        AcceptOut mine = s_own;
        // parallel tempering (MALA.cpp:397-461): adjacent pair, tempered log-likelihoods after the MH tests
        if (is_swap_iter(a, itp)) {
            double u;
            const int A = swap_first(a, itp, &u);
            const int B = A + 1;
            if (m == A || m == B) {  // workgroup-uniform branch
                const int partner = (m == A) ? B : A;
                accept_result(a, partner, itp, P, s_red, &s_partner);
                AcceptOut oA = (m == A) ? s_own : s_partner, oB = (m == A) ? s_partner : s_own;
                const int swapped = resolve_swap(a, A, u, oA, oB);
                if (swapped) { src = partner; mine = (m == A) ? oA : oB; }
                if (m == A && tid == 0 && writer) {  // (chain groups: launches of different iterations may overlap)
                    atomicAdd((unsigned long long *)&a.counters[2], 1ull);
                    if (swapped) atomicAdd((unsigned long long *)&a.counters[3], 1ull);
                }
            }
        }
        const int src_acc = (src == m) ? s_own.acc : s_partner.acc;
        const double *sv = (src_acc ? prpv : curv) + (size_t)src * Nv;
        const double *sp = (src_acc ? prpp : curp) + (size_t)src * Np;
        for (int i = tid; i < Nv; i += TB) { const double v = sv[i]; s_vars[i] = v; if (writer) newv[(size_t)m * Nv + i] = v; }
        for (int i = tid; i < Np; i += TB) { const double v = sp[i]; s_params[i] = v; if (writer) newp[(size_t)m * Np + i] = v; }
        if (learn_pending) {  // the adaptation sees the chain's OWN position after the MH test, before the swap
            const double *ov = (s_own.acc ? prpv : curv) + (size_t)m * Nv;
            for (int i = tid; i < Nv; i += TB) s_z[i] = ov[i];
        }
        if (tid == 0 && writer) {
            a.logL_cur[Q * C + m] = mine.logL;
            a.logPr_cur[Q * C + m] = mine.logPr;
            a.logPost_cur[Q * C + m] = mine.logPost;
            // a swap exchanges the pair's moved / Pmove entries too (MALA.cpp:425-446): what is recorded is the partner's
            a.moved[m] = (src == m) ? s_own.acc : s_partner.acc;
            a.Pmove[m] = (src == m) ? s_own.r : s_partner.r;
            if (m == 0 && a.moved[0]) a.counters[1] += 1;
            a.counters[8 + m] += a.moved[m];  // per-chain count of recorded moves (the acceptance diagnostic, outputs.cpp:1824-1858)
            if (m == 0) a.counters[0] = it;
            if (a.stats && rec >= 0) {  // update_buffer_stat_criteria (MALA.cpp:708)
                double *r = a.stats + ((size_t)rec * C + m) * 3;
                r[0] = mine.logL; r[1] = mine.logPr; r[2] = mine.logPost;
            }
        }
        __syncthreads();
        if (a.samples && rec >= 0 && writer)  // update_buffer_params (MALA.cpp:710)
            for (int i = tid; i < Nv; i += TB) a.samples[((size_t)rec * C + m) * Nv + i] = s_vars[i];
    } else {
        for (int i = tid; i < Nv; i += TB) { const double v = curv[(size_t)m * Nv + i]; s_vars[i] = v; if (writer) newv[(size_t)m * Nv + i] = v; }
        for (int i = tid; i < Np; i += TB) { const double v = curp[(size_t)m * Np + i]; s_params[i] = v; if (writer) newp[(size_t)m * Np + i] = v; }
        if (tid == 0 && writer) {
            a.logL_cur[Q * C + m] = a.logL_cur[P * C + m];
            a.logPr_cur[Q * C + m] = a.logPr_cur[P * C + m];
            a.logPost_cur[Q * C + m] = a.logPost_cur[P * C + m];
        }
    }
}

// ===============================================================================================================
// (B) LOCKSTEP.  ONE kernel per MCMC iteration besides the likelihood kernel.  Workgroup m:
//   (0) settles the pending iteration it-1 for chain m: MH test (own chain; the swap partner's too when chain m is in the
//       swap pair), adjacent-pair parallel-tempering swap, writes the chain's new current state into the OTHER parity
//       buffer (no workgroup ever writes what another one reads), records the sample, adapts the proposal law;
//   (1) proposes iteration `it` from that state: x' = x + L z, log-prior, params' -> multiplet table.
template <bool PROPOSE>
__global__ void __launch_bounds__(TB) k_iterate(const DevSamplerArgs a, const long it, const int P, const int pending,
                                               const long rec, const int learn_pending, double *scratch, const int c_off,
                                               const int nmain, const int pre_flags, const rgb::Slice rs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int Np = a.desc.Np, Nv = a.Nv, C = a.C;
    if ((int)blockIdx.x >= nmain) {
        // spare workgroup (launched while no adaptation touches L): L z of iteration it+1 for chain c_off + blockIdx.x - nmain
        const int ch = c_off + (int)blockIdx.x - nmain;
        double *z = (double *)s_raw;
        normals_into(a, ch, it + 1, z);
        __syncthreads();
        double *dst = a.lz + ((size_t)((it + 1) & 1) * C + ch) * Nv;
        for (int i = threadIdx.x; i < Nv; i += TB) dst[i] = Lz_row(a, ch, i, z);
        return;
    }
    double *s_params = (double *)s_raw;          // [Np]   current, then proposed parameter vector
    double *s_vars = s_params + Np;              // [Nv]   current, then proposed variables
    double *s_z = s_vars + Nv;                   // [Nv+1] normals / post-test position for the adaptation
    const UnpackLds U = carve_unpack_lds((unsigned char *)(s_z + Nv + 1));
    double *s_red = U.red;
    double *s_A = (double *)(((uintptr_t)(s_z + Nv + 1) + unpack_lds_bytes() + 15) & ~(uintptr_t)15);  // [Nv*Nv + Nv] when learning in LDS
    __shared__ AcceptOut s_own, s_partner;
    __shared__ double s_scal[4];

    const int m = blockIdx.x + c_off;  // c_off: first chain of this launch's chain group
    const int Q = P ^ 1;

    // ------------------------------------------------------------------ (0) settle the pending iteration
    settle_chain(a, m, it, P, pending, rec, learn_pending, true, s_vars, s_params, s_z, s_red, &s_own, &s_partner);
    if (pending && learn_pending) {
        double *Aw = a.chol_in_lds ? s_A : scratch + (size_t)m * ((size_t)Nv * Nv + 3 * Nv);
        // (the rank-one step's vectors: s_z is free once the deviation is formed; the unpack's LDS behind its reduction slots is idle until
        // the proposal -- (40 + 224) doubles at least, and a work matrix in LDS has Nv <= 138)
        static_assert(sizeof(mt::PolyTab) >= 160 * sizeof(double), "room for a coefficient vector of a work matrix that fits in LDS");
        adapt_chain(a, m, it - 1, s_z, s_own.r, Aw, Aw + (size_t)Nv * Nv, s_red, s_scal, learn_pending, s_z, U.w);
    }
    if (!PROPOSE) return;
    __syncthreads();

    // ------------------------------------------------------------------ (1) propose iteration `it`
    propose_common(a, U, m, it, m, a.vars_prop + (size_t)Q * C * Nv + (size_t)m * Nv, a.params_prop + (size_t)Q * C * Np + (size_t)m * Np,
                   a.logPr_prop + Q * C + m, a.status_prop + Q * C + m, s_vars, s_params, s_z,
                   (pre_flags & 1) ? a.lz + ((size_t)(it & 1) * C + m) * Nv : nullptr, &rs, (int)blockIdx.x);
}
