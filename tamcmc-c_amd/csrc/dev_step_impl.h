// dev_step_impl.h -- device code of the fused step (included by dev_sampler.hip, inside its anonymous namespace, after
// dev_iterate_impl.h): the argument block of the scheme, the decision every workgroup takes for itself (quick_decide, decide), the commit
// workgroups, the candidate roles, the L z blocks, the kernel k_step and its launcher.  The scheme is described at the head of
// dev_sampler.hip; the order of the definitions and the noinline boundaries are part of the kernel's register budget (168 VGPRs, three
// waves per SIMD).

// ===============================================================================================================
// (A) FUSED STEP.
struct FusedArgs {
    int NS;                // candidate slots per iteration: 2C + 8 (two blocks of four extra slots for a swap pair's cross candidates)
    int xsplit;            // first chain of the second chain group (C: none).  A chain's cross candidates after a swap live in extra block
                           // (chain >= xsplit): the two groups' launches run on different streams, possibly several iterations apart,
                           // and must never write what the other one still reads
    // candidates of iteration i live in candidate set i mod 3: [3][NS]...  (launch i reads the sets of iterations i-1 and i and writes
    // the set of iteration i+1)
    double *cand_vars, *cand_params;
    double *cand_logPr;                // [3][NS][2] the two halves of the log-prior's additive terms (wave_log_prior_part), added in order
    int *cand_rej;                     // [3][NS]    a hard constraint fails: the log-prior is -inf
    int *cand_stP, *cand_stR;          // [3][NS][2], [3][NS] status of the two prior roles / the rows role
    tamcmc_multiplet *mults;           // [3][NS][per]
    int *pairs, *nh, *nn;              // [3][2 NS], [3][NS], [3][NS]
    double *noise;                     // [3][NS][stride]
    double *bg;                        // [3][NS][ntiles][8] or nullptr
    // per chain, by the parity of the iteration: written by the launch of that iteration (commit_chain), read by the next one
    int *slot;                         // [2][C]   table slot of chain m's proposal at that iteration
    double *prop_logPr;                // [2][C]   that proposal's log-prior ...
    int *prop_st;                      // [2][C]   ... and status (prior role's, else rows role's)
    double *quick;                     // [2][C][QN] that iteration's MH and swap tests as thresholds on the sums of the partials (quick_decide)
    double *part;                      // [2][C][ntiles][2] the tiles' partial sums of that iteration
    double *lz;                        // [2][C][Nv] L z of chain m for the iteration of that parity, computed one launch ahead
    // per chain, by the iteration mod 3 (like the candidate sets): the tiles of launch i ADD c = part[..][0] + part[..][1] and |c| into
    // set i mod 3, launch i+1 reads that set (quick_decide), the chain's commit workgroup of launch i zeroes set (i+1) mod 3 -- last read
    // by launch i-1 -- and the closing launch of a stretch all three.  128 bytes per (set, chain), 128-byte aligned: no two chains share a
    // cache line.  QK keys only spread the atomics over as many addresses (the tile workgroup's id & 7); every reader sums all of them
    double *qacc;                      // [3][C][QK][2] sum of c, sum of |c|
    // quick_decide's safety margin (1e-11; +inf under TAMCMC_OPT_QUICK_DECIDE = 1: every margin test answers "undecided") and what the
    // tests read back (tamcmc_sampler_get_info): [0] fallbacks to decide() taken by the likelihood tiles, counted by each chain's tile 0;
    // [1] tests of chains outside a swap pair that those tiles decided from a kind-2 record, counted by the chain's commit workgroup;
    // [2] tests that the shortcut decided OTHERWISE than the exact decide(), counted by the commit workgroup, which has both (0, or a bug)
    double qmargin;
    unsigned long long *qcount;
};

constexpr int QK = 8;  // keys per (set, chain) of FusedArgs::qacc
constexpr int QN = 8;  // doubles per quick record (quick_decide): S*, kind, -pl/T, logL held, [pair's first chain: log u_swap, TA/TB - 1, TB/TA - 1], slot
constexpr int ST_L = 1, ST_BR = 2, ST_ENTRY = 4, ST_LZ = 8, ST_FIRST = 16, ST_COMMIT = 32;

// The decide / commit functions are real calls (register budget of the tile path) and get the argument blocks as pointers to their
// device-memory image.  That image is written by the host only, and the pointer is the same in every lane: read through a wave-uniform
// pointer into constant memory, a field costs a scalar load (SGPR, scalar cache) instead of a flat vector load per lane, and the
// pointers found there are known to be global (global_load / global_store instead of flat_).
typedef DevSamplerArgs __attribute__((address_space(4))) ConstArgs;
typedef FusedArgs __attribute__((address_space(4))) ConstFused;
__device__ __forceinline__ const void __attribute__((address_space(4))) *uniform_ptr(const void *p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(v & 0xffffffffull)), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32));
    return (const void __attribute__((address_space(4))) *)(((unsigned long long)hi << 32) | lo);
}

// What chain m enters iteration `it` with -- the outcome of iteration it-1's MH test and swap (MALA.cpp:397-461, 490-551).
struct Decided {
    int slot;       // candidate slot (set it mod 3) of the chain's proposal at iteration `it`
    int src;        // chain whose post-test position the chain continues from: itself, or its swap partner
    int src_acc;    // 1: that position is src's proposal of iteration it-1 (candidate set (it-1) mod 3, slot src_ps); 0: what src held
    int src_par;    // parity of the state arrays that hold src's position (src_acc == 0) -- the previous iteration's, or, in the first
                    // launch of a stretch, this iteration's (the chains are settled)
    int src_ps;
    int swap_first; // first chain of iteration it-1's swap pair when chain m is in it, else -1
    int swapped;
    double r;       // move probability of src's test (a swap exchanges the pair's moved / Pmove entries too, MALA.cpp:425-446)
    AcceptOut o;    // the scalars the chain holds (re-tempered after a swap)
};

// Iteration it-1 of chain m decided by ONE wave from what launch it-1 left in memory: the tiles' partial sums (summed in k_finalize's
// order), the proposal's prior and status, the scalars the chain held.  Every workgroup of launch `it` that needs the outcome -- each
// likelihood tile of the chain (its table slot), the chain's commit workgroup, the candidate roles built on the chain's vectors --
// recomputes it from the same inputs: same result everywhere, no hand-off inside a launch (no tickets, no device-scope accesses), and no
// settle step at the end of the launch's critical path.  For the two chains of iteration it-1's swap pair both tests are evaluated
// (lanes 0 and 1) and the swap resolved.  Returns the slot; `out` (LDS, may be null) gets the rest, written by lane 0.
__device__ __attribute__((noinline)) int decide(const DevSamplerArgs *ga, const FusedArgs *gf, int m, long it, int q, int settled, Decided *out) {
    const ConstArgs &a = *(const ConstArgs *)uniform_ptr(ga);
    const ConstFused &f = *(const ConstFused *)uniform_ptr(gf);
    const int lane = threadIdx.x & 63, C = a.C;
    if (settled) {  // first launch of a stretch: nothing is pending, the chain's slot was named by the launch that settled it
        const int s = f.slot[q * C + m] & 0xffff;
        if (out && lane == 0) {
            Decided d;
            d.slot = s; d.src = m; d.src_acc = 0; d.src_par = q; d.src_ps = 0; d.swap_first = -1; d.swapped = 0; d.r = 0;
            d.o.acc = 0; d.o.r = 0; d.o.logL = 0; d.o.logPr = 0; d.o.logPost = 0;
            *out = d;
        }
        return s;
    }
    const int p = q ^ 1, ntiles = a.ntiles;
    const long itp = it - 1;
    int A = -1;
    double u = 0;
    if (is_swap_iter(a, itp)) A = swap_first(a, itp, &u);
    const bool in_pair = A >= 0 && (m == A || m == A + 1);
    const int j0 = in_pair ? A : m;
    const int jl = (in_pair && lane == 1) ? A + 1 : j0;  // lane 1 tests the pair's second chain, every other lane repeats lane 0
    // every load before any arithmetic (one memory round trip): the scalars of this lane's chain, the partial sums of one or two chains
    const int ps = f.slot[p * C + jl] & 0xffff, st = f.prop_st[p * C + jl];
    const double pl = f.prop_logPr[p * C + jl], hL = a.logL_cur[p * C + jl], hP = a.logPr_cur[p * C + jl], hQ = a.logPost_cur[p * C + jl];
    const double Tj = a.Tcoefs[jl], il = a.init_logL[jl];
    const double *b0 = f.part + ((size_t)p * C + j0) * ntiles * 2;
    double S0, S1 = 0;
    if (ntiles <= TB) {  // the usual case, both chains' loads in flight together
        double v1[TB / 64], v2[TB / 64], w1[TB / 64], w2[TB / 64];
#pragma unroll
        for (int k = 0; k < TB / 64; k++) {
            const int t = k * 64 + lane;
            const bool in = t < ntiles;
            v1[k] = in ? b0[2 * t] : 0.0;
            v2[k] = in ? b0[2 * t + 1] : 0.0;
            w1[k] = (in && in_pair) ? b0[2 * (ntiles + t)] : 0.0;
            w2[k] = (in && in_pair) ? b0[2 * (ntiles + t) + 1] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < TB / 64; k++) { v1[k] = 0.0 + v1[k]; v2[k] = 0.0 + v2[k]; w1[k] = 0.0 + w1[k]; w2[k] = 0.0 + w2[k]; }  // (wave_partial_sum's first round)
        S0 = wave_sum_in_order(v1, v2);
        if (in_pair) S1 = wave_sum_in_order(w1, w2);
    } else {
        S0 = wave_partial_sum(b0, ntiles);
        if (in_pair) S1 = wave_partial_sum(b0 + (size_t)ntiles * 2, ntiles);
    }
    AcceptOut o = mh_outcome(a, jl, itp, (in_pair && lane == 1) ? S1 : S0, pl, st, hL, hP, hQ, Tj, il);
    AcceptOut o0, o1;
    o0.acc = __shfl(o.acc, 0, 64); o0.r = __shfl(o.r, 0, 64); o0.logL = __shfl(o.logL, 0, 64); o0.logPr = __shfl(o.logPr, 0, 64);
    o0.logPost = __shfl(o.logPost, 0, 64);
    const int ps0 = __shfl(ps, 0, 64);
    Decided d;
    d.swap_first = -1; d.swapped = 0;
    if (!in_pair) {
        d.slot = 2 * m + o0.acc; d.src = m; d.src_acc = o0.acc; d.src_par = p; d.src_ps = ps0; d.r = o0.r; d.o = o0;
    } else {
        o1.acc = __shfl(o.acc, 1, 64); o1.r = __shfl(o.r, 1, 64); o1.logL = __shfl(o.logL, 1, 64); o1.logPr = __shfl(o.logPr, 1, 64);
        o1.logPost = __shfl(o.logPost, 1, 64);
        const int ps1 = __shfl(ps, 1, 64);
        const int accA = o0.acc, accB = o1.acc;
        const double rA = o0.r, rB = o1.r;
        const int swapped = resolve_swap(a, A, u, o0, o1);  // (o0 = chain A's, o1 = chain B's: re-tempered in place)
        d.swap_first = A; d.swapped = swapped; d.src_par = p;
        const int B = A + 1;
        if (swapped) {  // each side continues from the other's post-test position: the extra candidate slots 2C .. 2C+3 (+4: second block)
            if (m == A) { d.slot = 2 * C + (A >= f.xsplit ? 4 : 0) + accB; d.src = B; d.src_acc = accB; d.src_ps = ps1; d.r = rB; d.o = o0; }
            else { d.slot = 2 * C + (B >= f.xsplit ? 4 : 0) + 2 + accA; d.src = A; d.src_acc = accA; d.src_ps = ps0; d.r = rA; d.o = o1; }
        } else {
            if (m == A) { d.slot = 2 * A + accA; d.src = A; d.src_acc = accA; d.src_ps = ps0; d.r = rA; d.o = o0; }
            else { d.slot = 2 * B + accB; d.src = B; d.src_acc = accB; d.src_ps = ps1; d.r = rB; d.o = o1; }
        }
    }
    if (out && lane == 0) *out = d;
    return d.slot;
}

// Chain m's workgroup of launch `it` (one wave): writes what iteration it-1 decided -- the chain's state for iteration `it` (parity q),
// the record of iteration it-1 (update_buffer_params / update_buffer_stat_criteria, MALA.cpp:708-710), the move flags and counters -- and,
// for the launch of iteration it+1, the slot, prior and status of the chain's proposal at iteration `it`.  With ST_COMMIT alone (after the
// last iteration of a stretch) the launch holds nothing else.
// (tiles: the launch holds the likelihood tiles of iteration `it`, which decided iteration it-1 themselves -- quick_decide)
//
// The chain's accumulators (FusedArgs::qacc) are this workgroup's too.  It asks the shortcut what the tiles of this launch asked it -- same
// function, same records, same accumulators -- and counts an answer that is not decide()'s (qcount[2]; the slot names the outcome of the
// test and of the swap as the chain sees them).  And it zeroes: launch `it` adds into set it mod 3 and reads set (it-1) mod 3, so set
// (it+1) mod 3, last read by the chain's launch it-1, is free -- 16 lanes, one store each, also in the first launch of a stretch.  The
// closing launch zeroes all three sets, for a next stretch that may start at any iteration; there the set it has just read is among
// them, and for a swap pair BOTH chains' workgroups would read both chains' sets: the pair's first chain asks for itself and zeroes both, the
// second does neither (nothing in a launch waits for anything else in it; the second chain's view of a stretch's LAST test is the one
// answer of the shortcut that goes unasked).
// (a function of its own that calls the leaf alone: what a caller keeps across a call lies above the callee's registers, and with a
// second decide() below commit_chain -- for the pair's second chain -- the kernel needs 180 of them and loses its third wave per SIMD)
__device__ int quick_decide_leaf(const DevSamplerArgs *ga, const FusedArgs *gf, int m, int q, int es, int pairA, Decided *out);
__device__ __attribute__((noinline)) void commit_sums(const DevSamplerArgs *ga, const FusedArgs *gf, int m, long it, int q, int settled, int tiles,
                                                      int slot, int swap_first) {
    const ConstArgs &a = *(const ConstArgs *)uniform_ptr(ga);
    const ConstFused &f = *(const ConstFused *)uniform_ptr(gf);
    const int lane = threadIdx.x, C = a.C;
    const int pairA = settled ? -1 : __builtin_amdgcn_readfirstlane(swap_first);
    const bool second = !tiles && pairA >= 0 && pairA != m;  // (closing launch: the pair's first chain does this chain's part)
    int differs = 0;
    if (!settled && !second) {
        const int es = (int)((it + 2) % 3);
        const int qs = quick_decide_leaf(ga, gf, m, q, es, pairA, nullptr);
        differs = (qs >= 0 && qs != slot) ? 1 : 0;
        if (lane == 0 && differs) atomicAdd(f.qcount + 2, 1ull);
    }
    // (after the reads above: in the closing launch the set they name is among those zeroed)
    const int z = lane;
    if (tiles) {
        if (z < 2 * QK) f.qacc[((size_t)((it + 1) % 3) * C + m) * (2 * QK) + z] = 0.0;
    } else if (!second && z < 3 * 2 * QK) {
        const size_t e = (size_t)(z / (2 * QK)) * C + m;
        f.qacc[e * (2 * QK) + z % (2 * QK)] = 0.0;
        if (pairA == m) f.qacc[(e + 1) * (2 * QK) + z % (2 * QK)] = 0.0;
    }
}
__device__ __attribute__((noinline)) void commit_chain(const DevSamplerArgs *ga, const FusedArgs *gf, int m, long it, int q, int settled, long rec,
                                                       int tiles, Decided *dec) {
    const int slot = decide(ga, gf, m, it, q, settled, dec);
    __syncthreads();
    commit_sums(ga, gf, m, it, q, settled, tiles, slot, dec->swap_first);
    const ConstArgs &a = *(const ConstArgs *)uniform_ptr(ga);
    const ConstFused &f = *(const ConstFused *)uniform_ptr(gf);
    const int lane = threadIdx.x, C = a.C, Nv = a.Nv, Np = a.desc.Np;
    const Decided d = *dec;
    if (lane == 0) {
        const size_t gs = (size_t)(it % 3) * f.NS + slot;
        const int stP0 = f.cand_stP[2 * gs], stP1 = f.cand_stP[2 * gs + 1], stR = f.cand_stR[gs];
        const double lp = f.cand_rej[gs] ? -INFINITY : f.cand_logPr[2 * gs] + f.cand_logPr[2 * gs + 1];
        const int stm = stP0 != TAMCMC_OK ? stP0 : (stP1 != TAMCMC_OK ? stP1 : stR);
        f.prop_logPr[q * C + m] = lp;
        f.prop_st[q * C + m] = stm;
        // The test of iteration `it` (mh_outcome) as a threshold on S = sum of the tiles' partials, for the next launch's quick_decide:
        // accept <=> log u <= -pl S / T + logPr - logPost_cur <=> S <= S*.  Everything but S is known here.
        double *w = f.quick + ((size_t)q * C + m) * QN;
        const double Tm = a.Tcoefs[m];
        double Sstar = 0, ok = -1;  // (-1: no shortcut, decide() it)
        double u, u1;
        rng_uniform2(a.seed, RNG_ACCEPT, (uint32_t)m, (uint64_t)it, 0, u, u1);
        if (stm == TAMCMC_OK && !(lp == -INFINITY || isnan(lp))) {
            const double cur = settled ? a.logPost_cur[q * C + m] : d.o.logPost;
            Sstar = -((log(u) - lp + cur) * Tm) / (double)a.pl;
            if (isfinite(Sstar)) ok = 1;
        } else if (u > 0.0) ok = 2;  // r = 0 whatever the sums (mh_outcome): rejected
        // (In practice kind 2 means "outside a prior's support".  A failed table cannot come from a proposal inside the priors for the
        // models that run fused: set_imin_imax fails only on a NaN width or splitting, or on a non-positive truncation parameter -- a
        // fixed input -- and a proposal is a finite sum of finite numbers.  tests/test_gpu_sampler.py counts the kind-2 tests it covers.)
        w[0] = Sstar; w[1] = ok; w[2] = -(double)a.pl / Tm; w[3] = settled ? a.logL_cur[q * C + m] : d.o.logL;
        double lus = 0, k1 = 0, k2 = 0;
        if (is_swap_iter(a, it)) {  // the swap test of iteration `it`, left by the pair's first chain: u <= exp(LA TA/TB + LB TB/TA - LA - LB)
            double us;
            if (swap_first(a, it, &us) == m) {
                const double TB = a.Tcoefs[m + 1];
                lus = log(us); k1 = Tm / TB - 1.0; k2 = TB / Tm - 1.0;
            }
        }
        w[4] = lus; w[5] = k1; w[6] = k2; w[7] = (double)slot;
    }
    if (settled) return;
    const double *sv, *sp;
    if (d.src_acc) {
        const size_t gp = (size_t)((it - 1) % 3) * f.NS + d.src_ps;
        sv = f.cand_vars + gp * Nv;
        sp = f.cand_params + gp * Np;
    } else {
        sv = a.vars_cur + ((size_t)d.src_par * C + d.src) * Nv;
        sp = a.params_cur + ((size_t)d.src_par * C + d.src) * Np;
    }
    double *dv = a.vars_cur + ((size_t)q * C + m) * Nv, *dp = a.params_cur + ((size_t)q * C + m) * Np;
    double *rv = (a.samples && rec >= 0) ? a.samples + ((size_t)rec * C + m) * Nv : nullptr;
    for (int i = lane; i < Nv; i += 64) { const double v = sv[i]; dv[i] = v; if (rv) rv[i] = v; }
    for (int i = lane; i < Np; i += 64) dp[i] = sp[i];
    if (lane == 0) {
        a.logL_cur[q * C + m] = d.o.logL;
        a.logPr_cur[q * C + m] = d.o.logPr;
        a.logPost_cur[q * C + m] = d.o.logPost;
        f.slot[q * C + m] = slot;
        a.moved[m] = d.src_acc;
        a.Pmove[m] = d.r;
        if (m == 0 && d.src_acc) a.counters[1] += 1;
        a.counters[8 + m] += d.src_acc;
        if (m == 0) a.counters[0] = it;
        if (d.swap_first == m) {  // (the pair's first chain counts the swap step)
            atomicAdd((unsigned long long *)&a.counters[2], 1ull);  // (the two chain groups' launches run side by side)
            if (d.swapped) atomicAdd((unsigned long long *)&a.counters[3], 1ull);
        }
        if (a.stats && rec >= 0) {
            double *r = a.stats + ((size_t)rec * C + m) * 3;
            r[0] = d.o.logL; r[1] = d.o.logPr; r[2] = d.o.logPost;
        }
        // (diagnostic: the one kind of record that this chain's tiles decided without decide() whatever the margin)
        if (tiles && d.swap_first < 0 && f.quick[((size_t)(q ^ 1) * C + m) * QN + 1] == 2.0) atomicAdd(f.qcount + 1, 1ull);
    }
}

// decide() for the workgroups that only need to know WHERE chain m stands -- the likelihood tiles (its table slot), the candidate roles
// (slot and the vector the chain continues from) -- the cheapest way that is still certain.  The MH test of iteration it-1 is a
// comparison of S = the sum of launch it-1's partials with a threshold S* that the previous launch's commit workgroup has left
// (commit_chain: everything in the test but S is known one launch earlier).  S is summed here in any order; when it is further from S*
// than every rounding involved could explain (summation: n eps sum|v| ~ 2e-14 sum|v|; the threshold and the test's own exp / division:
// a few eps of |S*|; the margin, FusedArgs::qmargin, is 1e-11 of those magnitudes) the outcome is the exact test's.  The swap test of iteration it-1's pair
// (pairA, named by the host: the same Philox draw) is taken the same way: log u against LA (TA/TB - 1) + LB (TB/TA - 1) with the
// post-test likelihoods from the approximate sums.  Otherwise -- about once in 1e5 tests -- decide() evaluates everything as written.
// A decide() of ~2000 dependent instructions costs a lone wave 5 us at the head of the launch's longest chains; this one ~0.5 us.
//
// The sums come from FusedArgs::qacc: every tile of launch it-1 has added ONE value, c_t = fl(p_t[0] + p_t[1]), and |c_t| into its chain's
// accumulators (StepTiles::store_sums: 8 keys x 2 doubles per chain, set (it-1) mod 3), so what is left to do here does not grow with the
// number of tiles: one load of the chain's 16 doubles by 16 lanes, three rotate-and-add rounds within that row of lanes, and the two sums
// and the record's fields are read from their lanes (v_readlane, constant lanes) -- no LDS round trip anywhere.  (Not scalar loads into
// 48 SGPRs, or 96 for a pair: the tile path has no SGPRs to spare -- the kernel then spills ~170 of them to VGPR lanes in every wave.)
// Why the margin still covers it.  The order in which the atomics arrive is not fixed, and need not be: S is the sum of the same n values
// c_t in SOME order -- whichever, each key's in its arrival order and the keys after one another, it is a chain of n-1 rounded additions,
// and "n eps sum|v|" above bounds every such chain.  The pre-addition adds one rounding of relative size eps to each term,
// |c_t - (p_t[0] + p_t[1])| <= eps (|p_t[0]| + |p_t[1]|), which is one more unit in that n; the magnitude is sum|c_t| (summed with the
// same n eps of relative error, which the margin does not feel), and sum|c_t| <= sum|p_t[0]| + sum|p_t[1]|, so the margin can only be the
// smaller of the two -- by the factor to which the two partials of a tile cancel.  They do not
// cancel to speak of: p_t[0] = sum y/M is ~ the tile's bin count with a chi-square scatter of its square root, p_t[1] = sum ln M moves
// with the units of the spectrum; even where ln M ~ -1 on every bin, |c_t| stays ~ sqrt(bins) = 1/50 of the magnitude.  1e-11 sum|c_t|
// against ~2e-14 (sum|p_t[0]| + sum|p_t[1]|) leaves three orders of magnitude, one and a half in that worst case.  A NaN or an infinite
// partial makes its accumulator NaN or infinite: every comparison below fails and the answer is "undecided".  (The exact decide(), the
// commit workgroups and the records keep reading `part`, in k_finalize's order; the commit workgroup also asks this shortcut and counts a
// decided answer that is not decide()'s -- FusedArgs::qcount[2].)

// x of every lane of the same parity in the lane's row of 16 added up (rotations by 8, 4 and 2 lanes within the row: register moves, no LDS
// round trip).  Every lane of a row ends with the same three additions of the same values in another order -- lanes 0 and 1 are read.
__device__ __forceinline__ double row_sum_by_parity(double x) {
#define TAMCMC_ROW_ROR(x, n)                                                                                                     \
    __longlong_as_double(((long long)__builtin_amdgcn_update_dpp(0, (int)(__double_as_longlong(x) >> 32), 0x120 + (n), 0xf, 0xf, false) << 32) | \
                         (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(__double_as_longlong(x) & 0xffffffffll), 0x120 + (n), 0xf, 0xf, false))
    x += TAMCMC_ROW_ROR(x, 8);
    x += TAMCMC_ROW_ROR(x, 4);
    x += TAMCMC_ROW_ROR(x, 2);
#undef TAMCMC_ROW_ROR
    return x;
}

// (the shortcut itself: -1 = undecided.  es: the accumulator set of the iteration to decide.  Inlined at the head of a likelihood tile,
// whose own first loads are in flight beside these -- StepTiles::head; a leaf function for the candidate roles and the commit workgroups)
__device__ __forceinline__ int quick_decide_core(const DevSamplerArgs *ga, const FusedArgs *gf, int m, int q, int es, int pairA, Decided *out) {
    const ConstArgs &a = *(const ConstArgs *)uniform_ptr(ga);
    const ConstFused &f = *(const ConstFused *)uniform_ptr(gf);
    const int lane = threadIdx.x & 63, C = a.C;
    const int p = q ^ 1;
    const bool in_pair = pairA >= 0 && (m == pairA || m == pairA + 1);
    const int j0 = in_pair ? pairA : m;
    const double *r0 = f.quick + ((size_t)p * C + j0) * QN;
    const double *g0 = f.qacc + ((size_t)es * C + j0) * (2 * QK);
    // two loads: the records (lane k < QN: field k of chain j0, lane QN + k: of chain j0 + 1) and the accumulators (lane k < 16: chain j0's,
    // lane 16 + k: chain j0 + 1's, which lie right behind -- one row of 16 lanes per chain, the sums of c in its even lanes, of |c| in its odd)
    const double rec = lane < (in_pair ? 2 * QN : QN) ? r0[lane] : 0.0;
    const double acc = lane < (in_pair ? 4 * QK : 2 * QK) ? g0[lane] : 0.0;
    const double sums = row_sum_by_parity(acc);
    double s0 = lane_value<0>(sums), a0 = lane_value<1>(sums);
    const double St0 = lane_value<0>(rec), ok0 = lane_value<1>(rec);
    const int ps0 = (int)lane_value<7>(rec);
    const double mg = f.qmargin;
    // kind 1: threshold test; kind 2: the proposal cannot be accepted (outside a prior's support, or its table failed: r = 0 and u > 0) --
    // its partial sums may be anything (an empty slot's tiles are skipped)
    int acc0 = 0;
    if (ok0 == 2.0) { s0 = 0; a0 = 0; }
    else if (ok0 > 0 && fabs(s0 - St0) > mg * (a0 + fabs(St0))) acc0 = s0 < St0 ? 1 : 0;  // (a NaN sum fails the comparison)
    else return -1;
    Decided d;
    d.swap_first = -1; d.swapped = 0; d.src_par = p; d.r = 0;
    d.o.acc = 0; d.o.r = 0; d.o.logL = 0; d.o.logPr = 0; d.o.logPost = 0;  // (the scalars are the commit workgroup's business: decide())
    if (!in_pair) { d.slot = 2 * m + acc0; d.src = m; d.src_acc = acc0; d.src_ps = ps0; }
    else {
        double s1 = lane_value<16>(sums), a1 = lane_value<17>(sums);
        const double St1 = lane_value<QN>(rec), ok1 = lane_value<QN + 1>(rec);
        const int ps1 = (int)lane_value<QN + 7>(rec);
        int acc1 = 0;
        if (ok1 == 2.0) { s1 = 0; a1 = 0; }
        else if (ok1 > 0 && fabs(s1 - St1) > mg * (a1 + fabs(St1))) acc1 = s1 < St1 ? 1 : 0;
        else return -1;
        const double c0 = lane_value<2>(rec), c1 = lane_value<QN + 2>(rec);
        const double LA = acc0 ? c0 * s0 : lane_value<3>(rec), LB = acc1 ? c1 * s1 : lane_value<QN + 3>(rec);
        const double lus = lane_value<4>(rec), x = LA * lane_value<5>(rec) + LB * lane_value<6>(rec);
        // (written as !(>): a NaN on either side -- a NaN sum, or inf * 0 under the forced margin -- is undecided)
        if (!(fabs(x - lus) > mg * (fabs(c0) * a0 + fabs(c1) * a1 + fabs(LA) + fabs(LB)))) return -1;
        const int swapped = x > lus ? 1 : 0;
        const int A = pairA, B = pairA + 1;
        d.swap_first = A; d.swapped = swapped;
        if (swapped) {
            if (m == A) { d.slot = 2 * C + (A >= f.xsplit ? 4 : 0) + acc1; d.src = B; d.src_acc = acc1; d.src_ps = ps1; }
            else { d.slot = 2 * C + (B >= f.xsplit ? 4 : 0) + 2 + acc0; d.src = A; d.src_acc = acc0; d.src_ps = ps0; }
        } else {
            if (m == A) { d.slot = 2 * A + acc0; d.src = A; d.src_acc = acc0; d.src_ps = ps0; }
            else { d.slot = 2 * B + acc1; d.src = B; d.src_acc = acc1; d.src_ps = ps1; }
        }
    }
    if (out && lane == 0) *out = d;
    return d.slot;
}
__device__ __attribute__((noinline)) int quick_decide_leaf(const DevSamplerArgs *ga, const FusedArgs *gf, int m, int q, int es, int pairA, Decided *out) {
    return quick_decide_core(ga, gf, m, q, es, pairA, out);
}

__device__ __forceinline__ int quick_decide(const DevSamplerArgs *ga, const FusedArgs *gf, int m, long it, int q, int settled, int pairA,
                                            Decided *out) {
    if (settled) return decide(ga, gf, m, it, q, 1, out);
    const int s = quick_decide_leaf(ga, gf, m, q, (int)((it + 2) % 3), pairA, out);
    return s >= 0 ? s : decide(ga, gf, m, it, q, 0, out);
}

// The fallback of a likelihood tile, which wants the slot alone (StepTiles::head).  It is counted (FusedArgs::qcount[0]) once per chain and
// iteration, by the chain's tile 0, inside the cold branch: the decided path has no instruction for it.
__device__ __attribute__((noinline)) int decide_counted(const DevSamplerArgs *ga, const FusedArgs *gf, int m, long it, int q, int tile) {
    if (tile == 0 && (threadIdx.x & 63) == 0) atomicAdd(((const ConstFused *)uniform_ptr(gf))->qcount, 1ull);
    return decide(ga, gf, m, it, q, 0, nullptr);
}

// Hook of the likelihood tiles of the fused step: evaluation b = chain first + b.
struct StepTiles {
    const DevSamplerArgs *ga;
    const FusedArgs *gf;
    long it;
    int q, first, settled, pairA;
    static constexpr bool early_loads = true;
    // The chain's slot and what it leads to.  A chain outside iteration it-1's swap pair proposes from slot 2m (that iteration rejected)
    // or 2m + 1 (accepted): both slots' words are requested before the decision's own loads and selected after it -- one memory round
    // trip less at the head of every tile.  (Not their 152-byte rows: two of them would have to stay in registers across the decision.)
    __device__ __forceinline__ tile::SlotWords head(const LoglikeArgs &a, int b, int tile) const {
        const int m = first + b;
        if (settled) return tile::slot_words(a, decide(ga, gf, m, it, q, 1, nullptr));
        // (a.per > 0, the candidates' fixed-size table slots: no word is loaded under a condition -- a register that one branch loads and
        // the other computes is waited for, with every load in flight, where it is computed)
        const bool lone = a.per > 0 && !(pairA >= 0 && (m == pairA || m == pairA + 1));
        tile::SlotWords w0{}, w1{};
        if (lone) { w0 = tile::slot_words(a, 2 * m); w1 = tile::slot_words(a, 2 * m + 1); }
        int s = quick_decide_core(ga, gf, m, q, (int)((it + 2) % 3), pairA, nullptr);
        if (s < 0) s = decide_counted(ga, gf, m, it, q, tile);
        if (lone && (s >> 1) == m) return (s & 1) ? w1 : w0;
        return tile::slot_words(a, s);
    }
    // (lane 0, beside the stores of the two sums: what quick_decide reads of this tile, added to the chain's accumulators of this
    // iteration's set.  Two atomics whose result nobody waits for; the key -- the workgroup's id & 7, as loglike_tile counts it: the roles'
    // and the L z blocks' workgroups before the tiles come in eights -- only spreads them over eight pairs of addresses)
    __device__ __forceinline__ void store_sums(int b, int /*tile*/, double s0, double s1) const {
        const ConstArgs &a = *(const ConstArgs *)uniform_ptr(ga);
        const ConstFused &f = *(const ConstFused *)uniform_ptr(gf);
        const double c = s0 + s1;
        double *g = f.qacc + (((size_t)(it % 3) * a.C + first + b) * QK + (blockIdx.x & 7)) * 2;
        atomicAdd(g, c);
        atomicAdd(g + 1, fabs(c));
    }
};

// The three kinds of work on one candidate (see candidate_role); the proposal vector is in LDS.
// (They are real function calls -- see candidate_role -- so their arguments are pointers to the DEVICE-MEMORY copies of the argument
// blocks: a reference to a kernel argument would have to be copied to the scratch stack first.)
__device__ __attribute__((noinline)) void role_prior(const DevSamplerArgs *ga, const FusedArgs *gf, size_t gs, int h, const double *s_vars,
                                                     const double *s_params, const UnpackLds *Up) {
    const DevSamplerArgs &a = *ga;
    const FusedArgs &f = *gf;
    const UnpackLds U = *Up;
    const int Nv = a.Nv, Np = a.desc.Np, tid = threadIdx.x;
    if (h == 0) {
        for (int i = tid; i < Nv; i += 64) f.cand_vars[gs * Nv + i] = s_vars[i];
        for (int i = tid; i < Np; i += 64) f.cand_params[gs * Np + i] = s_params[i];
    }
    int rej = 0;
#ifdef TAMCMC_PROBE
    long ps_[4] = {0, 0, 0, 0};
    const double fh = wave_log_prior_part(a.desc, s_params, U, TB - 128, h, &rej, ps_);
    if (tid == 0 && (int)(gs % f.NS) == 2) { long *w = a.counters + 8 + a.C + 16 * h + 4; w[0] += ps_[1] - ps_[0]; w[1] += ps_[2] - ps_[1]; }
#else
    const double fh = wave_log_prior_part(a.desc, s_params, U, TB - 128, h, &rej);  // the proposal kernel's 128 term lanes (dev_unpack.h)
#endif
    if (tid == 0) {
        f.cand_logPr[2 * gs + h] = fh;
        f.cand_stP[2 * gs + h] = *U.status;
        if (h == 0) f.cand_rej[gs] = rej;
    }
}
__device__ __forceinline__ TablePtrs candidate_tables(const DevSamplerArgs &a, const FusedArgs &f, int q_dst) {
    TablePtrs T;
    T.mults = f.mults + (size_t)q_dst * f.NS * a.desc.per; T.pairs = f.pairs + (size_t)q_dst * 2 * f.NS; T.nh = f.nh + (size_t)q_dst * f.NS;
    T.nn = f.nn + (size_t)q_dst * f.NS; T.noise = f.noise + (size_t)q_dst * f.NS * a.desc.stride;
    T.bg = nullptr; T.ntiles = a.ntiles; T.tile_bins = a.tile_bins;
    return T;
}
__device__ __attribute__((noinline)) void role_rows(const DevSamplerArgs *ga, const FusedArgs *gf, int q_dst, int slot, size_t gs,
                                                    const double *s_params, const UnpackLds *Up) {
    const DevSamplerArgs &a = *ga;
    const FusedArgs &f = *gf;
    const UnpackLds U = *Up;
    if (threadIdx.x == 0) mt::shared_scalars_base(a.desc.model_id, s_params, a.desc.plength, *U.S);
    __syncthreads();
    const TablePtrs T = candidate_tables(a, f, q_dst);
    // the table is built whatever the prior says (this role does not know it): a vector outside a prior's support is rejected by
    // the settle step before its likelihood is looked at (model_def.cpp:476-480), a table that cannot be built leaves an empty slot
#ifdef TAMCMC_PROBE
    __shared__ long ps_[8];
    wg_unpack(a.desc, s_params, U, slot, T, true, false, false, true, ps_);
    __syncthreads();
    if (threadIdx.x == 0 && (int)(gs % f.NS) == 2) {
        long *w = a.counters + 8 + a.C + 8 + 4; w[0] += ps_[1] - ps_[0]; w[1] += ps_[2] - ps_[1];
        long *v = a.counters + 8 + a.C + 32; v[0] += ps_[5] - ps_[4]; v[1] += ps_[6] - ps_[5]; v[2] += ps_[7] - ps_[6]; v[3] += 1;
    }
#else
    wg_unpack(a.desc, s_params, U, slot, T, true, false, false, true);
#endif
    if (threadIdx.x == 0) f.cand_stR[gs] = *U.status;
}
__device__ __attribute__((noinline)) void role_background(const DevSamplerArgs *ga, const FusedArgs *gf, int q_dst, int slot, int role,
                                                          const double *s_params, const UnpackLds *Up) {
    const DevSamplerArgs &a = *ga;
    const FusedArgs &f = *gf;
    const UnpackLds U = *Up;
    if (!f.bg) return;
    if (threadIdx.x == 0) mt::shared_scalars_base(a.desc.model_id, s_params, a.desc.plength, *U.S);
    __syncthreads();
    TablePtrs T = candidate_tables(a, f, q_dst);
    T.bg = f.bg + (size_t)q_dst * f.NS * a.ntiles * bg::NH;
    const int quarter = (a.ntiles + 3) / 4, k = role - 3;
    wg_bg_tiles(a.desc, s_params, U.S, slot, T, 0, 64, k * quarter, (k + 1) * quarter);
}

// L z of chain `m` for iteration `itn` into f.lz[parity q_dst] (same streams, same row sums as propose_common), one wave.
// (two separate functions, like the candidate roles: each stays within the register budget of the tile path)
__device__ __attribute__((noinline)) void lz_normals(const DevSamplerArgs *ga, long itn, int m, double *s_z) {
    normals_into(*ga, m, itn, s_z);
}
__device__ __attribute__((noinline)) void lz_rows(const DevSamplerArgs *ga, const FusedArgs *gf, int q_dst, int m, const double *s_z) {
    Lz_rows_wave(*ga, m, s_z, gf->lz + ((size_t)q_dst * ga->C + m) * ga->Nv);
}
__device__ __forceinline__ void lz_block(const DevSamplerArgs *ga, const FusedArgs *gf, long itn, int q_dst, int m, unsigned char *lds) {
    double *s_z = (double *)lds;
    lz_normals(ga, itn, m, s_z);
    __syncthreads();
    lz_rows(ga, gf, q_dst, m, s_z);
}

// One role of one candidate slot of iteration `itn`, by ONE wave.  Slot s < 2C: chain s/2, built on the position it enters iteration
// itn-1 with (even) or on its proposal of iteration itn-1 (odd); slots 2C..2C+3 (only when itn-1 swaps a pair A,B): chain A on B's two
// vectors, chain B on A's two.  Roles: 0 = position + first half of the log-prior (and the hard constraints), 1 = table rows + noise row,
// 2 = second half of the log-prior, 3..6 = background series of a quarter of the tiles each, 7 = none.  Every role re-derives the proposal vector itself (no communication between the roles), and -- inside a
// stretch -- first decides iteration itn-2 for the chain it builds on (decide(): where that chain stands at itn-1, which slot it proposes).
// entry: the candidates of iteration itn itself from the settled chains (state parity q_src), even slots only.
__device__ void candidate_role(const DevSamplerArgs &a, const FusedArgs &f, const DevSamplerArgs *ga, const FusedArgs *gf, long itn, int q_src,
                               int q_dst, int slot, int role, bool entry, int settled, int pairA, unsigned char *lds, Decided *dec) {
    if (role > 6) return;
    const int C = a.C, Nv = a.Nv, Np = a.desc.Np, tid = threadIdx.x;
    const int e_dst = (int)(itn % 3);
    int m, src, on_prop;
    if (slot < 2 * C) { m = slot >> 1; src = m; on_prop = slot & 1; }
    else {  // slot = 2C + e, e = 0..3: the pair's cross candidates, stored in the pair's extra block
        if (entry || !is_swap_iter(a, itn - 1)) return;
        const int A = swap_first(a, itn - 1, nullptr), e = slot - 2 * C;
        m = (e < 2) ? A : A + 1;
        src = (e < 2) ? A + 1 : A;
        on_prop = e & 1;
        slot += (m >= f.xsplit) ? 4 : 0;  // in the extra block of the chain that will use it (the group that owns that block never runs
                                          // ahead of itself; the OTHER group's launches may be several iterations ahead)
    }
    if (entry && on_prop) return;  // a stretch starts from settled chains: there is no pending proposal to build on
    if (entry && role == 0 && tid == 0) f.slot[q_src * C + m] = 2 * m;
#ifdef TAMCMC_PROBE
    long pt[6];
    pt[0] = (long)wall_clock64();
#define RSTAMP(k) pt[k] = (long)wall_clock64()
#else
#define RSTAMP(k)
#endif
    double *s_params = (double *)lds;
    double *s_vars = s_params + Np;
    double *s_z = s_vars + Nv;
    const UnpackLds U = carve_unpack_lds((unsigned char *)(s_z + Nv + 1));
    __shared__ UnpackLds s_U;  // handed to the role functions by address
    if (tid == 0) s_U = U;
    const double *bv, *bp;
    if (entry) {
        bv = a.vars_cur + ((size_t)q_src * C + src) * Nv;
        bp = a.params_cur + ((size_t)q_src * C + src) * Np;
    } else {
        const int ps = quick_decide(ga, gf, src, itn - 1, q_src, settled, pairA, dec);
        __syncthreads();
        const Decided d = *dec;
        if (on_prop) {  // src's proposal of iteration itn-1
            const size_t gp = (size_t)((itn - 1) % 3) * f.NS + ps;
            bv = f.cand_vars + gp * Nv;
            bp = f.cand_params + gp * Np;
        } else if (d.src_acc) {  // src enters iteration itn-1 at a proposal of iteration itn-2 that was accepted
            const size_t gp = (size_t)((itn - 2) % 3) * f.NS + d.src_ps;
            bv = f.cand_vars + gp * Nv;
            bp = f.cand_params + gp * Np;
        } else {
            bv = a.vars_cur + ((size_t)d.src_par * C + d.src) * Nv;
            bp = a.params_cur + ((size_t)d.src_par * C + d.src) * Np;
        }
    }
    RSTAMP(1);
    // everything the proposal vector is made of in ONE memory round trip: the base vectors, L z(itn) of chain m (q_dst: iteration itn's
    // parity; computed one launch ahead, lz_block), the scatter indices, the polynomial table
    const double *lz = f.lz + ((size_t)q_dst * C + m) * Nv;
    constexpr int PW = (int)(sizeof(mt::PolyTab) / sizeof(double));
    if (Nv <= 128 && Np <= 128 && PW <= 256) {
        double r_v[2], r_z[2], r_p[2], r_t[4];
        int r_i[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int i = tid + 64 * e;
            r_v[e] = i < Nv ? bv[i] : 0.0; r_z[e] = i < Nv ? lz[i] : 0.0; r_i[e] = i < Nv ? a.index_to_relax[i] : 0;
            r_p[e] = i < Np ? bp[i] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < 4; e++) { const int i = tid + 64 * e; r_t[e] = i < PW ? ((const double *)a.desc.poly)[i] : 0.0; }
#pragma unroll
        for (int e = 0; e < 2; e++) { const int i = tid + 64 * e; if (i < Np) s_params[i] = r_p[e]; }
#pragma unroll
        for (int e = 0; e < 4; e++) { const int i = tid + 64 * e; if (i < PW) ((double *)U.poly)[i] = r_t[e]; }
        if (tid == 0) { *U.status = TAMCMC_OK; *U.reject = 0; }  // (unpack_begin)
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int i = tid + 64 * e;
            if (i < Nv) { const double v = r_v[e] + 0.0 + r_z[e]; s_vars[i] = v; s_params[r_i[e]] = v; }  // same expression as propose_common; update_params_with_vars
        }
        __syncthreads();
    } else {
        for (int i = tid; i < Nv; i += 64) s_vars[i] = bv[i];
        for (int i = tid; i < Np; i += 64) s_params[i] = bp[i];
        unpack_begin(a.desc, U);  // (barrier)
        for (int i = tid; i < Nv; i += 64) s_vars[i] = s_vars[i] + 0.0 + lz[i];
        __syncthreads();
        for (int k = tid; k < Nv; k += 64) s_params[a.index_to_relax[k]] = s_vars[k];
        __syncthreads();
    }
    RSTAMP(2);
    const size_t gs = (size_t)e_dst * f.NS + slot;
    // (three separate functions: inlined side by side the roles' code raises the whole kernel's register allocation above the
    // three-waves-per-SIMD budget of the tile path)
#ifdef TAMCMC_PROBE
    if (a.probe & (0x100 << (role > 2 ? 2 : (role == 2 ? 0 : role)))) return;  // timing experiments: one kind of role left out
#endif
    if (role == 0 || role == 2) role_prior(ga, gf, gs, role >> 1, s_vars, s_params, &s_U);
    else if (role == 1) role_rows(ga, gf, e_dst, slot, gs, s_params, &s_U);
    else role_background(ga, gf, e_dst, slot, role, s_params, &s_U);
#ifdef TAMCMC_PROBE
    __syncthreads();
    RSTAMP(3);
    if (tid == 0 && slot == 2 && !entry && role < 4) {  // one slot's first four roles: decide | vectors, L z | the role itself (units of 10 ns)
        long *w = a.counters + 8 + C + 8 * role;
        w[0] += pt[1] - pt[0]; w[1] += pt[2] - pt[1]; w[2] += pt[3] - pt[2]; w[3] += 1;
    }
#endif
#undef RSTAMP
}

// Per-launch scalars of the fused step.
struct StepCtl {
    long it, rec, it_lz;   // iteration of the tiles; record index of iteration it-1 (-1: none); first iteration of the L z blocks
    int q, flags;          // parity of iteration `it`; ST_* bits
    int nbr, nlz;          // workgroups reserved for candidate roles / L z blocks + commits (multiples of 8: keeps the tiles' XCD mapping)
    int n_lz_live, q_lz;   // L z blocks that have work (chain first + e % cnt of iteration it_lz + e / cnt); parity of it_lz
    int first, cnt;        // the chains of this launch: [first, first + cnt) -- all of them, or one chain group (see run(): fused)
    int extra;             // 1: the launch also builds the four extra candidates of its iteration's swap pair (slots 2C..2C+3)
    int pairA;             // first chain of iteration it-1's swap pair, -1: none (quick_decide)
    const DevSamplerArgs *ga;  // device-memory copies of the first two kernel arguments (for the function calls)
    const struct FusedArgs *gf;
};

// Launch `it` of a fused stretch: [0, nbr) candidate roles of iteration it+1 (ST_BR; at the entry of a stretch, ST_ENTRY: of iteration
// `it` itself from the settled chains), [nbr, nbr+nlz): L z of later iterations (ST_LZ) and, in the last cnt of them, the chains' commit
// workgroups (ST_COMMIT), then the likelihood tiles of iteration `it` (ST_L).  ST_FIRST: the chains are settled (nothing to decide).
#define TAMCMC_STEP_BODY                                                                                                      \
    __shared__ tile::TileLds<MODE, 64> lds;                                                                                  \
    __shared__ Decided s_dec;                                                                                                \
    const int id = (int)blockIdx.x;                                                                                          \
    const int settled = (c.flags & ST_FIRST) ? 1 : 0;                                                                        \
    /* the few single-wave workgroups with long dependent chains (roles, L z, commit) issue ahead of the tiles they share a SIMD with */ \
    if (id < c.nbr + c.nlz) __builtin_amdgcn_s_setprio(3);                                                                   \
    if (id < c.nbr) {                                                                                                        \
        const int k = id >> 3, slot = k < 2 * c.cnt ? 2 * c.first + k : 2 * a.C + (k - 2 * c.cnt); /* the group's slots, then the pair's */ \
        if (k >= 2 * c.cnt && !c.extra) return;                                                                              \
        if (c.flags & ST_ENTRY) candidate_role(a, f, c.ga, c.gf, c.it, c.q, c.q, slot, id & 7, true, 1, -1, (unsigned char *)&lds, &s_dec);    \
        else if (c.flags & ST_BR)                                                                                            \
            candidate_role(a, f, c.ga, c.gf, c.it + 1, c.q, c.q ^ 1, slot, id & 7, false, settled, c.pairA, (unsigned char *)&lds, &s_dec); \
        return;                                                                                                              \
    }                                                                                                                        \
    if (id < c.nbr + c.nlz) {                                                                                                \
        const int e = id - c.nbr, k = e - (c.nlz - c.cnt);                                                                   \
        if (k >= 0 && (c.flags & ST_COMMIT)) commit_chain(c.ga, c.gf, c.first + k, c.it, c.q, settled, c.rec, c.flags & ST_L, &s_dec); \
        else if (e < c.n_lz_live)                                                                                            \
            lz_block(c.ga, c.gf, c.it_lz + e / c.cnt, (c.q_lz ^ (e / c.cnt)) & 1, c.first + e % c.cnt, (unsigned char *)&lds);  \
        return;                                                                                                              \
    }                                                                                                                        \
    if (c.flags & ST_L)                                                                                                      \
        tile::loglike_tile<MODE, 64, K, false, false>(la, id - c.nbr - c.nlz, lds, StepTiles{c.ga, c.gf, c.it, c.q, c.first, settled, c.pairA});
// The tile path of K <= 8 bins per lane fits 168 VGPRs = three waves per SIMD; the candidate roles (log-prior, series) would raise the
// kernel's allocation above that, so the occupancy is pinned here (those roles are separate functions, see candidate_role).
template <int MODE, int K>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) k_step(const DevSamplerArgs a, const FusedArgs f, const LoglikeArgs la,
                                                                                      const StepCtl c) {
    TAMCMC_STEP_BODY
}
template <int MODE, int K>
__global__ void __launch_bounds__(64) k_step_wide(const DevSamplerArgs a, const FusedArgs f, const LoglikeArgs la, const StepCtl c) {
    TAMCMC_STEP_BODY
}
#undef TAMCMC_STEP_BODY

// ev0 / ev1 (optional): events stamped at the kernel's own start and end (hipExtLaunchKernelGGL) -- the duration rocprofv3 reports for a
// dispatch, without the time the launch waits in its stream
template <int MODE>
bool launch_step_k(int K, int grid, hipStream_t st, const DevSamplerArgs &a, const FusedArgs &f, const LoglikeArgs &la, const StepCtl &c,
                   hipEvent_t ev0, hipEvent_t ev1) {
    if (K == 4) hipExtLaunchKernelGGL((k_step<MODE, 4>), dim3(grid), dim3(64), 0, st, ev0, ev1, 0, a, f, la, c);
    else if (K == 8) hipExtLaunchKernelGGL((k_step<MODE, 8>), dim3(grid), dim3(64), 0, st, ev0, ev1, 0, a, f, la, c);
    else if (K == 16) hipExtLaunchKernelGGL((k_step_wide<MODE, 16>), dim3(grid), dim3(64), 0, st, ev0, ev1, 0, a, f, la, c);
    else return false;
    return true;
}
hipError_t launch_step(int mode, int K, int grid, hipStream_t st, const DevSamplerArgs &a, const FusedArgs &f, const LoglikeArgs &la,
                       const StepCtl &c, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) {
    if (grid <= 0) return hipSuccess;
    bool ok;
    if (mode == TAMCMC_PRECISION_FAST) ok = launch_step_k<tile::M_FAST>(K, grid, st, a, f, la, c, ev0, ev1);
    else if (mode == TAMCMC_PRECISION_FAST_DIRECT) ok = launch_step_k<tile::M_FAST_DIRECT>(K, grid, st, a, f, la, c, ev0, ev1);
    else ok = launch_step_k<tile::M_STRICT>(K, grid, st, a, f, la, c, ev0, ev1);
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}
