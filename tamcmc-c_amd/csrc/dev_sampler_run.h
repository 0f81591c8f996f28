// dev_sampler_run.h -- the host drivers of the device-resident engine (included by dev_sampler.hip after dev_sampler_state.h): what
// they share (KernelTiming, SettleLoop, Impl::reserve_records, copy_records) and RunCall, one run() call.  Random walk: prepare, the
// schedule of step_schedule.h over run_lockstep / run_fused / run_env_step, finish.  Langevin step (dev_mala_impl.h): run_mala.

static std::atomic<int> g_running_calls{0};
struct RunningCall {
    RunningCall() { g_running_calls.fetch_add(1, std::memory_order_relaxed); }
    ~RunningCall() { g_running_calls.fetch_sub(1, std::memory_order_relaxed); }
};

// TAMCMC_CALL_TIMELINE=1: host-side stamps of every run() call on stderr (entry -> first launch -> all launches enqueued -> streams idle)
static const bool g_call_timeline = getenv("TAMCMC_CALL_TIMELINE") != nullptr;
struct CallTimeline {
    std::chrono::steady_clock::time_point t[5];
    int n = 0;
    void mark() { if (g_call_timeline && n < 5) t[n++] = std::chrono::steady_clock::now(); }
    ~CallTimeline() {
        if (!g_call_timeline || n < 2) return;
        fprintf(stderr, "run() timeline (us):");
        for (int k = 1; k < n; k++) fprintf(stderr, " %.1f", std::chrono::duration<double, std::micro>(t[k] - t[k - 1]).count());
        fprintf(stderr, "\n");
    }
};

// The likelihood kernel's time of one run() call (tamcmc_hip_get_timing; only with the context's timing option): which launches are
// bracketed by events, and what the brackets add up to.  The launch code asks for an event pair and gets one or none.  Nothing else
// adds to the context's counters.
struct DevSampler::Impl::KernelTiming {
    Impl &I;
    tamcmc_hip_ctx *c;
    int used_ev = 0;                             // lockstep: pairs I.ev[0..] handed out since the last drain_events
    std::vector<std::pair<int, long>> fused_ev;  // one-launch fused stretches of this call: (pair of I.ev, launches it brackets)
    // fused step with two chain groups: the launches of an iteration overlap, so the stretch's elapsed time is not a launch duration;
    // sampled launches of the second group are bracketed on their own stream instead
    int g_used = 0;                    // pairs of I.fu.gev handed out in this call
    long g_launches = 0, g_iters = 0;  // launches / iterations of the two-group stretches of this call
    double kernel_ms = 0;
    long n_launch = 0, n_eval = 0;
    bool stretch_timed = false;  // the current fused stretch: timed at all, its pair of I.ev, the next iteration to sample
    int fe = 0;
    long next_sample = 0;
    int b_timed = 0;  // Langevin step: sampled batches of this call (their times in kernel_ms) and the bins their delta launches touched
    long b_bins = 0;

    // lockstep stretch: the pair around launch k when every `every`-th one is sampled (the top 16 pairs: fused stretches)
    hipEvent_t *lockstep_pair(long k, long every) { return c->timing && k % every == 0 && used_ev < Impl::N_EV - 16 ? I.ev[used_ev++] : nullptr; }
    // ... and their average x launches_represented into the totals.  Call after a stream sync
    int drain_events(double launches_represented, long evals) {
        if (used_ev) {
            double tot = 0;
            for (int e = 0; e < used_ev; e++) {
                float ms = 0;
                DCHK(hipEventElapsedTime(&ms, I.ev[e][0], I.ev[e][1]));
                tot += ms;
            }
            kernel_ms += tot / used_ev * launches_represented;
            n_launch += (long)launches_represented;
            n_eval += evals;
        }
        used_ev = 0;
        return TAMCMC_OK;
    }
    // fused stretch of `len` iterations.  One launch per iteration: two events around the whole stretch, i.e. the average includes the
    // time between two launches.  Two groups: every 97th iteration, or the middle one of a short stretch -- the first two-group
    // iteration with the nominal groups at or after it: a joint iteration there must not leave a short call without a measured launch,
    // and a window's launches (eleven and nine chains at the headline shape) are not what the average is multiplied out for
    void begin_fused(long len) {
        stretch_timed = c->timing && fused_ev.size() < 16;
        fe = Impl::N_EV - 1 - (int)fused_ev.size();
        next_sample = len >= 97 ? 48 : len / 2;
    }
    hipEvent_t *stretch_pair() { return stretch_timed ? I.ev[fe] : nullptr; }
    hipEvent_t *sampled_pair(long k) {  // k: iteration of the stretch
        if (!(stretch_timed && g_used < Impl::N_GEV && k >= next_sample)) return nullptr;
        next_sample += 97;
        return I.fu.gev[g_used++];
    }
    void end_fused(long len, bool split, long n_split) {
        if (!stretch_timed) return;
        if (!split) fused_ev.push_back({fe, len});
        else { g_launches += 2 * n_split + (len - n_split); g_iters += len; }
    }
    // end of the call, streams idle: the fused stretches' events, then everything into the context's totals
    int total() {
        for (const auto &e : fused_ev) {
            float ms = 0;
            DCHK(hipEventElapsedTime(&ms, I.ev[e.first][0], I.ev[e.first][1]));
            kernel_ms += ms;
            n_launch += e.second;
            n_eval += e.second * (long)I.a.C;
        }
        if (g_launches > 0) {  // two-group stretches: (average duration of the sampled launches) x (launches); one launch = one group's chains
            double tot = 0;
            for (int e = 0; e < g_used; e++) {
                float ms = 0;
                DCHK(hipEventElapsedTime(&ms, I.fu.gev[e][0], I.fu.gev[e][1]));
                tot += ms;
            }
            if (g_used > 0) {
                kernel_ms += tot / g_used * (double)g_launches;
                n_launch += g_launches;
                n_eval += g_iters * (long)I.a.C;
            }
        }
        c->kernel_ms += kernel_ms;
        c->launches += n_launch;
        c->evals += n_eval;
        return TAMCMC_OK;
    }
    // Langevin step: two sampled batches per call (an event read needs a synchronisation), iterations 0 and n_iter / 2 ...
    hipEvent_t *batch_pair(long i, long n_iter) { return c->timing && (i == 0 || i == n_iter / 2) ? I.ev[0] : nullptr; }
    // ... read after the synchronisation that follows the sampled batch; then the bins its delta launch touched (FdBatch::delta_stats)
    int batch_sampled() {
        float ms = 0;
        DCHK(hipEventElapsedTime(&ms, I.ev[0][0], I.ev[0][1]));
        kernel_ms += ms;
        b_timed++;
        return TAMCMC_OK;
    }
    void batch_bins(long bins) { b_bins += bins; }
    // end of a Langevin call of n_iter batches of B evaluations (the sampled batches stand for all of them); lin / fall: the call's
    // linearised / fallback slots (FdBatch::hybrid_stats)
    void total_batches(long n_iter, long B, bool windowed, long lin, long fall) {
        c->rgb_adj_lin += lin;
        c->rgb_adj_fallback += fall;
        if (!b_timed) return;
        c->kernel_ms += kernel_ms / b_timed * n_iter;
        c->launches += n_iter;
        c->evals += n_iter * B;
        c->fd_bins += b_bins / b_timed * n_iter;
        c->fd_delta_evals += windowed ? n_iter * B : 0;
    }
};

// A settle-then-propose loop over [ia, ib]: launch i settles iteration i-1 (the first has nothing pending) and, for i < ib, proposes
// iteration i.  Each launch reads the state of parity P and writes parity P ^ 1; rec: the record row it writes, or -1
struct SettleLoop {
    int &P;
    const bool record;
    int pending = 0;
    long rec(long i) const { return (pending && record) ? i - 1 : (long)-1; }
    void launched() { P ^= 1; pending = 1; }
};

// Record buffers of a call of n_iter iterations: at least 256 iterations' worth and grown geometrically, so that a caller that records
// in buffers of a fixed length (the reference's Nbuffer) or a short call after a shorter one never pays an allocation -- nor, with it,
// new kernel arguments -- in its steady state (older, smaller buffers are released with the sampler)
int DevSampler::Impl::reserve_records(bool smp, bool st, size_t n_iter) {
    tamcmc_hip_ctx *c = ctx;
    auto reserve = [&](double **buf, size_t &cap, size_t unit) {
        if (cap >= n_iter * unit) return hipSuccess;
        const size_t want = std::max(std::max(n_iter * unit, 256 * unit), cap * 2);
        const hipError_t e = mem.dalloc(buf, want);
        if (e == hipSuccess) cap = want;
        return e;
    };
    if (smp) DCHK(reserve(&a.samples, smp_cap, (size_t)a.C * a.Nv));
    if (st) DCHK(reserve(&a.stats, stat_cap, (size_t)a.C * 3));
    return TAMCMC_OK;
}

// Copy of a call's records to the caller's (pageable) buffers, on the context stream
static hipError_t copy_records(double *samples, double *stats, const DevSamplerArgs &a, size_t n_iter, hipStream_t st) {
    const size_t C = (size_t)a.C, Nv = (size_t)a.Nv;
    hipError_t e = hipSuccess;
    if (samples) e = hipMemcpyAsync(samples, a.samples, n_iter * C * Nv * 8, hipMemcpyDeviceToHost, st);
    if (stats && e == hipSuccess) e = hipMemcpyAsync(stats, a.stats, n_iter * C * 3 * 8, hipMemcpyDeviceToHost, st);
    return e;
}

// One run() call: what every launch of the call needs, filled once by prepare() (Langevin step: prepare_langevin()).
struct DevSampler::Impl::RunCall {
    Impl &I;
    Groups &grp;
    FusedStep &fu;
    tamcmc_hip_ctx *c;
    DevSamplerArgs &a;
    const long it0, n_iter;
    const char *learn;
    double *samples, *stats;
    hipStream_t st;              // the context stream
    CallTimeline &tl;
    KernelTiming T;
    DevSamplerArgs args;         // a, with the record pointers of this call
    LoglikeArgs la[4], lf[3];    // likelihood arguments: (B) per chain group, (A) per candidate set (iteration mod 3)
    int goff[5];                 // chain groups [goff[g], goff[g+1]) of the lockstep scheme
    double *zc_smp = nullptr, *zc_st = nullptr;  // the caller's record buffers as the device sees them (Impl::device_view), else null
    bool use_fused = false;
    bool env_step = false;       // (C): quiet stretches run as k_env_step launches
    int env_nchunk = 0;
    bool split_ok = false;       // fused stretches run as two chain groups [0, f.xsplit), [f.xsplit, C)
    int P;                       // parity of the state buffers that hold the chains' current state
    // (A) the stretch being enqueued
    StepCtl sc{};
    int q = 0;                   // parity of the iteration being enqueued
    // (A) with two groups: the first group's and the joint launches go to st, the second group's to s1 = grp.gst[1]; who waits for whom
    // is the plan's business (step_schedule.h: StepPlanner, with its s1_must_wait and s1_ahead)
    bool s1_open = false;        // s1 still holds launches at the end of the call: the host waits for both streams (finish)
    // Langevin step
    Langevin &V;
    FdBatch::Buffers ws;         // the batch's scratch buffers (the sampler's own)
    MalaArgs M{};
    unsigned char *db = nullptr; // the batch's device block
    size_t lds_settle = 0, lds_test = 0;

    RunCall(Impl &I_, CallTimeline &tl_, long it0_, long n_iter_, const char *learn_, double *samples_, double *stats_)
        : I(I_), grp(I_.grp), fu(I_.fu), c(I_.ctx), a(I_.a), it0(it0_), n_iter(n_iter_), learn(learn_), samples(samples_), stats(stats_),
          st(I_.ctx->stream), tl(tl_), T{I_, I_.ctx}, P(I_.parity), V(I_.lan), ws(I_.lan.ws()) {}

    // tile geometry, scratch and record buffers, the argument blocks
    int prepare() {
        const size_t C = (size_t)a.C, Nv = (size_t)a.Nv;
        // (C): envelope.hip's 1024-bin tiles whatever the context's geometry options say; the xi partials (id 0) and the tile partials
        // are indexed by chain, so chain groups on different streams never share a slot
        a.tile_bins = I.env.on ? ETILE : tile_bins(c->wgs, c->K);
        a.ntiles = (a.desc.Nx + a.tile_bins - 1) / a.tile_bins;
        DCHK(c->d_part.reserve(C * (size_t)a.ntiles * 2));
        a.partials = c->d_part.p;
        a.bg = nullptr;
        use_fused = fu.ok && c->step_scheme != 1 && c->wgs == 64 && (c->K == 4 || c->K == 8 || c->K == 16);
        if (I.env.on) {
            env_nchunk = (a.desc.Nx + ECHUNK - 1) / ECHUNK;
            DCHK(c->d_env.reserve(C * (size_t)env_nchunk * 3));
            env_step = c->step_scheme != 1 && a.desc.Nx <= env_step_max_bins(I.model_id);
            if (env_step) DCHK(I.env.part.reserve(2 * C * (size_t)a.ntiles * 2));
        }
        fu.f.qmargin = c->quick_decide == 1 ? (double)INFINITY : 1e-11;  // (TAMCMC_OPT_QUICK_DECIDE: a test facility)
        const size_t NS = (size_t)fu.f.NS;
        fu.f.bg = nullptr;
        if (c->precision == TAMCMC_PRECISION_FAST && !I.env.on) {
            // background series per (slot, tile).  (B): C slots in the context's scratch (rewritten every iteration).  (A): 2 x NS slots of
            // the sampler's OWN -- the candidates prepared by the last launch of a call are carried over to the next call, and anything else
            // that runs on the context in between (another sampler, a batched evaluation) rewrites the context's scratch
            DCHK(c->d_bg.reserve(C * (size_t)a.ntiles * 8));
            a.bg = c->d_bg.p;
            if (use_fused) {
                DCHK(fu.bg.reserve(3 * NS * (size_t)a.ntiles * 8));
                fu.f.bg = fu.bg.p;
            }
        }
        if (use_fused) {  // (A): the tiles' partial sums by iteration parity (launch i writes one half and reads the other)
            DCHK(fu.part.reserve(2 * C * (size_t)a.ntiles * 2));
            fu.f.part = fu.part.p;
        }
        // (two groups pay once one launch no longer fits the GPU's resident waves -- 20 chains x 196 tiles: 27.7 -> 23.9 us, x 782 tiles:
        // 59.8 -> 49.6 us -- and cost below that: 8 chains x 196 tiles 20.5 -> 23.7 us, 20 chains x 20 tiles 33.5 -> 35.6 us;
        // tools/groups_probe.py)
        split_ok = fu.f.xsplit < a.C && c->step_scheme != 2 && (c->step_scheme == 3 || (long)a.C * a.ntiles >= 2500);
        zc_smp = Impl::device_view(samples, (size_t)n_iter * C * Nv * 8);
        zc_st = Impl::device_view(stats, (size_t)n_iter * C * 3 * 8);
        if (int rc = I.reserve_records(samples && !zc_smp, stats && !zc_st, (size_t)n_iter)) return rc;
        args = a;
        args.samples = samples ? (zc_smp ? zc_smp : a.samples) : nullptr;
        args.stats = stats ? (zc_st ? zc_st : a.stats) : nullptr;
        fill_loglike_args();
        return TAMCMC_OK;
    }

    void fill_loglike_args() {
        const int G = grp.G;
        const size_t NS = (size_t)fu.f.NS;
        for (int g = 0; g <= G; g++) goff[g] = (int)(((long)a.C * g) / G);
        auto fill_common = [&](LoglikeArgs &l, int B) {
            l.x = c->dx.p; l.y = c->dy.p; l.logx = c->dlogx.p; l.Nx = a.desc.Nx; l.B = B; l.ntiles = a.ntiles;
            l.x0 = a.desc.x_first; l.step = a.desc.step; l.noise_stride = a.desc.stride; l.model = nullptr; l.tile_rot = I.tile_rot;
        };
        for (int g = 0; g < G; g++) {
            LoglikeArgs &l = la[g];
            const int first = goff[g];
            fill_common(l, goff[g + 1] - goff[g]);
            l.mults = a.mults; l.offsets = a.pairs + 2 * first; l.noise = a.noise + (size_t)first * a.desc.stride;
            l.per = a.desc.per; l.slot0 = first;  // (chain m's table is rows [m per, (m+1) per) of a.mults: dev_unpack.h, rgb_prestep.hip)
            l.nharvey = a.nh + first; l.nnoise = a.nn + first; l.partials = a.partials + (size_t)first * a.ntiles * 2;
            l.bg_poly = a.bg ? a.bg + (size_t)first * a.ntiles * 8 : nullptr;
        }
        for (int e = 0; e < 3; e++) {  // (A): evaluation m = chain m, its table in a slot of candidate set e = iteration mod 3 (decide())
            LoglikeArgs &l = lf[e];
            const FusedArgs &f = fu.f;
            fill_common(l, a.C);
            l.mults = f.mults + (size_t)e * NS * a.desc.per; l.offsets = f.pairs + (size_t)e * 2 * NS; l.noise = f.noise + (size_t)e * NS * a.desc.stride;
            l.nharvey = f.nh + (size_t)e * NS; l.nnoise = f.nn + (size_t)e * NS; l.partials = f.part;
            l.bg_poly = f.bg ? f.bg + (size_t)e * NS * a.ntiles * 8 : nullptr;
            l.per = a.desc.per; l.slot0 = 0;
        }
    }

    int swap_pair_of(long it) const { return swap_pair(a.seed, a.C, a.dN_mixing, it, nullptr); }

    // stream `to` waits for what `from` holds so far
    int hop(hipEvent_t ev, hipStream_t from, hipStream_t to) {
        DCHK(hipEventRecord(ev, from));
        DCHK(hipStreamWaitEvent(to, ev, 0));
        return TAMCMC_OK;
    }

    // groups gA and gB wait for what the other has enqueued so far (one event each way, ev: one event per group)
    int exchange(hipEvent_t *ev, int gA, int gB) {
        DCHK(hipEventRecord(ev[gA], grp.gst[gA]));
        DCHK(hipEventRecord(ev[gB], grp.gst[gB]));
        DCHK(hipStreamWaitEvent(grp.gst[gA], ev[gB], 0));
        DCHK(hipStreamWaitEvent(grp.gst[gB], ev[gA], 0));
        return TAMCMC_OK;
    }

    // (B) red giants, the proposals' tables of every group: solver, then sort / zeta / rows (and the FAST background series)
    int rgb_tables() {
        RgbDeviceTables R;
        R.mults = a.mults; R.pairs = a.pairs; R.nh = a.nh; R.nn = a.nn; R.noise = a.noise; R.stride = a.desc.stride;
        R.status = a.status_prop + (size_t)P * a.C;
        R.bg = a.bg; R.ntiles = a.ntiles; R.tile_bins = a.tile_bins;
        for (int g = 0; g < grp.G; g++)
            if (int rc = rgb_device_stage(c, goff[g], goff[g + 1] - goff[g], I.rgb_bmax, g, a.desc.per, R, grp.gst[g])) return rc;
        return TAMCMC_OK;
    }

    // (B) the evaluation of group g's proposals, between the events of `pair` if there is one
    int evaluate(int g, hipEvent_t *pair) {
        if (pair) DCHK(hipEventRecord(pair[0], grp.gst[g]));
        if (I.env.on) {  // the rows k_iterate has just written -> the partials the next k_iterate's accept_result sums
            const size_t first = (size_t)goff[g];
            if (int rc = envelope_stage_enqueue(c, I.model_id, goff[g + 1] - goff[g], a.env_rows + first, c->d_env.p + first * env_nchunk * 3,
                                                a.partials + first * a.ntiles * 2, grp.gst[g]))
                return rc;
        } else {
            DCHK(launch_loglike(la[g], c->precision, c->wgs, c->K, false, grp.gst[g]));
        }
        if (pair) DCHK(hipEventRecord(pair[1], grp.gst[g]));
        return TAMCMC_OK;
    }

    // ---- (B) one iteration per round over [ia, ib): k_iterate settles iteration it-1 and proposes iteration it
    int run_lockstep(long ia, long ib) {
        const int G = grp.G;
        fu.disarm();
        I.n.it_lockstep += ib - ia;
        // the extra streams start after everything already enqueued on the context stream
        if (G > 1) {
            DCHK(hipEventRecord(grp.fork, st));
            for (int g = 1; g < G; g++) DCHK(hipStreamWaitEvent(grp.gst[g], grp.fork, 0));
        }
        const long len = ib - ia;
        const long ev_every = len > 32 ? len / 32 : 1;
        SettleLoop L{P, samples || stats};
        int have_pre = 0;
        for (long i = ia; i <= ib; i++) {
            const long it = it0 + i;
            // (0: no adaptation; else what the factor does in this adapting iteration, by the sampler's count of them: step_schedule.h)
            const int learn_p = (L.pending && learn && learn[i - 1]) ? factor_step_mode(I.factor_refresh, I.n_adapt++) : 0;
            // L z of iteration it+1 can be computed by spare workgroups of THIS launch when no adaptation rewrites L in this
            // launch (learn_p) nor in the next one before its proposal (learn[i])
            const int make_pre = (i + 1 < ib && !learn_p && !(learn && learn[i])) ? 1 : 0;
            const int pre_flags = (have_pre ? 1 : 0) | (make_pre ? 2 : 0);
            const size_t lds = I.lds_base + ((learn_p && a.chol_in_lds) ? I.lds_adapt : 0);
            // does settling iteration it-1 swap a pair that straddles two groups? (same draw as the kernel: Philox is host/device)
            int gA = -1, gB = -1;
            if (L.pending && G > 1) {
                const int A = swap_pair_of(it - 1);
                if (A >= 0 && group_of(A, goff, G) != group_of(A + 1, goff, G)) { gA = group_of(A, goff, G); gB = group_of(A + 1, goff, G); }
            }
            // each of the two groups needs the other's k_loglike(it-1) before it settles the pair
            if (gA >= 0) if (int rc = exchange(grp.kb, gA, gB)) return rc;
            for (int g = 0; g < G; g++) {
                const int cnt = goff[g + 1] - goff[g];
                if (i < ib)
                    hipLaunchKernelGGL(k_iterate<true>, dim3(make_pre ? 2 * cnt : cnt), dim3(TB), lds, grp.gst[g], args, it, P, L.pending, L.rec(i), learn_p,
                                       I.adapt_scratch, goff[g], cnt, pre_flags, I.rgb ? rgb_device_slice(c, I.rgb_bmax, g) : rgb::Slice());
                else  // settle the last iteration of this stretch (MH test, swap, record, adaptation); nothing is proposed
                    hipLaunchKernelGGL(k_iterate<false>, dim3(cnt), dim3(TB), lds, grp.gst[g], args, it, P, L.pending, L.rec(i), learn_p, I.adapt_scratch,
                                       goff[g], cnt, 0, rgb::Slice());
            }
            have_pre = make_pre;
            // ... and must not overwrite (next iteration) what the other group's settle is still reading
            if (gA >= 0) if (int rc = exchange(grp.ki, gA, gB)) return rc;
            L.launched();
            if (i == ib) break;
            if (I.rgb) if (int rc = rgb_tables()) return rc;
            for (int g = 0; g < G; g++)
                if (int rc = evaluate(g, g == 0 ? T.lockstep_pair(i - ia, ev_every) : nullptr)) return rc;
        }
        I.last.set(1, P ^ 1);  // (the closing launch read the last proposals from parity P before the flip above)
        // join: the context stream continues after every group
        for (int g = 1; g < G; g++) if (int rc = hop(grp.join[g], grp.gst[g], st)) return rc;
        if (c->timing) {  // (with chain groups every launch carries C/G evaluations and overlaps the other groups' kernels)
            DCHK(hipStreamSynchronize(st));
            return T.drain_events((double)len * G, len * (long)a.C);
        }
        return TAMCMC_OK;
    }

    // Device-memory image of the two argument blocks, for the fused step's function calls (re-uploaded only when a pointer or size
    // changed since the last run; the candidates carried over from the last call were built for the old buffers then)
    int sync_arg_image() {
        const size_t n1 = (sizeof(DevSamplerArgs) + 15) & ~(size_t)15, n2 = sizeof(FusedArgs);
        std::vector<unsigned char> img(n1 + n2, 0);
        std::memcpy(img.data(), &args, sizeof(DevSamplerArgs));
        std::memcpy(img.data() + n1, &fu.f, sizeof(FusedArgs));
        if (!fu.d_argcopy) DCHK(I.mem.dalloc(&fu.d_argcopy, n1 + n2));
        if (img != fu.h_argcopy) {
            DCHK(hipMemcpyAsync(fu.d_argcopy, img.data(), n1 + n2, hipMemcpyHostToDevice, st));
            DCHK(hipStreamSynchronize(st));  // (img is a stack object)
            fu.h_argcopy = img;
            fu.disarm();
        }
        sc.ga = (const DevSamplerArgs *)fu.d_argcopy;
        sc.gf = (const FusedArgs *)(fu.d_argcopy + n1);
        return TAMCMC_OK;
    }

    // Entry of a fused stretch at iteration ia, unless the last call's final launch has prepared it (armed): L z of the first two
    // iterations, then the candidates of iteration ia built on the settled chains (state of parity q).  *launched: whether it was needed
    int fused_entry(long ia, bool *launched) {
        *launched = !fu.armed(it0 + ia, q);
        if (!*launched) return TAMCMC_OK;
        const int nbr = 8 * fu.f.NS;                // candidate roles, a multiple of 8 (keeps the tiles' XCD mapping)
        const int nlz2 = ((2 * a.C + 7) / 8) * 8;
        sc.it = it0 + ia; sc.rec = -1; sc.q = q; sc.flags = ST_LZ; sc.nbr = 0; sc.nlz = nlz2; sc.n_lz_live = 2 * a.C; sc.it_lz = it0 + ia; sc.q_lz = q;
        DCHK(launch_step(c->precision, c->K, nlz2, st, args, fu.f, lf[0], sc));
        sc.flags = ST_ENTRY; sc.nbr = nbr; sc.nlz = 0; sc.n_lz_live = 0;
        DCHK(launch_step(c->precision, c->K, nbr, st, args, fu.f, lf[0], sc));
        return TAMCMC_OK;
    }

    // Launch i of a stretch for chains [first, first + cnt): the tiles of iteration i (each decides iteration i-1 for its chain first),
    // the chains' commit workgroups (state, record and counters of iteration i-1), the candidates of iteration i+1, the L z of iteration
    // i+2.  A, A_prev: the swap pairs of iterations i and i-1; settled: the chains are settled (first launch of a stretch: nothing to
    // decide or commit).  ev: an event pair around the kernel, or null.
    int launch_group(int first, int cnt, int A, int A_prev, long i, bool settled, hipStream_t stream, hipEvent_t *ev = nullptr) {
        const bool owns_pair = A >= first && A + 1 < first + cnt;
        const int ntiles_pad = ((a.ntiles + 7) / 8) * 8;
        sc.it = it0 + i; sc.rec = ((samples || stats) && !settled) ? i - 1 : (long)-1; sc.q = q;
        sc.flags = ST_L | ST_BR | ST_LZ | ST_COMMIT | (settled ? ST_FIRST : 0);
#ifdef TAMCMC_PROBE  // timing experiments only (results are wrong): leave kinds of workgroups out of the launch
        if (const char *ep = getenv("TAMCMC_PROBE_STEP")) {
            const int pm = atoi(ep);
            if (pm & 1) sc.flags &= ~ST_BR;
            if (pm & 2) sc.flags &= ~ST_COMMIT;
            if (pm & 4) sc.flags &= ~ST_LZ;
            if (pm & 8) sc.flags |= ST_FIRST;
            if (pm & 16) sc.flags &= ~ST_L;
        }
#endif
        sc.first = first; sc.cnt = cnt; sc.extra = owns_pair ? 1 : 0; sc.pairA = settled ? -1 : A_prev;
        sc.nbr = 8 * (2 * cnt + (owns_pair ? 4 : 0)); sc.nlz = ((2 * cnt + 7) / 8) * 8; sc.n_lz_live = cnt; sc.it_lz = it0 + i + 2; sc.q_lz = q;
        LoglikeArgs lq = lf[(it0 + i) % 3];
        lq.B = cnt;
        lq.partials = fu.f.part + ((size_t)q * a.C + first) * a.ntiles * 2;
        DCHK(launch_step(c->precision, c->K, sc.nbr + sc.nlz + ntiles_pad * cnt, stream, args, fu.f, lq, sc, ev ? ev[0] : nullptr, ev ? ev[1] : nullptr));
        return TAMCMC_OK;
    }

    // After the last iteration ib-1 of a stretch: the commit workgroups alone (iteration ib-1 decided, the chains settled in parity q).
    int launch_close(int first, int cnt, long ib, hipStream_t stream) {
        sc.it = it0 + ib; sc.rec = (samples || stats) ? ib - 1 : (long)-1; sc.q = q;
        sc.flags = ST_COMMIT;
        sc.first = first; sc.cnt = cnt; sc.extra = 0;
        sc.nbr = 0; sc.nlz = ((cnt + 7) / 8) * 8; sc.n_lz_live = 0; sc.it_lz = 0; sc.q_lz = 0;
        DCHK(launch_step(c->precision, c->K, sc.nlz, stream, args, fu.f, lf[0], sc));
        return TAMCMC_OK;
    }

    int s1_waits_for_st() { return hop(grp.fork, st, grp.gst[1]); }
    int st_waits_for_s1() { return hop(grp.join[1], grp.gst[1], st); }

    // ---- (A) fused steps over [ia, ib) (no adaptation inside): one launch per iteration on the context stream, or two (one per chain group).
    // Two chain groups, each with its own launch per iteration on its own stream: a launch is a chain of dependent steps (sums ->
    // decision -> table rows -> tile, ~18 us even for five chains) that leaves most of the GPU idle at its two ends; the two groups'
    // launches fill each other's ends.  Nothing is shared between the groups' launches except at a swap whose pair (xsplit-1, xsplit)
    // straddles the groups.  For that iteration and the next (a window) the boundary moves by one chain -- [0, xsplit+1) on st,
    // [xsplit+1, C) on s1 -- so that the pair lies inside the first group's launch: st waits for s1 once on the way in (chain xsplit's
    // earlier launches are there), s1 waits for st once on the way out, and the rest of the second group keeps running through both
    // hops (profiles/r05_straddle_summary.md: the cost of the joint launches this replaces, and of what is left).  Only a window iteration whose own or previous pair is (xsplit, xsplit+1) is
    // still one joint launch over all chains, on st after both groups' earlier launches.  step_schedule.h (StepPlanner) decides all of
    // this, iteration by iteration, with every wait; here the plan is enqueued.  (Same chains bit for bit: the launches hold the same
    // workgroups, every buffer of the step is per chain, and a chain's cross candidates stay in the extra block named by f.xsplit.)
    int run_fused(long ia, long ib) {
        const long len = ib - ia;
        hipStream_t s1 = grp.gst[1];
        I.n.it_fused += len;
        I.n.n_stretch += 1;
        q = P;
        sc = StepCtl{};
        if (int rc = sync_arg_image()) return rc;
        sc.first = 0; sc.cnt = a.C; sc.extra = 1;
        bool entered;
        if (int rc = fused_entry(ia, &entered)) return rc;
        StepPlanner plan(split_ok, a.C, fu.f.xsplit);
        // does the context stream hold work of this call that the second group's stream has to wait for?  (Every entry point of the
        // library returns with its streams idle, so a call that starts on carried-over candidates has nothing to wait for: the event
        // hop would only delay the second group's first launch by 12-14 us, profiles/r05_straddle_summary.md.)
        plan.s1_must_wait = ia > 0 || entered;
        plan.s1_ahead = false;
        T.begin_fused(len);
        if (!split_ok && T.stretch_pair()) DCHK(hipEventRecord(T.stretch_pair()[0], st));
        long n_two = 0;
        int A_prev = -1;
        for (long i = ia; i < ib; i++) {
            const int A = swap_pair_of(it0 + i);
            const bool settled = i == ia;
            const StepPlan p = plan.next(A);
            if (p.st_waits_s1) if (int rc = st_waits_for_s1()) return rc;
            if (p.s1_waits_st) if (int rc = s1_waits_for_st()) return rc;
            if (int rc = launch_group(0, p.b, A, A_prev, i, settled, st)) return rc;
            if (p.b < a.C) {
                if (int rc = launch_group(p.b, a.C - p.b, A, A_prev, i, settled, s1, p.window ? nullptr : T.sampled_pair(i - ia))) return rc;
                n_two++;
                I.n.it_window += p.window ? 1 : 0;
            } else if (split_ok) I.n.it_joint += 1;
            A_prev = A;
            q ^= 1;
        }
        // the closing launches, over the ranges the last iteration's pair asks for (iteration ib-1's swap is decided by them)
        const StepPlan p = plan.next(-1);
        if (p.st_waits_s1) if (int rc = st_waits_for_s1()) return rc;
        if (p.s1_waits_st) if (int rc = s1_waits_for_st()) return rc;
        if (int rc = launch_close(0, p.b, ib, st)) return rc;
        if (p.b < a.C) {
            if (int rc = launch_close(p.b, a.C - p.b, ib, s1)) return rc;
            if (ib >= n_iter) s1_open = true;  // the call's last stretch: the host waits for both streams (no event hop on the GPU)
            else if (int rc = st_waits_for_s1()) return rc;
        }
        if (!split_ok && T.stretch_pair()) DCHK(hipEventRecord(T.stretch_pair()[1], st));  // (read after the call's final synchronisation)
        T.end_fused(len, split_ok, n_two);
        P = q;
        fu.arm(it0 + ib, q);
        I.last.set(2, 0);
        return TAMCMC_OK;
    }

    // ---- (C) k_env_step over [ia, ib) (no adaptation inside): one launch per iteration on the context stream, then a settle-only launch
    template <int KIND>
    int run_env_step_kind(long ia, long ib) {
        const long len = ib - ia;
        if (KIND == 0 && env_nchunk > ENV_STEP_MAX_CHUNKS) return TAMCMC_ERR_BAD_ARG;  // (k_env_step's chunk partials in LDS; prepare() never routes this here)
        fu.disarm();
        I.n.it_fused += len;
        I.n.n_stretch += 1;
        const size_t half = (size_t)a.C * a.ntiles * 2;
        const size_t lds = env_step_lds_bytes((size_t)a.desc.Np, (size_t)a.Nv);
        EnvStepArgs e;
        e.x = c->dx.p; e.y = c->dy.p; e.logx = c->dlogx.p;
        e.h = c->hx[1] - c->hx[0]; e.xmax = c->xmax; e.nchunk = env_nchunk;
        T.begin_fused(len);
        if (T.stretch_pair()) DCHK(hipEventRecord(T.stretch_pair()[0], st));
        SettleLoop L{P, samples || stats};
        for (long i = ia; i <= ib; i++) {
            DevSamplerArgs la_ = args;
            la_.partials = I.env.part.p + (size_t)P * half;  // what the previous launch of the stretch wrote
            e.part_wr = I.env.part.p + (size_t)(P ^ 1) * half;
            if (i < ib) hipLaunchKernelGGL((k_env_step<KIND, true>), dim3(a.ntiles, a.C), dim3(TB), lds, st, la_, e, it0 + i, P, L.pending, L.rec(i));
            else hipLaunchKernelGGL((k_env_step<KIND, false>), dim3(1, a.C), dim3(TB), lds, st, la_, e, it0 + i, P, L.pending, L.rec(i));
            L.launched();
        }
        DCHK(hipGetLastError());
        if (T.stretch_pair()) DCHK(hipEventRecord(T.stretch_pair()[1], st));  // (read after the call's final synchronisation)
        T.end_fused(len, false, 0);
        I.last.set(2, P ^ 1);  // (the closing launch read the last proposals from parity P before the flip above)
        return TAMCMC_OK;
    }
    int run_env_step(long ia, long ib) {
        return I.model_id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN ? run_env_step_kind<0>(ia, ib) : run_env_step_kind<1>(ia, ib);
    }

    // every launch is enqueued: the records, the wait for the streams, the kernel times
    int finish() {
        I.parity = P;
        DCHK(hipGetLastError());
        tl.mark();  // (every launch enqueued)
        double *const staged_smp = (samples && !zc_smp) ? samples : nullptr, *const staged_st = (stats && !zc_st) ? stats : nullptr;
        if (s1_open && (staged_smp || staged_st)) {  // (the copies below read what the second group's launches write)
            if (int rc = st_waits_for_s1()) return rc;
            s1_open = false;
        }
        DCHK(copy_records(staged_smp, staged_st, a, (size_t)n_iter, st));
        const bool poll = g_running_calls.load(std::memory_order_relaxed) == 1;
        if (s1_open) DCHK(Impl::wait_stream(grp.gst[1], poll));
        DCHK(Impl::wait_stream(st, poll));
        tl.mark();  // (streams idle)
        return T.total();
    }

    // ---- The Langevin engine (use_drift): per iteration k_mala_settle (settle it-1, propose it) -> the finite-difference batch of the
    // proposals (k_fd_unpack -- red giants: k_fd_rgb_perturb and the pre-step --, base k_loglike with model rows, k_loglike<DELTA>,
    // k_finalize x2) -> k_mala_test.  See dev_mala_impl.h.  Records go to the device buffers and are copied at the end of the call
    // (k_mala_settle has never written into mapped host memory: no device_view here).

    // The batch's layout follows the context's options (arithmetic mode, geometry, windowed differences): re-laid out when they change
    // (red giants: layout() also re-reserves the context's pre-step workspace for the batch's chunk -- another sampler or a direct
    // gradient call may have been the last to size it; the slice is taken from the context at every enqueue, never kept.  A route
    // the model has not -- the adjoint -- is refused by layout() with the chains where they were)
    int layout_batch() {
        FdBatch nb;
        int rc = nb.layout(c, FdBatch::Request::FromOptions, I.model_id, I.prior_class, a.C, (int64_t)a.desc.Np, I.h_plength.data(), a.Nv);
        if (rc) return rc;
        const bool need_bg = c->precision == TAMCMC_PRECISION_FAST && !V.bg.p;  // (a switch to FAST between two calls keeps every size)
        if (nb.total_bytes == V.fd.total_bytes && nb.route == V.fd.route && nb.ntiles == V.fd.ntiles && nb.rgb == V.fd.rgb &&
            nb.chunk == V.fd.chunk && V.block.p && !need_bg)
            return TAMCMC_OK;
        V.fd = nb;
        rc = ensure_poly(c);
        if (rc) return rc;
        DCHK(V.block.reserve(nb.total_bytes));
        FdInputs in;  // the layout's constants; the vectors come from the device at every enqueue, the steps from k_mala_steps
        in.priors = V.h_priors.data(); in.extra_priors = V.h_extra.data(); in.priors_switch = V.h_sw.data();
        in.plength = I.h_plength.data(); in.index_to_relax = V.h_idx.data();
        std::vector<unsigned char> hb(nb.head.in_bytes);
        nb.head.stage(hb.data(), in);
        DCHK(hipMemcpyAsync(V.block.p, hb.data(), nb.head.in_bytes, hipMemcpyHostToDevice, st));
        DCHK(hipStreamSynchronize(st));
        DCHK(nb.reserve(c, ws));
        V.grad_valid = false;
        return TAMCMC_OK;
    }

    // the kernels' arguments, the record buffers, where the adaptation works
    int prepare_langevin() {
        const size_t C = (size_t)a.C, Nv = (size_t)a.Nv, Np = (size_t)a.desc.Np;
        M = V.mala;
        M.fd_step_rel = V.fd_step_rel; M.delta = V.delta;
        if (I.env.on) {  // ids 0 / 1: the analytic batch's results, in the sampler's own buffers
            M.S = V.envb.g.S; M.lpp = V.envb.k.lpp; M.lpm = V.envb.k.lpm; M.st = nullptr; M.dlogL = V.envb.k.dlogL;
            M.h = V.envb.h; M.E = a.Nv + 1; M.deltas = 0;
        } else {
            FdBatch &fd = V.fd;
            db = V.block.p;
            fd.count_slots = c->timing && fd.hybrid();  // (hybrid red-giant batches: linearised / fallback slots of this call, counted on the device)
            if (fd.count_slots) DCHK(fd.zero_slot_counts(c, db));
            const FdResults res = fd.head.results(db);  // (the device block: read by k_mala_test)
            M.S = V.S.p; M.lpp = res.lpp; M.lpm = res.lpm; M.st = res.status; M.dlogL = nullptr;
            M.h = fd.head.hstep(db); M.E = fd.E; M.deltas = fd.deltas() ? 1 : 0;
        }
        if (int rc = I.reserve_records(samples != nullptr, stats != nullptr, (size_t)n_iter)) return rc;
        args = a;
        if (!samples) args.samples = nullptr;
        if (!stats) args.stats = nullptr;
        lds_settle = (4 * Nv + Np + 1 + 8) * sizeof(double) + 32;
        const size_t lds_test0 = (5 * Nv + 8) * sizeof(double) + 32, lds_adapt = (Nv * Nv + Nv) * sizeof(double);
        const bool chol_lds = lds_test0 + lds_adapt <= 156 * 1024;
        // (the adaptation's work area is reserved in every step when it fits: without adaptation the triangular solves keep the factor there)
        lds_test = lds_test0 + (chol_lds ? lds_adapt : 0);
        args.chol_in_lds = chol_lds ? 1 : 0;
        V.chol_lds = args.chol_in_lds;
        I.n.it_lockstep += n_iter;
        if (!chol_lds && !I.adapt_scratch) DCHK(I.mem.dalloc(&I.adapt_scratch, C * (Nv * Nv + 3 * Nv)));
        if (lds_test0 + lds_adapt > 64 * 1024 && chol_lds)
            DCHK(hipFuncSetAttribute(I.env.on ? (const void *)k_mala_test<true> : (const void *)k_mala_test<false>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_test0 + lds_adapt)));
        return TAMCMC_OK;
    }

    // ids 0 / 1, the analytic batch at the vectors d_params [C][Np]: rows and log-priors, the bins (envelope.hip's kernels on the
    // sampler's buffers), the chain rule; everything on the context stream, nothing leaves the device
    int env_batch(const double *d_params, hipEvent_t *pair) {
        const EnvMalaArgs &k = V.envb.k;
        const int npts = a.C * (2 * a.Nv + 1);
        if (pair) DCHK(hipEventRecord(pair[0], st));
        hipLaunchKernelGGL(k_env_mala_front, dim3((npts + 63) / 64), dim3(64), 0, st, args, k, d_params);
        DCHK(hipGetLastError());
        if (int rc = envelope_grad_stage_enqueue(c, I.model_id, a.C, a.env_rows, V.envb.g, st)) return rc;
        hipLaunchKernelGGL(k_env_mala_chain, dim3(a.C), dim3(128), 0, st, args, k, d_params);
        DCHK(hipGetLastError());
        if (pair) DCHK(hipEventRecord(pair[1], st));
        return TAMCMC_OK;
    }

    int batch(const double *d_params, hipEvent_t *pair) {
        if (I.env.on) return env_batch(d_params, pair);
        return V.fd.enqueue(c, db, d_params, ws, pair ? pair[0] : nullptr, pair ? pair[1] : nullptr);
    }

    // gradient at the chains' current positions (start of a run, new positions from outside)
    int initial_gradient() {
        if (V.grad_valid) return TAMCMC_OK;
        hipLaunchKernelGGL(k_mala_steps, dim3(1), dim3(256), 0, st, args, M);
        if (int rc = batch(a.params_cur + (size_t)P * a.C * a.desc.Np, nullptr)) return rc;
        hipLaunchKernelGGL(I.env.on ? k_mala_ginit<true> : k_mala_ginit<false>, dim3(a.C), dim3(TB), 2 * (size_t)a.Nv * sizeof(double), st, args, M, P);
        DCHK(hipGetLastError());
        V.grad_valid = true;
        return TAMCMC_OK;
    }

    int langevin_loop() {
        SettleLoop L{P, samples || stats};
        for (long i = 0; i <= n_iter; i++) {
            const long it = it0 + i;
            if (i < n_iter) hipLaunchKernelGGL(k_mala_settle<true>, dim3(a.C), dim3(TB), lds_settle, st, args, M, it, P, L.pending, L.rec(i));
            else hipLaunchKernelGGL(k_mala_settle<false>, dim3(a.C), dim3(TB), lds_settle, st, args, M, it, P, L.pending, L.rec(i));
            L.launched();
            if (i == n_iter) break;
            hipEvent_t *pair = T.batch_pair(i, n_iter);
            if (int rc = batch(a.params_prop, pair)) return rc;
            const int learn_i = (learn && learn[i]) ? factor_step_mode(I.factor_refresh, I.n_adapt++) : 0;
            hipLaunchKernelGGL(I.env.on ? k_mala_test<true> : k_mala_test<false>, dim3(a.C), dim3(TB), lds_test, st, args, M, it, P, learn_i, I.adapt_scratch);
            if (pair) {
                DCHK(hipStreamSynchronize(st));
                if (int rc = T.batch_sampled()) return rc;
                long bins = 0;  // what the delta launch really touched (roofline bookkeeping, as fd_run does)
                if (!I.env.on && V.fd.route == FdBatch::Route::Windowed) DCHK(V.fd.delta_stats(db, &bins, nullptr));
                T.batch_bins(bins);
            }
        }
        return TAMCMC_OK;
    }

    int finish_langevin() {
        I.parity = P;
        DCHK(hipGetLastError());
        DCHK(copy_records(samples, stats, a, (size_t)n_iter, st));
        DCHK(hipStreamSynchronize(st));
        long lin = 0, fall = 0;
        if (I.env.on) {  // (one pass over the bins per chain: C evaluations a batch)
            T.total_batches(n_iter, (long)a.C, false, 0, 0);
            return TAMCMC_OK;
        }
        if (V.fd.count_slots) DCHK(V.fd.hybrid_stats(c, db, &lin, &fall));
        T.total_batches(n_iter, (long)V.fd.B, V.fd.route == FdBatch::Route::Windowed, lin, fall);
        return TAMCMC_OK;
    }

    int run_mala() {
        fu.disarm();
        // Red giants under STRICT: the batch would need the host's long-double unpack of every proposal (FdBatch::h_prep), and the proposals
        // exist on the device only.  Refused here, before anything is enqueued or counted: state, iteration and gradients stay as they are
        if (I.rgb && c->precision == TAMCMC_PRECISION_STRICT) return TAMCMC_ERR_BAD_ARG;
        // ids 0 / 1: one gradient route, the analytic one, with buffers laid out at creation; no mode table, so no table-space adjoint --
        // refused like any route a model has not, with the chains where they were
        if (I.env.on) {
            if (c->gradient == TAMCMC_GRADIENT_ADJOINT) return TAMCMC_ERR_BAD_MODEL;
            I.last.set(1, 0);  // (download_envelope_rows: the Langevin step keeps its proposals in the first half of params_prop)
        } else if (int rc = layout_batch()) return rc;
        if (int rc = prepare_langevin()) return rc;
        if (int rc = initial_gradient()) return rc;
        if (int rc = langevin_loop()) return rc;
        return finish_langevin();
    }
};
