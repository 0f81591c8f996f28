// dev_sampler_state.h -- host state of the device-resident engine (included by dev_sampler.hip after the device headers, inside
// namespace tamcmc): DevSampler::Impl, composed of one part per launch scheme.  Every part owns its resources -- a failed init and
// ~DevSampler unwind by scope -- and names its invalidation.  Members of Impl itself are the chains' state and constants, which every
// scheme reads; a part's members are read by its scheme's driver only (and by init, info and the download of its own audit).

#define DCHK(call) HIPCHK(c, call)  // (c: the context, in scope wherever it is used)

template <typename T>
static hipError_t up(T *dst, const T *src, size_t n, hipStream_t st) {
    return hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, st);
}

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// Device allocations that live as long as the sampler (a buffer that is outgrown stays until then: launches may still read it)
struct DevArena : NoCopy {
    std::vector<void *> allocs;
    ~DevArena() { for (void *p : allocs) (void)hipFree(p); }
    template <typename T>
    hipError_t dalloc(T **p, size_t n) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, (n ? n : 1) * sizeof(T));
        if (e == hipSuccess) { allocs.push_back(q); *p = (T *)q; }
        return e;
    }
};

// ... and its events: timing pairs (timed) and the streams' hand-over events
struct EventArena : NoCopy {
    std::vector<hipEvent_t> all;
    ~EventArena() { for (hipEvent_t e : all) (void)hipEventDestroy(e); }
    hipError_t make(hipEvent_t *e, bool timed) {
        const hipError_t r = timed ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming);
        if (r == hipSuccess) all.push_back(*e);
        return r;
    }
};

struct DevSampler::Impl {
    // ---- chain groups: the chains are split into G contiguous groups, each on its own stream, so that one group's k_iterate overlaps
    // the other groups' k_loglike (an iteration is a serial k_iterate -> k_loglike chain per group).  (First member: its streams are
    // destroyed after every event -- Impl::events -- and every buffer.)
    struct Groups : NoCopy {
        int G = 1;
        hipStream_t gst[4] = {};  // gst[0]: the context's stream (borrowed); the others are this part's own
        hipEvent_t fork, kb[4], ki[4], join[4];  // (in Impl::events)
        ~Groups() { for (int g = 1; g < 4; g++) if (gst[g]) (void)hipStreamDestroy(gst[g]); }
        void choose(const DevSamplerInit &in, bool rgb);
        int create(Impl &I);
    } grp;

    // ---- the chains' state and constants (every scheme)
    tamcmc_hip_ctx *ctx = nullptr;
    DevSamplerArgs a{};
    DevArena mem;  // a's arrays, the parts' fixed-size arrays, the record buffers
    int parity = 0;  // which of the two state buffers holds the chains' current state
    int tile_rot = 0;  // launch-order hint of k_loglike (first near-field tile of chain 0's initial table)
    std::vector<int32_t> h_plength;
    int prior_class = 0, model_id = 0;
    bool rgb = false;  // ids 25 / 27: k_iterate leaves the table to the pre-step kernels (rgb_device_stage), lockstep scheme; Langevin step: the gradient batch builds the tables
    int rgb_bmax = 0;  // chains per workspace slice (one slice per chain group; Langevin step: unused after init)
    size_t lds_base = 0, lds_adapt = 0;  // k_iterate's dynamic LDS: the iteration's own, the adaptation's work area (0: in adapt_scratch)
    double *adapt_scratch = nullptr;  // per chain Nv^2 + 3 Nv: the work matrix, the deviation, the rank-one step's two coefficient vectors
    int factor_refresh = 0;  // R of TAMCMC_OPT_FACTOR_REFRESH (at creation)
    long n_adapt = 0;        // adapting iterations enqueued since creation: what the factor's schedule counts (step_schedule.h::factor_step_mode)
    size_t smp_cap = 0, stat_cap = 0;  // record buffers a.samples / a.stats, in doubles (reserve_records)
    EventArena events;  // every event of the sampler
    static constexpr int N_EV = 64, N_GEV = 8;
    hipEvent_t ev[N_EV][2];  // timing (KernelTiming): the low 48 pairs around sampled lockstep launches and Langevin batches, the top 16 around fused stretches
    struct PackBlock : NoCopy {  // state download: device gather block (in mem) and its pinned host image
        double *d = nullptr, *h = nullptr;
        ~PackBlock() { if (h) (void)hipHostFree(h); }
    } pack;

    // ---- (A) fused step: candidate sets, per-chain slots and threshold records, partial sums, L z (dev_step_impl.h)
    struct FusedStep {
        FusedArgs f{};
        bool ok = false;
        DevBuf<double> bg, part;  // the candidates' background series, the tiles' partial sums by parity (sized by RunCall::prepare)
        unsigned char *d_argcopy = nullptr;  // device image of {DevSamplerArgs, FusedArgs} as last launched, and its host shadow
        std::vector<unsigned char> h_argcopy;
        hipEvent_t gev[N_GEV][2];  // (in Impl::events) two chain groups: pairs around sampled launches of the second group (on its stream)
        // carried over between run() calls: the last launch of a fused stretch also prepares the candidates of the iteration that
        // follows and the L z of the one after; a call that continues right there starts without the two entry launches.  Whoever
        // writes chain state, the proposal law or a buffer the candidates were built for disarms
        long armed_it = -1;
        int armed_q = 0;
        void arm(long it, int q) { armed_it = it; armed_q = q; }
        void disarm() { armed_it = -1; }
        bool armed(long it, int q) const { return armed_it == it && armed_q == q; }
        int create(Impl &I, const DevSamplerInit &in);
    } fu;

    // ---- (C) envelope step, ids 0 / 1: no table; rows (a.env_rows), envelope.hip's kernels or k_env_step
    struct EnvStep {
        bool on = false;
        DevBuf<double> part;  // k_env_step: the tiles' partial sums by launch parity
    } env;

    // ---- Langevin step (use_drift): the finite-difference batch object, its device block and scratch, the per-chain work arrays
    struct Langevin {
        bool use_drift = false;
        double delta = 0, fd_step_rel = 1e-7;
        FdBatch fd;
        DevBuf<unsigned char> block;
        DevBuf<double> part, S, model, bg;
        FdBatch::Buffers ws() { return FdBatch::Buffers{part, S, model, bg}; }
        MalaArgs mala{};
        // ids 0 / 1 (TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN): no FdBatch; the analytic batch's buffers, the sampler's own (in Impl::mem) and
        // indexed by chain, sized once at creation (the spectrum's length is the engine's constant a.desc.Nx)
        struct EnvBatch {
            EnvMalaArgs k{};     // what k_env_mala_front and k_env_mala_chain read and write
            EnvGradBuffers g;    // what envelope.hip's kernels write between them
            double *h = nullptr; // [Nv] the steps
        } envb;
        bool grad_valid = false;  // a.grad_cur holds the gradient at the chains' positions (upload_state and a new batch layout invalidate)
        int chol_lds = -1;
        std::vector<double> h_priors, h_extra;  // host copies of the constants the batch's head is staged from
        std::vector<int32_t> h_idx, h_sw;
        int create(Impl &I, const DevSamplerInit &in);
    } lan;

    // ---- counters since creation (tamcmc_sampler_get_info)
    struct Counters {
        long it_fused = 0, it_lockstep = 0;  // iterations run by each scheme
        long n_stretch = 0;                  // fused stretches (the first launch of each has nothing to decide)
        long it_joint = 0, it_window = 0;    // of it_fused with two chain groups: iterations run as one launch / as a window (StepPlanner)
    } n;

    // ---- the last stretch run() enqueued: 1 lockstep, 2 fused / k_env_step, and the parity of its last proposals (download_tables,
    // download_envelope_rows; the fused step's candidates are not kept by parity)
    struct LastStretch {
        int scheme = 0, prop_parity = 0;
        void set(int scheme_, int prop_parity_) { scheme = scheme_; prop_parity = prop_parity_; }
    } last;

    // init, step by step (dev_sampler.hip)
    int validate(const DevSamplerInit &in);
    int rgb_workspace(const DevSamplerInit &in);
    int create_chain_state(const DevSamplerInit &in);
    int ready_to_read();
    void set_tile_rot(const double *params);
    int reserve_records(bool smp, bool st, size_t n_iter);
#ifdef TAMCMC_PROBE
    void probe_report() const;
#endif

    // The caller's record buffer as the device sees it when it is pinned, mapped host memory (tamcmc_hip_host_alloc): the settle step then
    // writes the records straight into it (15 KB per iteration over PCIe, posted) and a call ends without its two device-to-host copies.
    // (asked on every call: an address says nothing about what the caller has freed and allocated since the last one)
    static double *device_view(const double *host, size_t bytes) {
        if (!host || !bytes) return nullptr;
        double *d = nullptr;
        void *dp = nullptr, *dq = nullptr;
        const char *last = (const char *)host + bytes - 1;
        // hipHostGetDevicePointer fails for pageable memory and returns the device address of THIS address for page-locked, mapped memory.
        // The whole record block [host, host + bytes) must lie inside ONE mapping: the last byte has to be page-locked too and map to the
        // first byte's device address + bytes - 1 -- a pinned buffer shorter than the call's records, or an interior pointer near the
        // end of one, would otherwise make the settle step write outside the mapping (a GPU fault instead of a host-side error)
        if (hipHostGetDevicePointer(&dp, const_cast<double *>(host), 0) == hipSuccess && dp &&
            hipHostGetDevicePointer(&dq, const_cast<char *>(last), 0) == hipSuccess && dq == (char *)dp + bytes - 1)
            d = (double *)dp;
        else (void)hipGetLastError();  // (pageable memory, or not one mapping over the whole block: the staged copy is used)
        return d;
    }

    // End of a call: the host waits for a stream by polling it for up to a millisecond before it blocks.  A blocking wait parks the
    // thread on an interrupt and wakes tens of microseconds after the last kernel has finished -- a tenth of a 20-iteration call (the
    // reference writes its ring buffer every Nbuffer iterations; a caller with short buffers makes short calls).
    // (only when this is the process's one running call: several host threads polling -- co-resident stars, tamcmc_sampler_run_packed --
    // would contend for the runtime's locks with the threads that are still enqueuing)
    static hipError_t wait_stream(hipStream_t st, bool poll) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int spin = 0; poll; spin++) {
            const hipError_t e = hipStreamQuery(st);
            if (e != hipErrorNotReady) return e;
            if ((spin & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(1000)) break;
        }
        (void)hipGetLastError();  // (hipErrorNotReady is sticky in the last-error slot)
        return hipStreamSynchronize(st);
    }

    struct KernelTiming;
    struct RunCall;  // one run() call
};
