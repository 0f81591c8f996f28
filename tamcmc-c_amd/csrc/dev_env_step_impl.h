// dev_env_step_impl.h -- the Gaussian-envelope models' one-launch iteration (included by dev_sampler.hip, inside its anonymous namespace,
// after dev_iterate_impl.h, whose pieces it is made of).
//
// The lockstep route of ids 0 / 1 is two or three dependent launches per iteration (k_iterate -> k_env_ksi (id 0) -> k_env_eval), each a
// few microseconds of work behind a launch latency: a spectrum of these fits has 5-32 tiles of 1024 bins.  Outside learning iterations
// the control work of an iteration is tiny (Nv <= 18: one MH test, an 18 x 18 triangular product, a serial prior of <= 19 terms, a row
// of 22 scalars), so EVERY tile workgroup of a chain does all of it for itself, from the same inputs with the same code -- hence the
// same bits in every sibling, no hand-off inside a launch -- and then evaluates its own tile:
//   k_env_step, grid (tiles, chains), 256 threads.  Workgroup (t, m)
//     (0) settles the pending iteration it-1 for chain m as k_iterate does (settle_chain: accept_result for m and, in a swap iteration,
//         for the partner, resolve_swap);
//     (1) draws the normals, forms x' = x + L z, the log-prior and the row (propose_position, env_front) in LDS;
//     (2) id 0: forms the three xi sums over the WHOLE spectrum in k_env_ksi's order (per 4096-bin chunk the strided per-thread sums
//         and the block reduction), then the chunk partials in k_env_eval's order: xi has the lockstep route's bits;
//     (3) evaluates tile t (env_tile, k_env_eval's body) and writes its tile partial.
//   Only tile 0 of a chain writes chain state, counters, records and the row block (the audit's copy); only parity-buffered arrays are
//   written, as in k_iterate.  Launch i reads the tile partials launch i-1 wrote while its siblings write their own: the partials exist
//   twice, by parity, in a buffer the sampler owns.  A stretch ends with a settle-only launch (one workgroup per chain); nothing is
//   carried over to the next stretch or call but the chains' state.  One stream, no chain groups.
// The redundant work grows with the tile count, and for id 0 every tile walks the whole spectrum once more for xi: the step serves
// spectra up to env_step_max_bins() bins (envelope_row.h: 32 768 for id 1, the measured crossover of 6 144 for id 0); above that the
// lockstep route runs.

struct EnvStepArgs {
    const double *x, *y, *logx;
    double h, xmax;    // get_ksinorm's step x(1) - x(0); the largest x (leakage filter)
    int nchunk;        // 4096-bin chunks of the xi pass (id 0: <= ENV_STEP_MAX_CHUNKS, the size of s_ksi)
    double *part_wr;   // [C x tiles x 2] the half of the partials this launch writes (DevSamplerArgs::partials: the half it reads)
};

template <int KIND, bool PROPOSE>  // KIND: model id (0 Kallinger, 1 Harvey)
__global__ void __launch_bounds__(TB) k_env_step(const DevSamplerArgs a, const EnvStepArgs e, const long it, const int P, const int pending,
                                                const long rec) {
    static_assert(TB == EWG, "the tile bodies of envelope_row.h are written for this workgroup");
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int Np = a.desc.Np, Nv = a.Nv, C = a.C;
    double *s_params = (double *)s_raw;  // [Np]   current, then proposed parameter vector
    double *s_vars = s_params + Np;      // [Nv]   current, then proposed variables
    double *s_z = s_vars + Nv;           // [Nv+1] normals
    double *s_pv = s_z + Nv + 1;         // [Nv], [Np]: where the tiles that do not write the chain's proposal put it
    double *s_pp = s_pv + Nv;
    __shared__ double s_red[3 * (TB / 64)];
    __shared__ double s_coef[3];
    __shared__ double s_ksi[3 * ENV_STEP_MAX_CHUNKS];
    __shared__ EnvRow s_row;
    __shared__ AcceptOut s_own, s_partner;
    __shared__ double s_lp;
    __shared__ int s_st;
    const int tile = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
    const bool writer = tile == 0;
    const int Q = P ^ 1;

    // (0) settle the pending iteration (never a learning one: the host routes those to the lockstep kernels)
    settle_chain(a, m, it, P, pending, rec, 0, writer, s_vars, s_params, s_z, s_red, &s_own, &s_partner);
    if (!PROPOSE) return;
    __syncthreads();

    // (1) propose iteration `it`
    normals_into(a, m, it, s_z);
    __syncthreads();
    propose_position(a, m, writer ? a.vars_prop + ((size_t)Q * C + m) * Nv : s_pv, writer ? a.params_prop + ((size_t)Q * C + m) * Np : s_pp, s_vars,
                     s_params, s_z, nullptr);
    env_front(a.desc, s_params, &s_row, &s_lp, &s_st);
    __syncthreads();
    if (writer) {
        if (tid == 0) {
            a.logPr_prop[Q * C + m] = s_lp;
            a.status_prop[Q * C + m] = s_st;
        }
        static_assert(sizeof(EnvRow) % 8 == 0 && sizeof(EnvRow) / 8 <= TB, "row copied as 64-bit words, one per lane");
        if (tid < (int)(sizeof(EnvRow) / 8)) ((unsigned long long *)(a.env_rows + m))[tid] = ((const unsigned long long *)&s_row)[tid];
    }

    // (2) id 0: the normalisations of the three super-Lorentzians
    const int Nx = a.desc.Nx;
    if (KIND == 0) {
        for (int ch = 0; ch < e.nchunk; ch++) {
            double out[3];
            env_ksi_chunk(e.logx, Nx, ch, s_row, s_red, out);
            if (tid == 0) {
                s_ksi[3 * ch] = out[0];
                s_ksi[3 * ch + 1] = out[1];
                s_ksi[3 * ch + 2] = out[2];
            }
            __syncthreads();
        }
        env_ksi_coef(s_ksi, e.nchunk, e.h, s_row, s_red, s_coef);
    }

    // (3) this workgroup's tile
    double out[2];
    env_tile<KIND, false>(e.x, e.y, e.logx, Nx, tile, e.xmax, s_row, s_coef, nullptr, s_red, out);
    if (tid == 0) {
        double *p = e.part_wr + ((size_t)m * a.ntiles + tile) * 2;
        p[0] = out[0];
        p[1] = out[1];
    }
}

__host__ inline size_t env_step_lds_bytes(size_t Np, size_t Nv) { return (2 * Np + 3 * Nv + 1) * sizeof(double) + 16; }
