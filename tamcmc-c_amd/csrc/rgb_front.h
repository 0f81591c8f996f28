// rgb_front.h -- the red-giant front end on the device: what stages ONE parameter vector (LDS) for the mixed-mode solver.  Its class-4
// log-prior (priors_calc.cpp:319-512: generic terms by lane, each kernel's own loop, then pr::prior_serial's
// constraints, ordered sum and smoothness tail by one lane), the scalar unpack (rgb_unpack.h) by one wave, and the result published
// into entry rb of a pre-step workspace slice and the vector's slot of a table block; rgb_device_stage (rgb_prestep.hip) builds the
// table from there.
// Two kernels are made of these pieces, each with its own schedule, barriers and rule for a prior that is dead or cannot be evaluated:
// the sampler's proposal (propose_common, dev_iterate_impl.h: 256 lanes take the terms, workgroup barriers) and the gradient batch's
// k_fd_rgb_perturb (fd_batch.hip: wave 0 takes the whole prior beside wave 1's unpack).  No piece knows which of them calls it.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_unpack.h"
#include "kernels.h"
#include "rgb_unpack.h"

namespace tamcmc {
namespace rgb {

// The staging record, declared __shared__ by each kernel
struct FrontLds {
    Prep P;
    RowIn R;
    double w[40];                              // the unpacking wave's scratch (WaveLanes)
    double noise[3 * TAMCMC_MAX_HARVEY + 4];   // the vector's noise row
    double lp;                                 // its log-prior
    int32_t hn[2];                             // nharvey, nnoise
    int stp;                                   // status of the prior: TAMCMC_OK, or why the device cannot evaluate it
};

// The serial tail, by ONE lane, behind a barrier of the lanes that took the generic terms: F.lp, F.stp.  st: what the terms left; terms
// may be nullptr (prior_serial then evaluates them itself)
__device__ __forceinline__ void front_prior_serial(const ModelDesc &d, const double *s_params, const mt::xreal *terms, int st, FrontLds &F) {
    F.lp = (double)pr::prior_serial(d.prior_class, s_params, d.plength, d.Np, d.priors, d.priors_switch, d.extra, &st, terms);
    F.stp = st;
}

// The scalar unpack of the vector, by the 64 lanes of ONE wave (it reads s_params only): F.P, F.R, F.noise, F.hn
__device__ __forceinline__ void front_unpack(const ModelDesc &d, const double *s_params, const Slice &rs, FrontLds &F) {
    WaveLanes x;
    x.w = F.w;
    double fmin;
    unpack_vector(x, s_params, d.plength, rs.step, d.model_id == TAMCMC_MODEL_RGB_ASYMPT_AJ_CTEWIDTH_V4_ID /* the constant-width law */, rs.dense, F.P,
                  F.R, F.noise, &F.hn[0], &F.hn[1], &fmin);
}

// The solver's counters of entry rb, by ONE lane
__device__ __forceinline__ void front_reset(const Slice &rs, int rb) {
    rs.norm_bits[rb] = 0ull;
    rs.nsol[rb] = 0;
}

// F -> entry rb of the slice and slot `slot` of the table block (noise rows of `stride` doubles), by the NT lanes of the workgroup,
// behind a workgroup barrier
template <int NT>
__device__ __forceinline__ void front_publish(const FrontLds &F, const Slice &rs, int rb, int slot, int stride, double *noise, int *nh, int *nn) {
    const int tid = threadIdx.x;
    static_assert(sizeof(Prep) % 8 == 0 && sizeof(RowIn) % 8 == 0, "copied as doubles");
    const double *src = (const double *)&F.P;
    double *dst = (double *)&rs.preps[rb];
    for (int i = tid; i < (int)(sizeof(Prep) / 8); i += NT) dst[i] = src[i];
    src = (const double *)&F.R;
    dst = (double *)&rs.rows[rb];
    for (int i = tid; i < (int)(sizeof(RowIn) / 8); i += NT) dst[i] = src[i];
    for (int i = tid; i < F.hn[1] && i < stride; i += NT) noise[(size_t)slot * stride + i] = F.noise[i];
    if (tid == 0) {
        front_reset(rs, rb);
        nh[slot] = F.hn[0];
        nn[slot] = F.hn[1];
    }
}

}  // namespace rgb
}  // namespace tamcmc
