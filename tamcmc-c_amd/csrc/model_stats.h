// model_stats.h -- posterior model spectrum (model_stats.hip): per-bin statistics of the model M over a stream of parameter vectors,
// accumulated on the device.  Launch interface of k_model_stats and the table stages it shares with tamcmc_hip_loglike_params_batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "ctx.h"

namespace tamcmc {

// The seven per-bin accumulators, one plane of Nx doubles each, `plane` doubles apart (the law: include/tamcmc_hip.h).
enum { MS_R = 0, MS_A1, MS_A2, MS_MIN, MS_MAX, MS_Q, MS_G, MS_PLANES };

constexpr int MS_TILE = 256;  // bins per workgroup: four waves, one bin per lane

struct ModelStatsArgs {
    LoglikeArgs a;          // spectrum and the staged tables of the launch's a.B vectors (x, y, Nx, mults, offsets, noise, nharvey, nnoise)
    const double *weights;  // [B]
    const int32_t *status;  // [B] table status of each vector, in device memory (0 = the table is good)
    double *planes;         // [MS_PLANES x plane]
    size_t plane;
    int have_ref;           // a vector was accepted before this launch: the planes hold its reference row and the running sums
};

// One launch = the a.B vectors of one chunk, walked in index order by every tile's workgroup; ceil(Nx / MS_TILE) workgroups.
hipError_t launch_model_stats(const ModelStatsArgs &m, hipStream_t st);

// the host table stage of tamcmc_hip_loglike_params_batch (capi.hip: ids 3, 11, 12, 13, 14, 23), tables left in c->h_stage
int stage_params_host(tamcmc_hip_ctx *c, int model_id, int B, const double *params, int64_t Nparams, const int32_t *plength, int32_t *status,
                      int *per_out, int *stride_out, int *first_err);

}  // namespace tamcmc
