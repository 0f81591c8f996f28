// fd_rgb_chunk.h -- the chunk rule of a red-giant finite-difference batch (fd_batch.hip), plain C++ so that a host test can compile it
// (tests/fd_rgb_chunk_driver.cpp).
#pragma once
#include <stddef.h>

namespace tamcmc {

// Vectors per pass through the ONE pre-step workspace slice: as many as fit `budget` bytes at `per_vector` bytes each, at least one
// (a single vector larger than the budget still has to run), at most the batch; an empty batch gets 1 so that the chunk loop's step
// is never zero.
constexpr size_t FD_RGB_WORKSPACE = (size_t)256 << 20;
inline int fd_rgb_chunk(int B, size_t per_vector, size_t budget) {
    size_t n = per_vector ? budget / per_vector : (size_t)(B > 0 ? B : 1);
    if (n < 1) n = 1;
    return n < (size_t)(B > 0 ? B : 1) ? (int)n : (B > 0 ? B : 1);
}
// The same rule for the chains of a Fisher-information call (fisher.hip): a chain keeps the model rows of its 2 Nvars perturbed vectors on
// the device, 2 Nvars Nx 8 bytes; as many chains per pass as fit TAMCMC_OPT_FISHER_WORKSPACE_MB (default below), a single chain above the
// budget still runs alone.
constexpr size_t FISHER_WORKSPACE_MB = 2048;
inline size_t fisher_chain_bytes(int Nvars, long Nx) { return (size_t)2 * (size_t)(Nvars > 0 ? Nvars : 0) * (size_t)(Nx > 0 ? Nx : 0) * 8; }
inline int fisher_chunk(int C, int Nvars, long Nx, size_t budget_mb) { return fd_rgb_chunk(C, fisher_chain_bytes(Nvars, Nx), budget_mb << 20); }
// Red giants (ids 25 / 27, TAMCMC_OPT_RGB_FISHER): a chain is also E = 2 Nvars + 1 vectors of the pre-step, and the chains of a pass go
// through its ONE workspace slice together: the smaller of fisher_chunk() and the whole chains among the fd_rgb_chunk() vectors that fit
// `ws_budget` at `per_vector` bytes each (and among the 65535 vectors of a red-giant batch).  A single chain above either budget still
// runs alone (its vectors then take the slice in chunks, as any red-giant batch does).
inline int fisher_rgb_chunk(int C, int Nvars, long Nx, size_t budget_mb, size_t per_vector, size_t ws_budget) {
    const int rows = fisher_chunk(C, Nvars, Nx, budget_mb);
    const long E = 2 * (long)(Nvars > 0 ? Nvars : 0) + 1;
    long vectors = fd_rgb_chunk(65535, per_vector, ws_budget);
    long chains = vectors / E;
    if (chains < 1) chains = 1;
    return chains < rows ? (int)chains : rows;
}
// Chunks a batch of B vectors takes.
inline int fd_rgb_chunks(int B, int chunk) { return B > 0 ? (B + chunk - 1) / chunk : 0; }

}  // namespace tamcmc
