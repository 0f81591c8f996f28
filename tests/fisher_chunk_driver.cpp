// Prints what the chunk rule gives for the chains of a Fisher-information call (tamcmc-c_amd/csrc/fd_rgb_chunk.h: fisher_chunk) for the
// cases named on the command line as "C Nvars Nx budget_MiB" quadruples; tests/test_fisher_numpy.py restates the expectations.
#include <cstdio>
#include <cstdlib>

#include "../tamcmc-c_amd/csrc/fd_rgb_chunk.h"

int main(int argc, char **argv) {
    for (int i = 1; i + 3 < argc; i += 4) {
        const int C = std::atoi(argv[i]), Nv = std::atoi(argv[i + 1]);
        const long Nx = std::atol(argv[i + 2]);
        const size_t mb = std::strtoull(argv[i + 3], nullptr, 10);
        const int chunk = tamcmc::fisher_chunk(C, Nv, Nx, mb);
        long covered = 0;
        for (int c0 = 0; c0 < C; c0 += chunk) covered += C - c0 < chunk ? C - c0 : chunk;
        std::printf("%d %d %ld %zu\n", chunk, tamcmc::fd_rgb_chunks(C, chunk), covered, tamcmc::fisher_chain_bytes(Nv, Nx));
    }
    std::printf("default_budget_mb %zu\n", (size_t)tamcmc::FISHER_WORKSPACE_MB);
    return 0;
}
