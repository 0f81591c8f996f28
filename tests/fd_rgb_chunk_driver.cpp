// Prints what the chunk rule of a red-giant finite-difference batch gives (tamcmc-c_amd/csrc/fd_rgb_chunk.h) for the cases named on
// the command line as "B per_vector budget" triples; tests/test_fd_rgb_chunk.py restates the expectations.
#include <cstdio>
#include <cstdlib>

#include "../tamcmc-c_amd/csrc/fd_rgb_chunk.h"

int main(int argc, char **argv) {
    for (int i = 1; i + 2 < argc; i += 3) {
        const int B = std::atoi(argv[i]);
        const size_t per = std::strtoull(argv[i + 1], nullptr, 10), budget = std::strtoull(argv[i + 2], nullptr, 10);
        const int chunk = tamcmc::fd_rgb_chunk(B, per, budget);
        // every vector is covered exactly once by [b0, b0 + n) with n <= chunk
        long covered = 0;
        int worst = 0;
        for (int b0 = 0; b0 < B; b0 += chunk) {
            const int n = B - b0 < chunk ? B - b0 : chunk;
            covered += n;
            if (n > worst) worst = n;
        }
        std::printf("%d %d %ld %d\n", chunk, tamcmc::fd_rgb_chunks(B, chunk), covered, worst);
    }
    std::printf("default_budget %zu\n", (size_t)tamcmc::FD_RGB_WORKSPACE);
    return 0;
}
