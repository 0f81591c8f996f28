// Prints what tamcmc-c_amd/csrc/fisher_rgb_rule.h chooses for each triple of hand-made tables named on the command line, one line per case:
// "status_base status_plus status_minus n_base n_plus n_minus x0 x_plus x_minus", then the rows "l fc" of the base table, of the table at
// theta + h e_k and of the one at theta - h e_k; a case follows the other.  Per case: form, reciprocal index, substituted side, the two
// freeze flags, and the reciprocal taken from the three candidates formed as fisher.hip forms them (%a).  Last line: the enum values.
// With "chunk" as the first word: the pass rule of a red-giant call (fd_rgb_chunk.h: fisher_rgb_chunk) for the cases
// "C Nvars Nx budget_MiB per_vector ws_budget".  tests/test_rgb_fisher_rule.py makes the cases and states what it expects.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tamcmc-c_amd/csrc/fd_rgb_chunk.h"
#include "../tamcmc-c_amd/csrc/fisher_rgb_rule.h"

static int chunks(int argc, char **argv) {
    for (int i = 2; i + 5 < argc; i += 6) {
        const int C = std::atoi(argv[i]), Nv = std::atoi(argv[i + 1]);
        const long Nx = std::atol(argv[i + 2]);
        const size_t mb = std::strtoull(argv[i + 3], nullptr, 10), pv = std::strtoull(argv[i + 4], nullptr, 10),
                     wsb = std::strtoull(argv[i + 5], nullptr, 10);
        const int chunk = tamcmc::fisher_rgb_chunk(C, Nv, Nx, mb, pv, wsb);
        long covered = 0;
        for (int c0 = 0; c0 < C; c0 += chunk) covered += C - c0 < chunk ? C - c0 : chunk;
        std::printf("%d %d %ld %zu\n", chunk, tamcmc::fd_rgb_chunks(C, chunk), covered, tamcmc::fisher_chain_bytes(Nv, Nx));
    }
    std::printf("workspace %zu\n", (size_t)tamcmc::FD_RGB_WORKSPACE);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "chunk")) return chunks(argc, argv);
    int i = 1;
    while (i + 8 < argc) {
        int st[3], n[3];
        for (int q = 0; q < 3; q++) { st[q] = std::atoi(argv[i + q]); n[q] = std::atoi(argv[i + 3 + q]); }
        const double x0 = std::strtod(argv[i + 6], nullptr);
        volatile double xp = std::strtod(argv[i + 7], nullptr), xm = std::strtod(argv[i + 8], nullptr);
        i += 9;
        if (n[0] < 0 || n[1] < 0 || n[2] < 0 || i + 2 * (n[0] + n[1] + n[2]) > argc) return 2;
        // (exactly the rows named: an access beyond a table's count is the sanitizer's to find)
        std::vector<tamcmc_multiplet> t[3];
        for (int q = 0; q < 3; q++) {
            t[q].resize((size_t)n[q]);
            for (int j = 0; j < n[q]; j++, i += 2) {
                t[q][(size_t)j] = tamcmc_multiplet();
                t[q][(size_t)j].l = std::atoi(argv[i]);
                t[q][(size_t)j].fc = std::strtod(argv[i + 1], nullptr);
            }
        }
        const tamcmc::FisherRgbChoice ch =
            tamcmc::fisher_rgb_choose_tables(st[0], st[1], st[2], t[0].data(), n[0], t[1].data(), n[1], t[2].data(), n[2]);
        const double rh3[3] = {1.0 / (xp - xm), 1.0 / (xp - x0), 1.0 / (x0 - xm)};
        std::printf("%d %d %d %d %d %a\n", ch.form, ch.rh, ch.substitute, ch.freeze_plus ? 1 : 0, ch.freeze_minus ? 1 : 0, rh3[ch.rh]);
    }
    std::printf("forms %d %d %d %d rh %d %d %d sides %d %d %d\n", tamcmc::FISHER_RGB_FAILED, tamcmc::FISHER_RGB_CENTRAL, tamcmc::FISHER_RGB_ONE_SIDED,
                tamcmc::FISHER_RGB_UNFROZEN, tamcmc::FISHER_RGB_RH_CENTRAL, tamcmc::FISHER_RGB_RH_PLUS, tamcmc::FISHER_RGB_RH_MINUS,
                tamcmc::FISHER_RGB_SIDE_NONE, tamcmc::FISHER_RGB_SIDE_PLUS, tamcmc::FISHER_RGB_SIDE_MINUS);
    return 0;
}
