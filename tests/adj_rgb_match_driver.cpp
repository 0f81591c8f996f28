// Prints the class tamcmc-c_amd/csrc/adj_rgb_match.h gives each pair of hand-made tables named on the command line, one number per case:
// "status_base status_pert n_base n_pert" then n_base rows "l fc" of the base table and n_pert rows of the perturbed one; a case follows
// the other.  Last line: the three class values and the flag.  tests/test_adj_rgb_match.py makes the cases and states what it expects.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tamcmc-c_amd/csrc/adj_rgb_match.h"

int main(int argc, char **argv) {
    int i = 1;
    while (i + 3 < argc) {
        const int st0 = std::atoi(argv[i]), st1 = std::atoi(argv[i + 1]), n0 = std::atoi(argv[i + 2]), n1 = std::atoi(argv[i + 3]);
        i += 4;
        if (n0 < 0 || n1 < 0 || i + 2 * (n0 + n1) > argc) return 2;
        std::vector<tamcmc_multiplet> t((size_t)n0 + n1 + 1);
        for (int j = 0; j < n0 + n1; j++, i += 2) {
            t[j] = tamcmc_multiplet();
            t[j].l = std::atoi(argv[i]);
            t[j].fc = std::strtod(argv[i + 1], nullptr);
        }
        std::printf("%d\n", tamcmc::adj_rgb_class(st0, st1, t.data(), n0, t.data() + n0, n1));
    }
    std::printf("classes %d %d %d flag %d\n", tamcmc::ADJ_RGB_FAILED, tamcmc::ADJ_RGB_LINEARISABLE, tamcmc::ADJ_RGB_FALLBACK, tamcmc::ADJ_RGB_FLAG_LINEAR);
    return 0;
}
