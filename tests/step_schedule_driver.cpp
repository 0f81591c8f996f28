// Prints what csrc/step_schedule.h computes, for tests/test_step_schedule.py (plain C++: no HIP, no library).
//   step_schedule_driver <seed> <mask>...     a mask is a string of 0/1 (learn[i]), or null:<n> for "no learn array, n iterations"
// Output lines:
//   S <use_fused> <mask> <start>:<end>:<fused> ...       the stretches of a call, in the order run() takes them
//   P <C> <dN_mixing> <it> <swap_pair> <swap_draw>        iterations 0..200
//   J <C> <xsplit> <dN_mixing> <split_ok> <ia> <i> <joint>   the joint-launch rule over a fused stretch [ia, 200]
//   G <group of chain 0> ... <of chain 6>                 three groups [0,2) [2,5) [5,7)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../tamcmc-c_amd/csrc/rng.h"
#include "../tamcmc-c_amd/csrc/step_schedule.h"

using namespace tamcmc;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const uint64_t seed = strtoull(argv[1], nullptr, 10);
    for (int k = 2; k < argc; k++) {
        std::string learn;
        long n;
        const bool null = strncmp(argv[k], "null:", 5) == 0;
        if (null) n = atol(argv[k] + 5);
        else {
            for (const char *p = argv[k]; *p; p++) learn.push_back(*p == '1' ? 1 : 0);
            n = (long)learn.size();
        }
        for (int use_fused = 0; use_fused < 2; use_fused++) {
            printf("S %d %s", use_fused, argv[k]);
            long guard = 0;
            for (long i = 0, end = 0; i < n && guard <= n; i = end, guard++) {
                bool fused = false;
                next_stretch(null ? nullptr : learn.data(), n, i, use_fused != 0, &end, &fused);
                printf(" %ld:%ld:%d", i, end, fused ? 1 : 0);
            }
            printf("\n");
        }
    }
    const int Cs[5] = {1, 2, 3, 8, 20};
    const long dNs[4] = {0, 1, 3, 7};
    for (int C : Cs)
        for (long dN : dNs)
            for (long it = 0; it <= 200; it++) printf("P %d %ld %ld %d %d\n", C, dN, it, swap_pair(seed, C, dN, it, nullptr), swap_draw(seed, C, it, nullptr));
    const int shapes[2][2] = {{8, 4}, {20, 10}};
    for (const auto &s : shapes)
        for (long dN : dNs)
            for (int split_ok = 0; split_ok < 2; split_ok++)
                for (long ia : {1l, 6l}) {
                    int A_prev = swap_pair(seed, s[0], dN, ia - 1, nullptr);  // (what `first` must make the rule ignore)
                    for (long i = ia; i <= 200; i++) {
                        const int A = swap_pair(seed, s[0], dN, i, nullptr);
                        printf("J %d %d %ld %d %ld %ld %d\n", s[0], s[1], dN, split_ok, ia, i, joint_launch(split_ok != 0, s[1], A, A_prev, i == ia) ? 1 : 0);
                        A_prev = A;
                    }
                }
    const int goff[4] = {0, 2, 5, 7};
    printf("G");
    for (int ch = 0; ch < 7; ch++) printf(" %d", group_of(ch, goff, 3));
    printf("\n");
    return 0;
}
