// Host driver of tests/test_fd_block.py: the head of the gradient batch's block (tamcmc-c_amd/csrc/fd_block.h) for one (C, Np, Nvars).
//   argv: C Np Nvars present   (present = 1: every input given, 0: every optional input null -- all of them are optional)
//   line 1: o_params o_h o_pr o_ex o_pl o_idx o_sw in_bytes o_lpp o_lpm o_st out_bytes
//   line 2: the block after stage(), in hex: [0, in_bytes) and the 64 guard bytes behind (pre-filled with 0xA5)
//   line 3: B, then the bytes of lpp, lpm, status as results() sees them in a block holding the counting pattern byte i = i mod 256
//   line 4: first_status() of statuses all zero; of -5 in the last slot alone; of -4 in slot 0 and -5 in the last
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tamcmc-c_amd/csrc/fd_block.h"

// byte k of input array j (0 params, 1 hstep, 2 priors, 3 extra_priors, 4 plength, 5 index_to_relax, 6 priors_switch): never zero
static std::vector<unsigned char> pattern(int j, size_t n) {
    std::vector<unsigned char> v(n ? n : 1);
    for (size_t k = 0; k < n; k++) v[k] = (unsigned char)(1 + (j * 37 + k * 11) % 250);
    return v;
}

static void hex(const unsigned char *p, size_t n) {
    for (size_t i = 0; i < n; i++) std::printf("%02x", p[i]);
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const int C = std::atoi(argv[1]), Np = std::atoi(argv[2]), Nvars = std::atoi(argv[3]), present = std::atoi(argv[4]);
    const tamcmc::FdBlockHead H(C, Np, Nvars);
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", H.o_params, H.o_h, H.o_pr, H.o_ex, H.o_pl, H.o_idx, H.o_sw, H.in_bytes, H.o_lpp,
                H.o_lpm, H.o_st, H.out_bytes);
    const size_t c = (size_t)C, np = (size_t)Np, nv = (size_t)Nvars, B = c * (nv + 1);
    // exact-size heap arrays: a copy that reads past an input, or writes past in_bytes + guard, is an AddressSanitizer report
    const std::vector<unsigned char> a0 = pattern(0, c * np * 8), a1 = pattern(1, nv * 8), a2 = pattern(2, 4 * np * 8), a3 = pattern(3, 80),
                                     a4 = pattern(4, 44), a5 = pattern(5, nv * 4), a6 = pattern(6, np * 4);
    tamcmc::FdInputs in;
    if (present) {
        in.params = (const double *)a0.data(); in.hstep = (const double *)a1.data(); in.priors = (const double *)a2.data();
        in.extra_priors = (const double *)a3.data(); in.plength = (const int32_t *)a4.data(); in.index_to_relax = (const int32_t *)a5.data();
        in.priors_switch = (const int32_t *)a6.data();
    }
    std::vector<unsigned char> blk(H.in_bytes + 64, 0xA5);
    H.stage(blk.data(), in);
    hex(blk.data(), blk.size());
    std::printf("\n");

    std::vector<unsigned char> full(H.in_bytes + H.out_bytes);
    for (size_t i = 0; i < full.size(); i++) full[i] = (unsigned char)(i & 255);
    tamcmc::FdResults r = H.results(full.data());
    std::printf("%d ", r.B);
    hex((const unsigned char *)r.lpp, B * 8);
    std::printf(" ");
    hex((const unsigned char *)r.lpm, B * 8);
    std::printf(" ");
    hex((const unsigned char *)r.status, B * 4);
    std::printf("\n");

    std::vector<int> st(B, 0);
    r.status = st.data();
    const int f0 = r.first_status();
    st[B - 1] = -5;
    const int f1 = r.first_status();
    st[0] = -4;
    const int f2 = r.first_status();
    std::printf("%d %d %d\n", f0, f1, f2);
    return 0;
}
