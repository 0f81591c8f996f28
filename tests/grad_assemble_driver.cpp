// Host driver of tests/test_grad_assemble.py: the one gradient assembly of tamcmc-c_amd/csrc/grad_assemble.h on the cases the test
// sends.  Numbers travel as hexadecimal bit patterns of doubles, so nothing is rounded on the way.
//   stdin, whitespace separated:
//     C Nvars Np share(0 full sums, 1 base + differences, 2 ready derivative) p has_prior has_status want_logPr0 want_grad_prior
//     params [C x Np]  index_to_relax [Nvars]  hstep [Nvars]  Tcoefs [C]  S [B | C + B | C]
//     dlogL [C x Nvars] (share 2)   lpp [B], lpm [B] (has_prior)   status [B] (has_status)            B = C (Nvars + 1)
//   stdout: the returned status; logL0 [C]; logPr0 [C] or "-"; grad [C x Nvars]; grad_prior [C x Nvars] or "-"
// Every array has its exact size on the heap: a read or write past one is an AddressSanitizer report in the sanitized build.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tamcmc-c_amd/csrc/grad_assemble.h"

static std::vector<double> read_doubles(size_t n) {
    std::vector<double> v(n);
    for (size_t i = 0; i < n; i++) {
        uint64_t b = 0;
        if (std::scanf("%" SCNx64, &b) != 1) std::exit(3);
        std::memcpy(&v[i], &b, 8);
    }
    return v;
}

static std::vector<int32_t> read_ints(size_t n) {
    std::vector<int32_t> v(n);
    for (size_t i = 0; i < n; i++)
        if (std::scanf("%" SCNd32, &v[i]) != 1) std::exit(3);
    return v;
}

static void print_doubles(const std::vector<double> *v) {
    if (!v) {
        std::printf("-\n");
        return;
    }
    for (double d : *v) {
        uint64_t b;
        std::memcpy(&b, &d, 8);
        std::printf("%016" PRIx64 " ", b);
    }
    std::printf("\n");
}

int main() {
    int C, Nvars, Np, share, has_prior, has_status, want_pr0, want_gp;
    double p;
    if (std::scanf("%d %d %d %d %lf %d %d %d %d", &C, &Nvars, &Np, &share, &p, &has_prior, &has_status, &want_pr0, &want_gp) != 9) return 2;
    const size_t c = (size_t)C, nv = (size_t)Nvars, B = c * (nv + 1);
    const std::vector<double> params = read_doubles(c * (size_t)Np);
    const std::vector<int32_t> idx = read_ints(nv);
    const std::vector<double> hstep = read_doubles(nv), T = read_doubles(c);
    const std::vector<double> S = read_doubles(share == 0 ? B : share == 1 ? c + B : c);
    std::vector<double> dlogL, lpp, lpm;
    std::vector<int32_t> status;
    if (share == 2) dlogL = read_doubles(c * nv);
    if (has_prior) { lpp = read_doubles(B); lpm = read_doubles(B); }
    if (has_status) status = read_ints(B);
    std::vector<double> logL0(c), logPr0(c), grad(c * nv), gp(c * nv);
    const tamcmc::LikelihoodShare kind = share == 0   ? tamcmc::LikelihoodShare::FullSums
                                         : share == 1 ? tamcmc::LikelihoodShare::Differences
                                                      : tamcmc::LikelihoodShare::Derivative;
    const int rc = tamcmc::assemble_gradient(C, Nvars, params.data(), Np, idx.data(), hstep.data(), T.data(), p, kind, S.data(),
                                             share == 2 ? dlogL.data() : nullptr, has_prior ? lpp.data() : nullptr,
                                             has_prior ? lpm.data() : nullptr, has_status ? status.data() : nullptr, logL0.data(),
                                             want_pr0 ? logPr0.data() : nullptr, grad.data(), want_gp ? gp.data() : nullptr);
    std::printf("%d\n", rc);
    print_doubles(&logL0);
    print_doubles(want_pr0 ? &logPr0 : nullptr);
    print_doubles(&grad);
    print_doubles(want_gp ? &gp : nullptr);
    return 0;
}
