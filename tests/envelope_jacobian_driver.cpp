// envelope_jacobian_driver.cpp -- env_row_jacobian of csrc/envelope_row.h through a plain C++ compiler (tests/test_envelope_gradient.py):
// prints, for every parameter vector on stdin ("<model id> <n> <n values>" per line, values as hex floats or decimals), first the
// constants of the analytic gradient's layout, then per vector the TAMCMC_ENVELOPE_GRAD_N x n entries d(row quantity q)/d(parameter j),
// row by row, as long-double hex floats.
#include <cstdio>
#include <vector>

#include "../include/tamcmc_hip.h"
#include "../tamcmc-c_amd/csrc/envelope_row.h"

int main() {
    using namespace tamcmc;
    static_assert(sizeof(EnvRow) == 192, "22 doubles and 4 ints");
    static_assert(ENV_GRAD_N == TAMCMC_ENVELOPE_GRAD_N && ENV_GRAD_NKSI == TAMCMC_ENVELOPE_KSI_N, "the audit entry's layout");
    std::printf("C %d %d %d %d %d\n", TAMCMC_ENVELOPE_GRAD_N, TAMCMC_ENVELOPE_KSI_N, ENV_GRAD_NRAW0, ENV_GRAD_NRAW1, TAMCMC_OPT_ENVELOPE_GRADIENT);
    int id, n;
    while (std::scanf("%d %d", &id, &n) == 2) {
        std::vector<double> p((size_t)n);
        for (int i = 0; i < n; i++)
            if (std::scanf("%la", &p[(size_t)i]) != 1) return 2;
        if (n != (id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN ? 19 : 10)) return 3;
        std::vector<long double> J((size_t)ENV_GRAD_N * n);
        env_row_jacobian(id, p.data(), J.data());
        std::printf("J");
        for (long double v : J) std::printf(" %La", v);
        std::printf("\n");
    }
    return 0;
}
