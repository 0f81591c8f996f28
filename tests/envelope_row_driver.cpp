// envelope_row_driver.cpp -- the host side of csrc/envelope_row.h through a plain C++ compiler (tests/test_envelope_row.py): prints, for
// every parameter vector on stdin ("<model id> <n> <n values>" per line, values as hex floats or decimals), the EnvRow fields in the
// order of tamcmc_sampler_get_envelope_rows as hex floats, and first the constants the sampler's routing uses.
#include <cstdio>
#include <vector>

#include "../include/tamcmc_sampler.h"
#include "../tamcmc-c_amd/csrc/envelope_row.h"

int main() {
    using namespace tamcmc;
    static_assert(sizeof(EnvRow) == 192, "22 doubles and 4 ints");
    static_assert(TAMCMC_ENVELOPE_ROW_N == 24, "the audit entry's layout");
    std::printf("C %d %d %d %d %d %d %d\n", ETILE, ECHUNK, ENV_STEP_MAX_BINS, ENV_STEP_MAX_BINS_KSI, ENV_STEP_MAX_CHUNKS,
                env_step_max_bins(TAMCMC_MODEL_KALLINGER2014_GAUSSIAN), env_step_max_bins(TAMCMC_MODEL_HARVEY_GAUSSIAN));
    int id, n;
    while (std::scanf("%d %d", &id, &n) == 2) {
        std::vector<double> p((size_t)n);
        for (int i = 0; i < n; i++)
            if (std::scanf("%la", &p[(size_t)i]) != 1) return 2;
        EnvRow R;
        env_row(id, p.data(), R);
        double r[TAMCMC_ENVELOPE_ROW_N];
        r[0] = R.amp; r[1] = R.numax; r[2] = R.sig2; r[3] = R.N0;
        for (int k = 0; k < 2; k++) { r[4 + k] = R.H[k]; r[6 + k] = R.lna[k]; r[8 + k] = R.pw[k]; r[22 + k] = R.hon[k] ? 1.0 : 0.0; }
        for (int k = 0; k < 3; k++) { r[10 + k] = R.b[k]; r[13 + k] = R.lnb[k]; r[16 + k] = R.c[k]; r[19 + k] = R.a2[k]; }
        std::printf("R");
        for (int f = 0; f < TAMCMC_ENVELOPE_ROW_N; f++) std::printf(" %a", r[f]);
        std::printf("\n");
    }
    return 0;
}
