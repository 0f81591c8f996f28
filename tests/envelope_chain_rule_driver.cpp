// envelope_chain_rule_driver.cpp -- the chain rule of the Gaussian-envelope fits' analytic gradient through a plain C++ compiler:
// env_grad_rows, env_row_jacobian and env_chain_contract of csrc/envelope_row.h, one text for two arithmetics.
//   "d"  the DOUBLE instantiation, the arithmetic k_env_mala_chain (csrc/dev_mala_impl.h) runs them in (tests/test_envelope_device_chain_rule.py)
//   "l"  the LONG DOUBLE instantiation, the host's chain rule (envelope.hip: envelope_grad_unfold, envelope_chain_rule), replayed on the sums
//        and rows a device sampler hands out (tests/test_gpu_envelope_device_langevin.py)
// Per line of stdin "<d|l> <model id> <n> <n parameters> <h> <16 tile sums> <12 xi sums> <row>" (hex floats or decimals), <row> = 0: the
// row is env_row's of the parameters, as on the device; 1 followed by the 24 doubles of tamcmc_sampler_get_envelope_rows: that row.
// It prints three lines: "G" and the n components dS/dtheta_j, "M" and the n magnitudes sum_q |dS/drow_q J_qj|, "R" and the 13
// row-space values dS/d(row quantity); every value as two hex doubles, the value rounded to double and the rest.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/tamcmc_hip.h"
#include "../include/tamcmc_sampler.h"
#include "../tamcmc-c_amd/csrc/envelope_row.h"

using namespace tamcmc;

template <class T>
static void put(T v) {
    const double hi = (double)v;
    const double lo = std::isfinite(hi) ? (double)(v - (T)hi) : 0.0;
    std::printf(" %a %a", hi, lo);
}

template <class T>
static void run(int id, int n, const double *p, const EnvRow &R, double h, const double *raw, const double *kraw) {
    T dS[ENV_GRAD_N];
    std::vector<T> J((size_t)ENV_GRAD_N * n);
    env_grad_rows<T>(id, R, h, raw, kraw, dS, nullptr);
    env_row_jacobian<T>(id, p, J.data());
    std::printf("G");
    for (int j = 0; j < n; j++) put(env_chain_contract<T>(dS, J.data(), n, j));
    std::printf("\nM");
    for (int j = 0; j < n; j++) {
        T m = 0;
        for (int q = 0; q < ENV_GRAD_N; q++)
            if (J[(size_t)q * n + j] != T(0)) m += std::fabs(dS[q] * J[(size_t)q * n + j]);
        put(m);
    }
    std::printf("\nR");
    for (T v : dS) put(v);
    std::printf("\n");
}

int main() {
    static_assert(TAMCMC_ENVELOPE_ROW_N == 24, "the audit entry's row");
    char mode[4];
    int id, n;
    while (std::scanf("%3s %d %d", mode, &id, &n) == 3) {
        if (n != (id == TAMCMC_MODEL_KALLINGER2014_GAUSSIAN ? 19 : 10)) return 3;
        std::vector<double> p((size_t)n);
        double h, raw[ENV_GRAD_NRAWMAX], kraw[ENV_GRAD_NKRAW], r[TAMCMC_ENVELOPE_ROW_N];
        int given;
        for (int i = 0; i < n; i++)
            if (std::scanf("%la", &p[(size_t)i]) != 1) return 2;
        if (std::scanf("%la", &h) != 1) return 2;
        for (double &v : raw)
            if (std::scanf("%la", &v) != 1) return 2;
        for (double &v : kraw)
            if (std::scanf("%la", &v) != 1) return 2;
        if (std::scanf("%d", &given) != 1) return 2;
        EnvRow R;
        env_row(id, p.data(), R);
        if (given) {  // env_row_as_doubles, backwards
            for (double &v : r)
                if (std::scanf("%la", &v) != 1) return 2;
            R.amp = r[0]; R.numax = r[1]; R.sig2 = r[2]; R.N0 = r[3];
            for (int k = 0; k < 2; k++) { R.H[k] = r[4 + k]; R.lna[k] = r[6 + k]; R.pw[k] = r[8 + k]; R.hon[k] = r[22 + k] != 0.0 ? 1 : 0; }
            for (int k = 0; k < 3; k++) { R.b[k] = r[10 + k]; R.lnb[k] = r[13 + k]; R.c[k] = r[16 + k]; R.a2[k] = r[19 + k]; }
        }
        if (mode[0] == 'd') run<double>(id, n, p.data(), R, h, raw, kraw);
        else if (mode[0] == 'l') run<long double>(id, n, p.data(), R, h, raw, kraw);
        else return 4;
    }
    return 0;
}
