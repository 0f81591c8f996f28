// Host driver of the red-giant scalar unpack (tamcmc-c_amd/csrc/rgb_unpack.h, unpack_vector<OneThread>): reads vectors from stdin and
// prints Prep and RowIn field by field, for tests/test_rgb_reference.py (stage (a) of tests/rgb_reference.py, no GPU).
// Input, whitespace separated, repeated until EOF:  model_id  step  Np  params[Np]  plength[11]
#include <cstdio>
#include <vector>

#include "../tamcmc-c_amd/csrc/rgb_unpack.h"

using namespace tamcmc;

static void arr(const char *name, const double *v, int n) {
    std::printf("%s", name);
    for (int i = 0; i < n; i++) std::printf(" %.17g", v[i]);
    std::printf("\n");
}

int main() {
    int model_id, Np;
    double step;
    while (std::scanf("%d %lf %d", &model_id, &step, &Np) == 3) {
        std::vector<double> p((size_t)Np);
        int32_t pl[11];
        for (int i = 0; i < Np; i++)
            if (std::scanf("%lf", &p[(size_t)i]) != 1) return 2;
        for (int i = 0; i < 11; i++)
            if (std::scanf("%d", &pl[i]) != 1) return 2;
        static rgb::Prep P;
        static rgb::RowIn R;
        std::vector<double> noise((size_t)(pl[8] > 0 ? pl[8] : 1), 0.0);
        int32_t nh = -1, nn = -1;
        double fmin = 0;
        const int st = rgb::unpack_vector(rgb::OneThread(), p.data(), pl, step, model_id == 27, 0, P, R, noise.data(), &nh, &nn, &fmin);
        std::printf("status %d\nnh %d\nnn %d\n", st, nh, nn);
        arr("noise", noise.data(), nn > 0 ? nn : 0);
        if (st == 0) {
            std::printf("Lp %d\nLg %d\nng_min %d\n", P.Lp, P.Lg, P.ng_min);
            const double sc[8] = {P.Dnu_p, P.DPl, P.alpha, P.q, P.zone, P.resol, P.fact, 0};
            arr("prep", sc, 7);
            arr("keep", &P.keep_lo, 1);
            arr("keep_hi", &P.keep_hi, 1);
            arr("nu_p", P.nu_p, P.Lp);
            arr("dnu_loc", P.dnu_loc, P.Lp);
            arr("dnup", P.dnup, P.Lp);
            std::printf("ig0");
            for (int i = 0; i < P.Lp; i++) std::printf(" %d", P.ig0[i]);
            std::printf("\n");
            std::printf("rowin %d %d %d %d %d %d %d\n", R.Nfl0, R.Nfl2, R.Nfl3, R.lmax, R.do_amp, R.bias_n, R.cte_width);
            arr("Wl0", R.Wl0, R.Nfl0);
            arr("Hl0", R.Hl0, R.Nfl0);
            arr("Vl", R.Vl, 4);
            for (int l = 0; l < 4; l++) arr("V", R.V[l], 7);
            const double sr[6] = {R.eta0, R.Hfactor, R.Wfactor, R.rot_env, R.rot_core, R.trunc_c};
            arr("scal", sr, 6);
            arr("sb", R.sb, R.bias_n);
            arr("sc", R.sc, R.bias_n);
            arr("sd", R.sd, R.bias_n);
            arr("sc0", &R.sc0, 1);
        }
        std::printf("end\n");
    }
    return 0;
}
