"""The fields of tamcmc_sampler_get_envelope_rows restated in long double: env_row's expressions (csrc/envelope_row.h, the scalar part of
model_Harvey_Gaussian / model_Kallinger2014_Gaussian) on one parameter vector.  Shared by tests/test_envelope_row.py (host build of the
row builder) and tests/test_gpu_envelope_device.py (the device engine's rows)."""
import numpy as np

FIELDS = ("amp", "numax", "sig2", "N0", "H0", "H1", "lna0", "lna1", "pw0", "pw1", "b0", "b1", "b2", "lnb0", "lnb1", "lnb2",
          "c0", "c1", "c2", "a2_0", "a2_1", "a2_2", "hon0", "hon1")


def row_reference(model_id, p):
    ld = np.longdouble
    p = np.asarray(p, dtype=ld)
    r = np.zeros(24, dtype=ld)
    with np.errstate(divide="ignore"):
        if model_id == 1:
            r[0], r[1], r[2], r[3] = abs(p[7]), p[8], abs(p[9]) ** 2, abs(p[6])
            for q in range(2):
                tc = abs(p[3 * q + 1])
                r[4 + q], r[6 + q], r[8 + q], r[22 + q] = abs(p[3 * q]), np.log(ld("1e-3") * tc), abs(p[3 * q + 2]), 1.0 if tc != 0 else 0.0
            return r
        numax, mu = abs(p[15]), p[17]
        r[0], r[1], r[2], r[3] = abs(p[14]), numax, abs(p[16]) ** 2, abs(p[13])
        a = (abs(p[0] * numax ** p[1]), p[5], p[6])
        b = (abs(p[2] * abs(numax + mu) ** p[3]), abs(p[7] * abs(numax + mu) ** p[8]), abs(p[10] * abs(numax + mu) ** p[11]))
        c = (abs(p[4]), abs(p[9]), abs(p[12]))
        for k in range(3):
            r[10 + k], r[13 + k], r[16 + k], r[19 + k] = b[k], np.log(b[k]), c[k], a[k] ** 2
    return r
