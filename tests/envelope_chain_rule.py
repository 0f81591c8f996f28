"""tests/envelope_chain_rule_driver.cpp from Python: the chain rule of the Gaussian-envelope fits' analytic gradient (env_grad_rows,
env_row_jacobian, env_chain_contract of csrc/envelope_row.h) compiled with g++ in double ("d", the device's arithmetic) or long double
("l", the host's), on folded sums and -- optionally -- rows that the caller supplies."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def build(directory):
    exe = os.path.join(str(directory), "chain_rule_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "envelope_chain_rule_driver.cpp")], check=True, capture_output=True, timeout=300)
    return exe


def _word(w):
    return float.fromhex(w) if "0x" in w else float(w)


def _values(line, tag):
    words = line.split()
    assert words[0] == tag, line
    v = [_word(w) for w in words[1:]]
    return np.array([LD(hi) + LD(lo) for hi, lo in zip(v[0::2], v[1::2])], dtype=LD)


def run(exe, mode, model_id, P, h, raw, kraw, rows=None):
    """Per vector of P [C x Np]: (dS/dtheta [C x Np], sum_q |dS/drow_q J_qj| [C x Np], dS/d(row quantity) [C x 13]) as long doubles.
    h: x(1) - x(0); raw [C x 16], kraw [C x 12]: the folded sums; rows [C x 24] or None (None: env_row of the vector)."""
    text = ""
    for c, p in enumerate(P):
        words = [float(v).hex() for v in list(p) + [h] + list(raw[c]) + list(kraw[c])]
        words.append("0" if rows is None else "1 " + " ".join(float(v).hex() for v in rows[c]))
        text += "%s %d %d %s\n" % (mode, model_id, len(p), " ".join(words))
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(out) == 3 * len(P)
    G = np.array([_values(line, "G") for line in out[0::3]])
    M = np.array([_values(line, "M") for line in out[1::3]])
    R = np.array([_values(line, "R") for line in out[2::3]])
    return G, M, R
