"""The route rule of a gradient batch (tamcmc-c_amd/csrc/fd_route.h) with its trailing rgb_adjoint argument (TAMCMC_OPT_RGB_ADJOINT), on the
CPU: a small C++ driver of its own (tests/fd_route_rgb_driver.cpp, g++) prints what the header decides for the full product of its inputs,
the new flag and the Tables request included; the extended rule is restated here.  With the flag off every line is what the seven-argument
driver of tests/test_fd_route.py prints."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, ERR_BAD_MODEL, ERR_BAD_ARG = 0, -4, -5            # include/tamcmc_hip.h
STRICT, FAST, FAST_DIRECT = 0, 1, 2                   # TAMCMC_PRECISION_*
GRADIENT_FD, GRADIENT_ADJOINT = 0, 1                  # TAMCMC_GRADIENT_*
BRUTE, WINDOWED, ADJOINT, ROWS = 0, 1, 2, 3           # FdRoute, in the order of its declaration
FROM_OPTIONS, REQ_ADJOINT, REQ_ROWS, REQ_TABLES = 0, 1, 2, 3   # FdRequest

OLD = list(itertools.product((FROM_OPTIONS, REQ_ADJOINT, REQ_ROWS), (GRADIENT_FD, GRADIENT_ADJOINT), (0, 1), (STRICT, FAST, FAST_DIRECT),
                             (1, 0), (0, 3), (0, 1)))
CASES = list(itertools.product((FROM_OPTIONS, REQ_ADJOINT, REQ_ROWS, REQ_TABLES), (GRADIENT_FD, GRADIENT_ADJOINT), (0, 1),
                               (STRICT, FAST, FAST_DIRECT), (1, 0), (0, 3), (0, 1), (0, 1)))


def expected(request, gradient, fd_windowed, precision, delta_geometry, nvars, rgb, rgb_adjoint):
    """(code, route or None)."""
    if request == REQ_TABLES:                            # the batch's tables and nothing after them: the smallest layout, always
        return OK, BRUTE
    if request == REQ_ROWS:
        if rgb or precision == STRICT:
            return ERR_BAD_ARG, None
        return OK, ROWS
    if request == REQ_ADJOINT or gradient == GRADIENT_ADJOINT:
        if rgb and not rgb_adjoint:
            return ERR_BAD_MODEL, None
        if precision == STRICT:
            return ERR_BAD_ARG, None
        return OK, ADJOINT
    if fd_windowed and precision != STRICT and delta_geometry and nvars > 0:
        return OK, WINDOWED
    return OK, BRUTE


def _build(tmp, name):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", name + ".cpp")], check=True)
    return exe


def _lines(exe, cases):
    args = [str(v) for case in cases for v in case]
    return subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.split("\n")


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("route_rgb")
    return _build(tmp, "fd_route_rgb_driver"), _build(tmp, "fd_route_driver")


def test_extended_route_rule(drivers):
    new, _ = drivers
    assert len(CASES) == 768
    out = _lines(new, CASES)
    assert out[len(CASES)] == "routes %d %d %d %d requests %d %d %d %d" % (BRUTE, WINDOWED, ADJOINT, ROWS, FROM_OPTIONS, REQ_ADJOINT, REQ_ROWS,
                                                                            REQ_TABLES)
    seen = set()
    for case, line in zip(CASES, out):
        code, route = (int(v) for v in line.split())
        want = expected(*case)
        assert (code, route if code == OK else None) == want, (case, line)
        assert (code == OK) == (route >= 0)
        seen.add(want)
    assert seen == {(OK, BRUTE), (OK, WINDOWED), (OK, ADJOINT), (OK, ROWS), (ERR_BAD_ARG, None), (ERR_BAD_MODEL, None)}


def test_flag_off_is_the_seven_argument_rule(drivers):
    """The default argument: every line of the old driver, case for case."""
    new, old = drivers
    got = _lines(new, [case + (0,) for case in OLD])
    want = _lines(old, OLD)
    assert len(OLD) == 288 and got[:len(OLD)] == want[:len(OLD)]


def test_red_giants_with_the_flag_on(drivers):
    new, _ = drivers
    for request, gradient in ((FROM_OPTIONS, GRADIENT_ADJOINT), (REQ_ADJOINT, GRADIENT_FD), (REQ_ADJOINT, GRADIENT_ADJOINT)):
        for fd_windowed, delta_geometry, nvars in itertools.product((0, 1), (0, 1), (0, 3)):
            cases = [(request, gradient, fd_windowed, prec, delta_geometry, nvars, 1, 1) for prec in (FAST, FAST_DIRECT, STRICT)]
            out = _lines(new, cases)
            assert out[0] == out[1] == "%d %d" % (OK, ADJOINT), (cases[0], out[0])
            assert out[2] == "%d -1" % ERR_BAD_ARG, (cases[2], out[2])
    # the flag opens nothing else: the finite-difference routes of a red giant are what they were, REQ_ROWS is still refused
    for prec, fd_windowed in itertools.product((STRICT, FAST, FAST_DIRECT), (0, 1)):
        a, b = _lines(new, [(FROM_OPTIONS, GRADIENT_FD, fd_windowed, prec, 1, 3, 1, flag) for flag in (0, 1)])[:2]
        assert a == b
        for gradient, flag in itertools.product((GRADIENT_FD, GRADIENT_ADJOINT), (0, 1)):
            assert _lines(new, [(REQ_ROWS, gradient, fd_windowed, prec, 1, 3, 1, flag)])[0] == "%d -1" % ERR_BAD_ARG
