"""Input front end (csrc/host_io.cpp): the COMPLETE output of the three `.model` loaders -- every field of every successful load,
the code and text of every refusal -- on the four `.model` fixtures and six files derived from them by the text edits the other
loader tests use, against records under tests/golden/inputs_dump/.  The records were written by tests/inputs_dump_driver.cpp built
with the host_io.cpp that preceded the restatement of its three builders in shared pieces ("The input front end's
builders stated once"); that change was accepted on equal bytes over 18 294 variants of these files (`--variants`), most of them
malformed, and this test keeps the ten base files pinned.

Names, prior names, integers and refusal texts compare exactly; doubles at rtol = 1e-13, the tolerance of test_inputs_local.py for
this loader: pow, cos and sqrt may round differently under another libm."""
import os
import shutil
import subprocess

import pytest

from test_hnlm_models import _classic_dialect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RECORDS = os.path.join(GOLDEN, "inputs_dump")
RTOL = 1e-13
LOCAL, SUN, RGB, NOBIAS = ("TF_3443483_local-v3.model", "Sun_19992002_incfix_fast_Priorevalrange.model", "RGB_10722175.model",
                           "RGB_10722175_nobias.model")
DOUBLES_FROM = {"range": 1, "dnu": 1, "c_l": 1, "extra": 1, "p": 6}   # record line tag -> first field that is a double


def _one_column(lines):
    """RGB, one-column hyper priors (test_inputs_rgb.py)."""
    return [ln.split()[0] if ("Gaussian" in ln and ln.strip()[0].isdigit()) else ln for ln in lines]


def base_files(folder):
    """The ten base files: the four fixtures and six text edits of them, written into `folder`."""
    def derived(src, name, edit):
        lines = open(os.path.join(GOLDEN, src)).read().split("\n")
        path = os.path.join(str(folder), name)
        with open(path, "w") as f:
            f.write("\n".join(edit(lines)))
        return path
    classic = "model_MS_Global_a1etaa3_HarveyLike_Classic"
    return [os.path.join(GOLDEN, n) for n in (LOCAL, SUN, RGB, NOBIAS)] + [
        derived(LOCAL, "TF_3443483_local_Hnlm.model", lambda L: [ln.replace("model_MS_local_basic", "model_MS_local_Hnlm") if "model_fullname" in ln else ln for ln in L]),
        derived(RGB, "RGB_10722175_CteWidth.model", lambda L: [ln.replace("_aj_AppWidth_", "_aj_CteWidth_") if "model_fullname" in ln else ln for ln in L]),
        derived(RGB, "RGB_10722175_onecolumn.model", _one_column),
        derived(SUN, "Sun_Classic.model", lambda L: _classic_dialect(L, classic)),
        derived(SUN, "Sun_Classic_v2.model", lambda L: _classic_dialect(L, classic + "_v2")),
        derived(SUN, "Sun_Classic_v3.model", lambda L: _classic_dialect(L, classic + "_v3"))]


def build_driver(exe, *flags):
    src = os.path.join(ROOT, "tamcmc-c_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", *flags, "-o", exe, os.path.join(ROOT, "tests", "inputs_dump_driver.cpp"),
           os.path.join(src, "host_io.cpp"), os.path.join(src, "host_cfg.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)


def records(text):
    """{(file, loader): [lines of the record]} of the driver's output for un-varied files."""
    out, cur = {}, None
    for ln in text.split("\n"):
        if ln.startswith("== "):
            file, variant, loader = ln[3:].split(" | ")
            assert variant == "base"
            cur = out.setdefault((file, loader), [])
        elif ln:
            cur.append(ln)
    return out


def _same(got, want):
    if got == want:
        return True
    g, w = got.split("\t"), want.split("\t")
    k = DOUBLES_FROM.get(w[0])
    if k is None or len(g) != len(w) or g[:k] != w[:k]:
        return False
    return all(abs(float.fromhex(a) - float.fromhex(b)) <= RTOL * abs(float.fromhex(b)) for a, b in zip(g[k:], w[k:]))


@pytest.fixture(scope="module")
def needs_gxx():
    if shutil.which("g++") is None:
        pytest.skip("no g++")


def test_every_field_of_every_loader_on_the_base_files(needs_gxx, tmp_path):
    exe = str(tmp_path / "dump")
    build_driver(exe)
    r = subprocess.run([exe] + base_files(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = records(r.stdout)
    want = {}
    for name in sorted(os.listdir(RECORDS)):
        want.update(records(open(os.path.join(RECORDS, name)).read()))
    assert len(want) == 10 * 11 and sorted(got) == sorted(want)        # ten files x (nine slices, global, red-giant)
    loads = 0
    for key in sorted(want):
        g, w = got[key], want[key]
        assert len(g) == len(w), key
        for a, b in zip(g, w):
            assert _same(a, b), (key, a, b)
        loads += w[0] == "rc 0"
    assert loads == 23      # local, Hnlm: eight slices each; aj, Classic, Classic_v2; AppWidth, no-bias, CteWidth, one-column


def test_dump_driver_under_sanitizers(needs_gxx, tmp_path):
    """The same driver, stand-alone, with AddressSanitizer (leaks included) and UBSan over the base files."""
    exe = str(tmp_path / "dump_san")
    build_driver(exe, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")   # (no -g: it doubles the compile time)
    r = subprocess.run([exe] + base_files(tmp_path), capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-4000:]
    assert len(records(r.stdout)) == 110
