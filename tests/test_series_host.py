"""CPU: sperr_amd/csrc/series.h compiled as host C++ -- a program of its own, tests/cpp/series_check.cpp, under
-fsanitize=address,undefined -- against tests/series_model.py on shared inputs: the plan, the needs, the tolerances, the
two butterflies and the info record, bit pattern by bit pattern."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import series_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("series_check") / "series_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "series_check.cpp"), "-o", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def run(exe, *args):
    r = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "FAILED" not in r.stdout, \
        r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def bits_of(v):
    return int(np.float64(v).view(np.uint64))


def test_checks_of_its_own(exe):
    assert "series_check ok" in run(exe)


@pytest.mark.parametrize("levels", range(5))
def test_plan_and_needs(exe, levels):
    for n in (1, 2, 3, 5, 8, 11, 16, 21, 40):
        got = [tuple(int(v) for v in line.split()) for line in run(exe, "plan", n, levels).split("\n") if line]
        assert got == sm.plan(n, levels), (n, levels)
    n = 11
    lines = [line for line in run(exe, "needs", n, levels).split("\n") if line]
    want = []
    for t0 in range(n):
        for nt in range(1, n - t0 + 1):
            need = set(sm.needs(n, levels, t0, nt))
            want.append("".join("1" if b in need else "0" for b in range(n)))
    assert lines == want


@pytest.mark.parametrize("levels", range(5))
def test_tolerances(exe, levels):
    for tol, M in ((1e-4, 1.0), (3.7e-9, 812.25), (1e-3 * 1.7e38, 3.4e38), (10.0, 1.0), (1e-15, 1.0), (2e-16, 1.0),
                   (1e-3, 0.0)):
        got = run(exe, "tol", bits_of(tol), bits_of(M), levels).split()
        want = sm.tolerance(tol, M, levels)
        if want is None:
            assert got == ["refused"], (tol, M, levels)
        else:
            assert got == ["ok", str(bits_of(want[0]))] + [str(bits_of(t)) for t in want[1]], (tol, M, levels)


@pytest.mark.parametrize("l", [1, 2, 3, 4])
def test_butterflies(exe, tmp_path, l):
    g = 1 << l
    rng = np.random.default_rng(l)
    m = 513
    x = rng.standard_normal((g, m)) * 10.0 ** rng.uniform(-30, 30, (1, m))
    x[:, :8] = np.float32(3.4028235e38) * rng.choice((-1.0, 1.0), (g, 8))      # fp32 extremes, widened
    x[:, 8:16] = rng.standard_normal((g, 8)).astype(np.float32)
    x[:, 16] = 0.0
    x[:, 17] = 1.0
    x.tofile(tmp_path / "in.f64")
    run(exe, "butterfly", l, tmp_path / "in.f64", tmp_path / "out.f64")
    out = np.fromfile(tmp_path / "out.f64", dtype=np.float64).reshape(2, g, m)
    fwd = sm.forward_group(x)
    assert np.array_equal(out[0].view(np.uint64), fwd.view(np.uint64))
    assert np.array_equal(out[1].view(np.uint64), sm.inverse_group(fwd).view(np.uint64))


def test_info_record(exe):
    args = (11, 3, 20, 18, 16, 1, 0, 1e-4, 2.0, 1.5, 7e-15)
    out = run(exe, "info", *args[:7], *[bits_of(v) for v in args[7:]]).split()
    want = sm.write_info(11, 3, (20, 18, 16), True, 0, 1e-4, 2.0, 1.5, 7e-15)
    assert out == [want.hex(), "1"]
