"""CPU: sperr_amd/csrc/rel.h -- the rule of point-wise relative error: the tolerance with its floor and refusals, the
forward map, the inverse, the side stream with every refusal of its header -- checked by tests/cpp/rel_check.cpp, a
program of its own built with the address and undefined sanitizers and run directly.  The header is plain C++, so the
host compiler builds it.  The program's y, side stream and inverse of the adversarial samples are compared bit for bit
with tests/rel_model.py, the numpy statement of the same rule."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rel_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("rel_check") / "rel_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "rel_check.cpp"), "-o", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def run(exe, *args):
    r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_rel_rule_streams_and_refusals_under_sanitizers(exe):
    r = run(exe)
    assert r.returncode == 0 and "rel_check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def samples(dtype, n):
    """n samples: the adversarial ones, then values over many decades with both signs and runs of zeros"""
    adv = R.adversarial(dtype)
    rng = np.random.default_rng(n)
    lo, hi = (-140.0, 120.0) if dtype == np.float32 else (-1000.0, 1000.0)
    v = (np.exp2(rng.uniform(lo, hi, n)) * rng.choice([-1.0, 1.0], n)).astype(dtype)
    v[(np.arange(n) // 37) % 5 == 2] = 0
    k = min(n, adv.size)
    v[:k] = adv[:k]
    return v


@pytest.mark.parametrize("n", [4913, 1024, 1025])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_forward_stream_and_inverse_of_the_program_are_the_models(exe, tmp_path, dtype, n):
    x = samples(dtype, n)
    tag = "f32" if dtype == np.float32 else "f64"
    eps = 1e-2
    y, zero, neg = R.forward(x)
    x.tofile(tmp_path / "x.bin")
    r = run(exe, "forward", tag, float(eps).hex(), tmp_path / "x.bin", tmp_path / "y.bin", tmp_path / "side.bin")
    assert r.returncode == 0, r.stdout + r.stderr
    got_y = np.fromfile(tmp_path / "y.bin", dtype=np.float64)
    assert np.array_equal(got_y.view(np.uint64), y.view(np.uint64))
    side = (tmp_path / "side.bin").read_bytes()
    assert side == R.side_stream(zero, neg, eps, dtype == np.float32) and len(side) <= R.max_size(n)
    isf, e, nn, z2, n2 = R.parse(side)
    assert (isf, e, nn) == (int(dtype == np.float32), eps, n) and np.array_equal(z2, zero) and np.array_equal(n2, neg)
    # the inverse of y itself and of y moved by +-t, and of values that need the clamp
    t = R.tolerance(eps, dtype == np.float32)
    rng = np.random.default_rng(5)
    for k, yp in enumerate((y, y + t, y - t, y + rng.uniform(-3000.0, 3000.0, n))):
        yp.tofile(tmp_path / "yp.bin")
        for out_tag, odt in (("f32", np.float32), ("f64", np.float64)):
            r = run(exe, "inverse", out_tag, tmp_path / "yp.bin", tmp_path / "side.bin", tmp_path / "out.bin")
            assert r.returncode == 0, r.stdout + r.stderr
            got = np.fromfile(tmp_path / "out.bin", dtype=odt)
            want = R.inverse(yp, zero, neg, odt == np.float32, dtype == np.float32)
            u = np.uint32 if odt == np.float32 else np.uint64
            assert np.array_equal(got.view(u), want.view(u)), (k, out_tag)
            assert np.isfinite(got).all()
            if k == 0 and odt == dtype:   # (y is exact for floats; doubles come back within the rounding of y)
                assert (got[zero] == 0).all() and np.array_equal(np.signbit(got), np.signbit(x))   # (double subnormals too)
                if dtype == np.float32:
                    nz = ~zero
                    assert np.array_equal(got[nz].view(u), x[nz].view(u))


def test_a_sample_that_is_not_finite_refuses_the_volume(exe, tmp_path):
    for bad in (np.inf, -np.inf, np.nan):
        x = np.array([1.0, 2.0, bad, 4.0], dtype=np.float32)
        assert R.forward(x) is None
        x.tofile(tmp_path / "x.bin")
        r = run(exe, "forward", "f32", float(1e-2).hex(), tmp_path / "x.bin", tmp_path / "y.bin", tmp_path / "s.bin")
        assert r.returncode == 3 and "refused" in r.stdout


@pytest.mark.parametrize("is_float", [True, False], ids=["f32", "f64"])
def test_tolerance_floor_and_refusals_of_the_program_are_the_models(exe, is_float):
    floor = R.tolerance_floor(is_float)
    s = R.slack(is_float)
    below = float(np.nextafter(np.float64(floor), np.float64(0.0)))
    assert R.tolerance(floor, is_float) >= s and R.tolerance(below, is_float) is None
    # the floor is the boundary eps of the precision: a hair over 2 s
    assert 2.0 * s < floor < 2.0 * s * (1.0 + 8.0 * s)
    for eps in (floor, below, 1e-4, 1e-2, 0.5, float(np.nextafter(0.5, 1.0)), 0.0, -1e-2, -1.0, np.inf, np.nan, 2.0 * s):
        want = R.tolerance(eps, is_float)
        arg = "nan" if eps != eps else float(eps).hex()
        got = run(exe, "tolerance", arg, int(is_float)).stdout.strip()
        assert (got == "refused") == (want is None), (eps, got, want)
        assert want is None or float.fromhex(got) == want, (eps, got, want)
