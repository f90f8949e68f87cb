"""CPU: the LOG map kind of sperr_amd/csrc/rel.h -- rel_log2 and rel_exp2, this kind's tolerance with its floor and
refusals, the forward map, the inverse, the side stream "SPLG" with every refusal of its header -- checked by
tests/cpp/rel_log_check.cpp, a program of its own built with the address and undefined sanitizers and -ffp-contract=off
and run directly.  The program's y, side stream and inverse are compared bit for bit with tests/rel_log_model.py, the
numpy statement of the same sequence of IEEE operations."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rel_log_model as L
import rel_model as R
from test_rel_host import run, samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("rel_log_check") / "rel_log_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "rel_log_check.cpp"), "-o", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def test_log_kind_rule_streams_and_refusals_under_sanitizers(exe):
    r = run(exe)
    assert r.returncode == 0 and "rel_log_check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("n", [4913, 1024, 1025])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_forward_stream_and_inverse_of_the_program_are_the_models(exe, tmp_path, dtype, n):
    x = samples(dtype, n)
    is_float = dtype == np.float32
    tag = "f32" if is_float else "f64"
    eps = 1e-2
    y, zero, neg = L.forward(x)
    x.tofile(tmp_path / "x.bin")
    r = run(exe, "forward", tag, float(eps).hex(), tmp_path / "x.bin", tmp_path / "y.bin", tmp_path / "side.bin")
    assert r.returncode == 0, r.stdout + r.stderr
    got_y = np.fromfile(tmp_path / "y.bin", dtype=np.float64)
    assert np.array_equal(got_y.view(np.uint64), y.view(np.uint64))
    side = (tmp_path / "side.bin").read_bytes()
    assert side == L.side_stream(zero, neg, eps, is_float) and len(side) <= R.max_size(n)
    isf, e, nn, z2, n2 = L.parse(side)
    assert (isf, e, nn) == (int(is_float), eps, n) and np.array_equal(z2, zero) and np.array_equal(n2, neg)
    # the inverse of y itself and of y moved by +-t, and of values that need the clamp
    t = L.tolerance(eps, is_float)
    rng = np.random.default_rng(5)
    for k, yp in enumerate((y, y + t, y - t, y + rng.uniform(-3000.0, 3000.0, n))):
        yp.tofile(tmp_path / "yp.bin")
        for out_tag, odt in (("f32", np.float32), ("f64", np.float64)):
            r = run(exe, "inverse", out_tag, tmp_path / "yp.bin", tmp_path / "side.bin", tmp_path / "out.bin")
            assert r.returncode == 0, r.stdout + r.stderr
            got = np.fromfile(tmp_path / "out.bin", dtype=odt)
            want = L.inverse(yp, zero, neg, odt == np.float32, is_float)
            u = np.uint32 if odt == np.float32 else np.uint64
            assert np.array_equal(got.view(u), want.view(u)), (k, out_tag)
            assert np.isfinite(got).all()
            if k == 0 and odt == dtype:
                assert (got[zero] == 0).all() and np.array_equal(np.signbit(got), np.signbit(x))
                if is_float:   # every float comes back
                    nz = ~zero
                    assert np.array_equal(got[nz].view(u), x[nz].view(u))
    # the same y' under the linear kind's stream is the linear kind's inverse: the kind is the stream's
    (tmp_path / "lin.bin").write_bytes(R.side_stream(zero, neg, eps, is_float))
    r = run(exe, "inverse", "f64", tmp_path / "yp.bin", tmp_path / "lin.bin", tmp_path / "out.bin")
    assert r.returncode == 0
    want = R.inverse(yp, zero, neg, False, is_float)
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", dtype=np.float64).view(np.uint64), want.view(np.uint64))


def test_a_sample_that_is_not_finite_refuses_the_volume(exe, tmp_path):
    for bad in (np.inf, -np.inf, np.nan):
        x = np.array([1.0, 2.0, bad, 4.0], dtype=np.float32)
        assert L.forward(x) is None
        x.tofile(tmp_path / "x.bin")
        r = run(exe, "forward", "f32", float(1e-2).hex(), tmp_path / "x.bin", tmp_path / "y.bin", tmp_path / "s.bin")
        assert r.returncode == 3 and "refused" in r.stdout


@pytest.mark.parametrize("is_float", [True, False], ids=["f32", "f64"])
def test_tolerance_floor_and_refusals_of_the_program_are_the_models(exe, is_float):
    floor = L.tolerance_floor(is_float)
    s = R.slack(is_float)
    below = float(np.nextafter(np.float64(floor), np.float64(0.0)))
    assert L.tolerance(floor, is_float) >= s and L.tolerance(below, is_float) is None
    rng = np.random.default_rng(17)
    swept = list(np.exp(rng.uniform(np.log(floor), np.log(0.5), 60)))
    for eps in [floor, below, 1e-4, 1e-2, 0.5, float(np.nextafter(0.5, 1.0)), 0.0, -1e-2, -1.0, -2.0, np.inf, np.nan,
                2.0 * s, R.tolerance_floor(is_float)] + swept:
        want = L.tolerance(eps, is_float)
        arg = "nan" if eps != eps else float(eps).hex()
        got = run(exe, "tolerance", arg, int(is_float)).stdout.strip()
        assert (got == "refused") == (want is None), (eps, got, want)
        assert want is None or float.fromhex(got) == want, (eps, got, want)

