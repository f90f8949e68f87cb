"""CPU: sperr_amd/csrc/psnr_vol.h compiled as host C++ -- a program of its own, tests/cpp/psnr_vol_check.cpp, under
-fsanitize=address,undefined -- against tests/psnr_vol_model.py: the table, every rung's estimate, the pick and the width
rule, bit pattern by bit pattern, on the ladder inputs (every rung 0 to 4 is where one of them stops) and on two chunks of
the fp64 plume at 225 dB (one needs 64-bit coefficients, one does not) and at 400 dB (refused)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import psnr_vol_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("psnr_vol_check") / "psnr_vol_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "psnr_vol_check.cpp"), "-o", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def bits_of(v):
    return int(np.float64(v).view(np.uint64))


def test_parts_of_the_header(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "psnr_vol_check ok" in r.stdout and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-3000:]


def header_says(exe, tmp_path, w, rng, psnr):
    np.ascontiguousarray(w, dtype=np.float64).tofile(tmp_path / "coeffs.f64")
    r = subprocess.run([str(exe), str(tmp_path / "coeffs.f64"), str(bits_of(rng)), repr(float(psnr))], capture_output=True,
                       text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    lad, mse, pick = (line.split() for line in r.stdout.strip().split("\n"))
    assert lad[0] == "ladder" and mse[0] == "mse" and pick[0] == "pick"
    return {"ok": int(lad[1]), "t": int(lad[3]), "q": [int(v) for v in lad[5:10]], "mse": [int(v) for v in mse[1:6]],
            "pick": int(pick[1]), "width": int(pick[3]), "maxabs": int(pick[5])}


def compare(got, w, rng, psnr):
    t, qs = pm.ladder(rng, psnr)
    assert got["ok"] == 1 and got["t"] == bits_of(t) and got["q"] == [bits_of(q) for q in qs]
    k, _ = pm.pick(w, t, qs)
    assert got["pick"] == (-1 if k is None else k)
    for r in range(pm.RUNGS if k is None else k + 1):
        assert got["mse"][r] == bits_of(pm.estimate(w, qs[r])), r
    maxabs = float(np.abs(w).max())
    assert got["maxabs"] == bits_of(maxabs)
    want = None if k is None else pm.width(maxabs, qs[k])
    assert got["width"] == {None: -1, 4: 0, 8: 1}[want]
    return k, want


@pytest.mark.parametrize("rung,inv_q0", list(enumerate(pm.LADDER_INV_Q0)))
@pytest.mark.parametrize("shape", sorted(pm.LADDER_SHAPES))
def test_header_on_the_ladder_inputs(exe, oracle, tmp_path, shape, rung, inv_q0):
    v, _, _ = oracle.condition(pm.ladder_chunk(oracle, pm.LADDER_SHAPES[shape]))
    w = oracle.dwt3d(v)
    rng = pm.range_for(inv_q0, pm.LADDER_PSNR)
    k, width = compare(header_says(exe, tmp_path, w, rng, pm.LADDER_PSNR), w, rng, pm.LADDER_PSNR)
    assert k == rung and width == 4


@pytest.mark.parametrize("psnr", [225.0, 400.0])
def test_header_on_the_plume_at_extreme_targets(exe, oracle, tmp_path, psnr):
    from test_gpu_size import plume
    vol = plume(np.float64)
    rng = pm.value_range(vol)
    widths = []
    for ck in (vol[:32, :32, :32], vol[:32, :32, 32:]):
        v, _, _ = oracle.condition(np.ascontiguousarray(ck))
        w = oracle.dwt3d(v)
        widths.append(compare(header_says(exe, tmp_path, w, rng, psnr), w, rng, psnr)[1])
    print(psnr, widths)
    assert widths == ([8, 4] if psnr == 225.0 else [None, None])
