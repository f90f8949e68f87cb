"""GPU (-m gpu): sperr3d -d --pct P decodes the first P percent of every chunk's stream; alone, with a box and with a
level the files are the oracle's results for the container sperr_trunc_3d makes, bit for bit.  (The option's checks
need no GPU: tests/test_portion_host.py.)"""
import os
import subprocess

import numpy as np
import pytest

from sperr_amd.synth import turbulence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tools():
    from sperr_amd import api
    if not os.path.exists(api.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sperr_amd", "csrc"), "-j4"])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cli")])
    return BIN


def run(tools, *args):
    p = subprocess.run([os.path.join(tools, "sperr3d")] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=600)
    return p.returncode, p.stdout + p.stderr


def test_pct_files_are_the_truncated_containers_decode(tools, oracle, tmp_path):
    v = turbulence((64, 64, 64))
    stream = oracle.comp_3d(v, (32, 32, 32), 1, 3.0)
    (tmp_path / "c.sperr").write_bytes(stream)
    cut = oracle.trunc_3d(stream, 40)
    want64, want32 = oracle.decomp_3d(cut, False), oracle.decomp_3d(cut, True)
    assert not np.array_equal(want32, oracle.decomp_3d(stream, True))
    level0 = oracle.decomp_3d_multi_res(cut)[1][0]
    assert not np.array_equal(level0, oracle.decomp_3d_multi_res(stream)[1][0])
    f32, f64 = tmp_path / "o.f32", tmp_path / "o.f64"

    def files(*args):
        rc, out = run(tools, tmp_path / "c.sperr", "-d", "--pct", 40, *args, "--decomp_f", f32, "--decomp_d", f64)
        assert rc == 0, out
        return np.fromfile(f64, dtype=np.float64).tobytes(), np.fromfile(f32, dtype=np.float32).tobytes()

    assert files() == (want64.tobytes(), want32.tobytes())
    lo, dims = (31, 5, 17), (20, 50, 33)
    box = (slice(lo[2], lo[2] + dims[2]), slice(lo[1], lo[1] + dims[1]), slice(lo[0], lo[0] + dims[0]))
    assert files("--box_origin", *lo, "--box_dims", *dims) == (np.ascontiguousarray(want64[box]).tobytes(),
                                                               np.ascontiguousarray(want32[box]).tobytes())
    assert files("--level", 0) == (level0.tobytes(), level0.astype(np.float32).tobytes())
    # --pct 100 and above: the whole streams
    rc, out = run(tools, tmp_path / "c.sperr", "-d", "--pct", 100, "--decomp_d", f64)
    assert rc == 0, out
    assert np.fromfile(f64, dtype=np.float64).tobytes() == oracle.decomp_3d(stream, False).tobytes()
    rc, out = run(tools, tmp_path / "c.sperr", "-d", "--pct", 40, "--box_origin", 60, 0, 0, "--box_dims", 5, 1, 1,
                  "--decomp_f", tmp_path / "x.f32")
    assert rc != 0 and "Decompression failed!" in out
