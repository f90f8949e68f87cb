"""sperr3d -d --box_origin X Y Z --box_dims NX NY NZ: --decomp_f / --decomp_d hold only that box.

CPU: the options' arities and dependencies.  GPU (-m gpu): the files are the oracle's whole decode cut to the
box, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from sperr_amd.synth import turbulence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")


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


def test_help_lists_the_box_options(tools):
    rc, out = run(tools, "--help")
    assert rc == 0 and "--box_origin" in out and "--box_dims" in out


@pytest.mark.parametrize("args,message", [
    (("s", "-d", "--decomp_f", "o", "--box_origin", 0, 0, 0), "requires --box_dims"),
    (("s", "-d", "--decomp_f", "o", "--box_dims", 1, 1, 1), "requires --box_origin"),
    (("s", "-c", "--box_origin", 0, 0, 0, "--box_dims", 1, 1, 1), "requires -d"),
    (("s", "-d", "--decomp_f", "o", "--box_origin", 0, 0, "--box_dims", 1, 1, 1), "Could not convert"),
    (("s", "-d", "--decomp_f", "o", "--box_dims", 1, 1), "3 required"),
    (("s", "-d", "--decomp_lowres_f", "o", "--box_origin", 0, 0, 0, "--box_dims", 1, 1, 1), "excludes"),
])
def test_box_option_checks(tools, args, message):
    rc, out = run(tools, *args)
    assert rc != 0 and message in out


@pytest.mark.gpu
def test_box_files_are_the_cropped_decode(tools, oracle, tmp_path):
    v = turbulence((50, 64, 72))
    stream = oracle.comp_3d(v, (32, 32, 32), 1, 3.0)
    (tmp_path / "c.sperr").write_bytes(stream)
    full64, full32 = oracle.decomp_3d(stream, False), oracle.decomp_3d(stream, True)
    for lo, dims in [((31, 5, 17), (40, 50, 20)), ((0, 0, 0), (72, 64, 50)), ((71, 0, 49), (1, 64, 1))]:
        f32, f64 = tmp_path / "box.f32", tmp_path / "box.f64"
        rc, out = run(tools, tmp_path / "c.sperr", "-d", "--box_origin", *lo, "--box_dims", *dims,
                      "--decomp_f", f32, "--decomp_d", f64)
        assert rc == 0, out
        cut = (slice(lo[2], lo[2] + dims[2]), slice(lo[1], lo[1] + dims[1]), slice(lo[0], lo[0] + dims[0]))
        assert np.fromfile(f64, dtype=np.float64).tobytes() == np.ascontiguousarray(full64[cut]).tobytes()
        assert np.fromfile(f32, dtype=np.float32).tobytes() == np.ascontiguousarray(full32[cut]).tobytes()
    rc, out = run(tools, tmp_path / "c.sperr", "-d", "--box_origin", 70, 0, 0, "--box_dims", 3, 1, 1,
                  "--decomp_f", tmp_path / "x.f32")
    assert rc != 0 and "Decompression failed!" in out
