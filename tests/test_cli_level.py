"""sperr3d -d --level H: --decomp_f / --decomp_d hold level H of the lower resolutions alone; with --box_origin /
--box_dims, the box of it in that level's coordinates.

CPU: the option's dependencies.  GPU (-m gpu): the files equal the files of the same level that
--decomp_lowres_d / --decomp_lowres_f write, and the box form equals the numpy crop of the oracle's level."""
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


def test_help_lists_the_level_option(tools):
    rc, out = run(tools, "--help")
    assert rc == 0 and "--level" in out


@pytest.mark.parametrize("args,message", [
    (("s", "-c", "--level", 0), "requires -d"),
    (("s", "--level", 0, "--decomp_f", "o"), "requires -d"),
    (("s", "-d", "--level", 0, "--decomp_lowres_f", "o"), "excludes"),
    (("s", "-d", "--level", 0, "--decomp_lowres_d", "o"), "excludes"),
    (("s", "-d", "--level", 0, "--decomp_d", "o", "--decomp_lowres_d", "p"), "excludes"),
    (("s", "-d", "--level", "--decomp_f", "o"), "Could not convert"),
    (("s", "-d", "--level", 0, "--decomp_f", "o", "--box_dims", 1, 1, 1), "requires --box_origin"),
    (("s", "-d", "--level", 0, "--decomp_lowres_f", "o", "--box_origin", 0, 0, 0, "--box_dims", 1, 1, 1), "excludes"),
])
def test_level_option_checks(tools, args, message):
    rc, out = run(tools, *args)
    assert rc != 0 and message in out


@pytest.mark.gpu
def test_level_files_are_the_lowres_files(tools, oracle, tmp_path):
    v = turbulence((64, 64, 96))
    stream = oracle.comp_3d(v, (32, 32, 32), 1, 3.0)
    src = tmp_path / "c.sperr"
    src.write_bytes(stream)
    levels = oracle.decomp_3d_multi_res(stream)[1]
    assert len(levels) > 0
    rc, out = run(tools, src, "-d", "--decomp_lowres_d", tmp_path / "low.f64", "--decomp_lowres_f", tmp_path / "low.f32")
    assert rc == 0, out
    for h, lv in enumerate(levels):
        tag = "." + "x".join(str(d) for d in reversed(lv.shape))
        f32, f64 = tmp_path / "lev.f32", tmp_path / "lev.f64"
        rc, out = run(tools, src, "-d", "--level", h, "--decomp_f", f32, "--decomp_d", f64)
        assert rc == 0, out
        assert f64.read_bytes() == (tmp_path / ("low.f64" + tag)).read_bytes() == lv.tobytes()
        assert f32.read_bytes() == (tmp_path / ("low.f32" + tag)).read_bytes()
        # the box form, in the level's coordinates: across the corner of the first chunk
        lz, ly, lx = lv.shape
        r = lx // 3
        lo, dims = (r - 1, ly - 1, 0), (min(3, lx - r + 1), 1, lz)
        rc, out = run(tools, src, "-d", "--level", h, "--box_origin", *lo, "--box_dims", *dims, "--decomp_f", f32,
                      "--decomp_d", f64)
        assert rc == 0, out
        cut = np.ascontiguousarray(lv[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]])
        assert f64.read_bytes() == cut.tobytes()
        assert f32.read_bytes() == cut.astype(np.float32).tobytes()
    # a level the container does not have, and a box that leaves the level
    rc, out = run(tools, src, "-d", "--level", len(levels), "--decomp_f", tmp_path / "x.f32")
    assert rc != 0 and "Decompression failed!" in out
    lx = levels[0].shape[2]
    rc, out = run(tools, src, "-d", "--level", 0, "--box_origin", lx - 1, 0, 0, "--box_dims", 2, 1, 1, "--decomp_f",
                  tmp_path / "x.f32")
    assert rc != 0 and "Decompression failed!" in out
