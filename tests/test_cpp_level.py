"""GPU: SPERR3D_OMP_D::decompress_level, the C++ mirror's decode of one level of the hierarchy
(include/sperr_hip.hpp), driven by tests/cpp/level_check.cpp: the level, or the box of it, is the oracle's
hierarchy cut to it, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from sperr_amd.synth import turbulence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sperr_amd import api
    path = tmp_path_factory.mktemp("level_check") / "level_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "level_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


@pytest.mark.parametrize("mode,q", [(1, 2.5), (3, 1e-3)])
def test_mirror_decompress_level(oracle, exe, tmp_path, mode, q):
    v = turbulence((64, 64, 96))
    stream = oracle.comp_3d(v, (32, 32, 32), mode, q)
    (tmp_path / "c.sperr").write_bytes(stream)
    levels = oracle.decomp_3d_multi_res(stream)[1]
    assert len(levels) > 0
    out = tmp_path / "level.f64"
    for h, lv in enumerate(levels):
        r = lv.shape[0] // 2   # a chunk's corner at this level (2 chunks along z)
        lz, ly, lx = lv.shape
        for box in (None, ((r - 1, 0, r - 1), (min(3, lx - r + 1), ly, 2)), ((lx - 1, ly - 1, lz - 1), (1, 1, 1))):
            args = [str(h)] + ([str(x) for x in box[0] + box[1]] if box else [])
            p = subprocess.run([str(exe), str(tmp_path / "c.sperr"), *args, str(out)], capture_output=True, text=True,
                               timeout=600)
            assert p.returncode == 0, p.stdout + p.stderr
            want = lv
            if box:
                lo, dims = box
                want = np.ascontiguousarray(lv[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]])
            got = np.fromfile(out, dtype=np.float64).reshape(want.shape)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (h, box)
