"""GPU: SPERR3D_OMP_D::decompress_box, the C++ mirror's sub-box decode (include/sperr_hip.hpp), driven by
tests/cpp/box_check.cpp: the box is the oracle's whole decode cut to it, bit for bit."""
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
    path = tmp_path_factory.mktemp("box_check") / "box_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "box_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


@pytest.mark.parametrize("mode,q,lo,dims", [(1, 2.5, (31, 5, 17), (40, 50, 20)),
                                            (3, 1e-3, (0, 0, 0), (72, 64, 50)),
                                            (1, 2.5, (71, 63, 49), (1, 1, 1))])
def test_mirror_decompress_box(oracle, exe, tmp_path, mode, q, lo, dims):
    v = turbulence((50, 64, 72))
    stream = oracle.comp_3d(v, (32, 32, 32), mode, q)
    (tmp_path / "c.sperr").write_bytes(stream)
    out = tmp_path / "box.f64"
    p = subprocess.run([str(exe), str(tmp_path / "c.sperr"), *map(str, lo), *map(str, dims), str(out)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    full = oracle.decomp_3d(stream, False)
    want = np.ascontiguousarray(full[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]])
    got = np.fromfile(out, dtype=np.float64).reshape(want.shape)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
