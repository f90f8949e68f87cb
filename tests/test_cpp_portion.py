"""GPU: the portion methods of the C++ mirror (include/sperr_hip.hpp) -- SPERR3D_OMP_D::decompress_portion, the trailing
pct of decompress_box and decompress_level, SPERR3D_Stream_Tools::progressive_truncate_dev -- driven by
tests/cpp/portion_check.cpp: what they give is the oracle's truncation and the oracle's decode of it, bit for bit."""
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
    path = tmp_path_factory.mktemp("portion_check") / "portion_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "portion_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


@pytest.mark.parametrize("mode,q,pct", [(1, 4.0, 37), (3, 1e-3, 60)])
def test_mirror_portion_methods(oracle, exe, tmp_path, mode, q, pct):
    v = turbulence((64, 64, 64))
    stream = oracle.comp_3d(v, (32, 32, 32), mode, q)
    (tmp_path / "c.sperr").write_bytes(stream)
    p = subprocess.run([str(exe), str(tmp_path / "c.sperr"), str(pct), str(tmp_path / "out")], capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    cut = oracle.trunc_3d(stream, pct)
    want = oracle.decomp_3d(cut, False)
    assert not np.array_equal(want, oracle.decomp_3d(stream, False))
    assert (tmp_path / "out.trunc").read_bytes() == cut
    assert np.fromfile(tmp_path / "out.whole.f64", dtype=np.float64).tobytes() == want.tobytes()
    box = np.ascontiguousarray(want[9:9 + 21, 7:7 + 30, 5:5 + 40])
    assert np.fromfile(tmp_path / "out.box.f64", dtype=np.float64).tobytes() == box.tobytes()
    level0 = oracle.decomp_3d_multi_res(cut)[1][0]
    assert np.fromfile(tmp_path / "out.level.f64", dtype=np.float64).tobytes() == level0.tobytes()
