"""GPU: the fill overloads of the C++ header (include/sperr_hip.hpp: mask_make_dev and compress_masked_dev with a
FillKind), driven by tests/cpp/mask_fill_api_check.cpp on a (30, 44, 37) volume with a ball of NaNs: the in-filled
volumes are the models' bit for bit, the mask is the model's, and the containers are the oracle's of the models'
in-filled volumes byte for byte.  The program itself checks the refusals and that FillKind::Midrange is the call
without a fill."""
import os
import subprocess

import numpy as np
import pytest

import mask_fill_model as F
import mask_model as M
from sperr_amd.synth import turbulence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sperr_amd import api
    path = tmp_path_factory.mktemp("mask_fill_api_check") / "mask_fill_api_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "mask_fill_api_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_cpp_fill_overloads(oracle, exe, tmp_path):
    shape = (30, 44, 37)
    v = turbulence(shape, dtype=np.float64).astype(np.float32)
    mask = M.ball_mask(shape, 12)
    v[mask] = np.nan
    dz, dy, dx = shape
    v.tofile(tmp_path / "vol.f32")
    names = ["smooth.f32", "value.f32", "c_smooth.bin", "c_value.bin", "mask.bin"]
    p = subprocess.run([str(exe), str(tmp_path / "vol.f32"), str(dx), str(dy), str(dz)] +
                       [str(tmp_path / nm) for nm in names], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert (tmp_path / "mask.bin").read_bytes() == M.stream(mask)
    smooth, valued = F.smooth_filled(v, mask), F.value_filled(v, mask, 3.5)
    got = np.fromfile(tmp_path / "smooth.f32", dtype=np.float32).reshape(shape)
    assert np.array_equal(got.view(np.uint32), smooth.view(np.uint32))
    got = np.fromfile(tmp_path / "value.f32", dtype=np.float32).reshape(shape)
    assert np.array_equal(got.view(np.uint32), valued.view(np.uint32))
    assert (tmp_path / "c_smooth.bin").read_bytes() == oracle.comp_3d(smooth, (32, 32, 32), 1, 2.5)
    assert (tmp_path / "c_value.bin").read_bytes() == oracle.comp_3d(valued, (32, 32, 32), 1, 2.5)
