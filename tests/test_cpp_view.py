"""GPU: the view calls of the C++ header (include/sperr_hip.hpp: decompress_view_dev, quality_view_dev), driven by
tests/cpp/view_api_check.cpp on device arrays with ghost cells: the decoded interior is the Python decode bit for bit
with the halo untouched, and the figures are those of SperrHip.quality on the packed arrays."""
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
    path = tmp_path_factory.mktemp("view_api_check") / "view_api_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "view_api_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


@pytest.mark.parametrize("mode,q", [(1, 2.5), (3, 1e-3)])
def test_cpp_view_decode_and_quality(oracle, exe, tmp_path, mode, q):
    import torch
    from sperr_amd.api import SperrHip
    v = turbulence((30, 44, 37))
    dz, dy, dx = v.shape
    stream = oracle.comp_3d(v, (32, 32, 32), mode, q)
    (tmp_path / "c.sperr").write_bytes(stream)
    v.tofile(tmp_path / "orig.f32")
    p = subprocess.run([str(exe), str(tmp_path / "c.sperr"), str(tmp_path / "orig.f32"), str(dx), str(dy), str(dz),
                        str(tmp_path / "parent.f32"), str(tmp_path / "fig.f64")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    eng = SperrHip()
    dev = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    back = eng.decompress(dev, output_float=True)
    parent = np.fromfile(tmp_path / "parent.f32", dtype=np.float32).reshape(dz + 2, dy + 3, dx + 5).view(np.uint32)
    assert np.array_equal(parent[1:-1, 1:-2, 2:-3], back.cpu().numpy().view(np.uint32)), "the interior differs"
    halo = parent.copy()
    halo[1:-1, 1:-2, 2:-3] = 0x7FC0BEEF
    assert (halo == 0x7FC0BEEF).all(), "the halo was written"
    want = eng.quality(torch.from_numpy(v).cuda(), back)
    got = np.fromfile(tmp_path / "fig.f64", dtype=np.float64)
    ref = np.array([want.rmse, want.linfty, want.psnr, want.min, want.max, want.mean, want.var, want.mse])
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (got, ref)
