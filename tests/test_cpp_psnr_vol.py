"""GPU: the whole-volume PSNR calls of the C++ header (include/sperr_hip.hpp: range_dev, compress_psnr_dev), driven by
tests/cpp/psnr_vol_api_check.cpp on tests/golden/vort_crop.f32 in chunks of two shapes: the range and the container are
the Python calls' bit for bit; the program itself checks the refusals, the dense view and an explicit range."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sperr_amd import api
    path = tmp_path_factory.mktemp("psnr_vol_api_check") / "psnr_vol_api_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "psnr_vol_api_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_cpp_range_and_compress_to_psnr(exe, tmp_path):
    import torch
    from sperr_amd.api import SperrHip
    v = np.fromfile(os.path.join(ROOT, "tests", "golden", "vort_crop.f32"), dtype=np.float32).reshape(33, 36, 40)
    dz, dy, dx = v.shape
    chunks, psnr = (20, 18, 16), 70.0
    v.tofile(tmp_path / "vol.f32")
    p = subprocess.run([str(exe), str(tmp_path / "vol.f32"), str(dx), str(dy), str(dz)] + [str(c) for c in chunks] +
                       [repr(psnr), str(tmp_path / "c.bin"), str(tmp_path / "range.f64")], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    eng = SperrHip()
    d = torch.from_numpy(v).cuda()
    lo, hi = np.fromfile(tmp_path / "range.f64", dtype=np.float64)
    assert (lo, hi) == eng.value_range(d) == (float(v.min()), float(v.max()))
    assert (tmp_path / "c.bin").read_bytes() == bytes(eng.compress_to_psnr(d, chunks, psnr).cpu().numpy())
    eng.release()
