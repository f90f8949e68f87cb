"""GPU: the mask calls of the C++ header (include/sperr_hip.hpp: mask_make_dev, mask_apply_dev, compress_masked_dev,
decompress_masked_dev, quality_masked_dev), driven by tests/cpp/mask_api_check.cpp on a (30, 44, 37) volume with a ball
of NaNs: the mask is the model's, the container the oracle's of the model's in-filled volume byte for byte, the decodes
are the Python decodes with the values put in bit for bit, and the figures are those of SperrHip.quality on the
compacted arrays."""
import os
import subprocess

import numpy as np
import pytest

import mask_model as M
from sperr_amd.synth import turbulence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sperr_amd import api
    path = tmp_path_factory.mktemp("mask_api_check") / "mask_api_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "mask_api_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_cpp_mask_compress_decode_apply_and_quality(oracle, exe, tmp_path):
    import torch
    from sperr_amd.api import SperrHip
    shape = (30, 44, 37)
    v = turbulence(shape, dtype=np.float64).astype(np.float32)
    mask = M.ball_mask(shape, 12)
    v[mask] = np.nan
    dz, dy, dx = shape
    v.tofile(tmp_path / "vol.f32")
    names = ["c.bin", "mask.bin", "dec.f32", "box.f32", "fig.f64"]
    p = subprocess.run([str(exe), str(tmp_path / "vol.f32"), str(dx), str(dy), str(dz)] +
                       [str(tmp_path / nm) for nm in names], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    container = (tmp_path / "c.bin").read_bytes()
    assert (tmp_path / "mask.bin").read_bytes() == M.stream(mask)
    assert container == oracle.comp_3d(M.filled(v, mask), (32, 32, 32), 1, 2.5), "the container differs from the oracle's"
    eng = SperrHip()
    dev = torch.from_numpy(np.frombuffer(container, dtype=np.uint8).copy()).cuda()
    whole = eng.decompress(dev).cpu().numpy()
    want = whole.copy()
    want[mask] = np.float32(-7.5)
    got = np.fromfile(tmp_path / "dec.f32", dtype=np.float32).reshape(shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    box = eng.decompress_box(dev, (3, 5, 7), (20, 9, 20)).cpu().numpy()
    box[mask[7:27, 5:14, 3:23]] = np.float32(1e20)
    got = np.fromfile(tmp_path / "box.f32", dtype=np.float32).reshape(box.shape)
    assert np.array_equal(got.view(np.uint32), box.view(np.uint32))
    keep = torch.from_numpy(~mask).cuda()
    q = eng.quality(torch.from_numpy(v).cuda()[keep].contiguous(), torch.from_numpy(want).cuda()[keep].contiguous())
    ref = np.array([q.rmse, q.linfty, q.psnr, q.min, q.max, q.mean, q.var, q.mse])
    fig = np.fromfile(tmp_path / "fig.f64", dtype=np.float64)
    assert np.array_equal(fig.view(np.uint64), ref.view(np.uint64)), (fig, ref)
