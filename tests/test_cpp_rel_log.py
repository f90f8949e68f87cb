"""GPU: the relative error calls of the C++ header with RelMap::log (include/sperr_hip.hpp: the trailing map argument of
rel_tolerance, rel_forward_dev and compress_rel_dev; the decodes take the kind from the side stream), driven by
tests/cpp/rel_log_api_check.cpp on tests/golden/vort_crop.f32 with a ball of zeros: y and the side stream are the log
model's, the containers of both kinds are the Python calls' byte for byte, and the decodes are the model's inverse of
the dense double decode bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import rel_log_model as L
import rel_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sperr_amd import api
    path = tmp_path_factory.mktemp("rel_log_api_check") / "rel_log_api_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "rel_log_api_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_cpp_rel_log_forward_compress_decode_and_inverse(exe, tmp_path):
    import torch
    from sperr_amd.api import SperrHip
    eps = 1e-2
    v = R.vort_with_zeros()
    dz, dy, dx = v.shape
    v.tofile(tmp_path / "vol.f32")
    names = ["c.bin", "side.bin", "y.f64", "dec.f32", "box.f64", "lin.bin"]
    p = subprocess.run([str(exe), str(tmp_path / "vol.f32"), str(dx), str(dy), str(dz), repr(eps)] +
                       [str(tmp_path / nm) for nm in names], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    y, zero, neg = L.forward(v)
    got_y = np.fromfile(tmp_path / "y.f64", dtype=np.float64)
    assert np.array_equal(got_y.view(np.uint64), y.view(np.uint64))
    assert (tmp_path / "side.bin").read_bytes() == L.side_stream(zero, neg, eps, True)
    eng = SperrHip()
    dev = torch.from_numpy(v).cuda()
    container, _ = eng.compress_rel(dev, (20, 18, 16), eps, map="log")
    assert (tmp_path / "c.bin").read_bytes() == bytes(container.cpu().numpy())
    linear, _ = eng.compress_rel(dev, (20, 18, 16), eps)
    assert (tmp_path / "lin.bin").read_bytes() == bytes(linear.cpu().numpy())
    yp = eng.decompress(container, output_float=False).cpu().numpy()
    want = L.inverse(yp, zero.reshape(v.shape), neg.reshape(v.shape), True, True)
    got = np.fromfile(tmp_path / "dec.f32", dtype=np.float32).reshape(v.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    cut = (slice(7, 20), slice(5, 22), slice(3, 24))
    want = L.inverse(yp[cut], zero.reshape(v.shape)[cut], neg.reshape(v.shape)[cut], False, True)
    box = np.fromfile(tmp_path / "box.f64", dtype=np.float64).reshape(want.shape)
    assert np.array_equal(box.view(np.uint64), want.view(np.uint64))
    eng.release()
