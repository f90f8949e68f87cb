"""GPU: the time-series calls of the C++ header (include/sperr_hip.hpp: series_plan, series_needs, series_tolerance,
series_forward_dev, series_inverse_dev, compress_series_dev, decompress_series_dev), driven by
tests/cpp/series_api_check.cpp on a drifting series of tests/golden/vort_crop.f32 in ragged chunks: the containers, the
info record, the bands and a decoded range of steps are the Python calls' bit for bit; the program itself checks the
host calls, the refusals and the stages' round trip."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sperr_amd import api
    path = tmp_path_factory.mktemp("series_api_check") / "series_api_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "series_api_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_cpp_series_calls(exe, tmp_path):
    import torch
    from sperr_amd.api import SperrHip
    from test_gpu_series import series_of
    steps = series_of("vort_crop", np.float32)
    ns, dz, dy, dx = steps.shape
    chunks, levels, t0, nt = (16, 10, 8), 3, 5, 4
    tol = 1e-3 * (float(steps.max()) - float(steps.min()))
    steps.tofile(tmp_path / "series.f32")
    names = ["c.bin", "offs.u64", "info.bin", "steps.f64", "bands.f64"]
    p = subprocess.run([str(exe), str(tmp_path / "series.f32"), str(ns), str(dx), str(dy), str(dz)] +
                       [str(c) for c in chunks] + [str(levels), repr(tol)] + [str(tmp_path / f) for f in names[:3]] +
                       [str(t0), str(nt)] + [str(tmp_path / f) for f in names[3:]], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    eng = SperrHip()
    d = torch.from_numpy(steps).cuda()
    conts, info = eng.compress_series(d, chunks, tol=tol, levels=levels)
    offs = np.fromfile(tmp_path / "offs.u64", dtype=np.uint64)
    blob = (tmp_path / "c.bin").read_bytes()
    assert [blob[int(offs[b]):int(offs[b + 1])] for b in range(ns)] == [bytes(c.cpu().numpy()) for c in conts]
    assert (tmp_path / "info.bin").read_bytes() == info
    back = eng.decompress_series(conts, info, t0=t0, nt=nt, output_float=False).cpu().numpy()
    assert (tmp_path / "steps.f64").read_bytes() == back.tobytes()
    assert (tmp_path / "bands.f64").read_bytes() == eng.series_forward(d, levels).cpu().numpy().tobytes()
    eng.release()
