"""GPU: the size mode's calls of the C++ header (include/sperr_hip.hpp: size_survey_dev, compress_size_dev), driven by
tests/cpp/size_api_check.cpp on tests/golden/vort_crop.f32 in chunks of two shapes: the survey, the budgets and the
container are the Python calls' byte for byte, and a target that does not hold the headers is refused with the
destination untouched (the program checks that itself)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sperr_amd import api
    path = tmp_path_factory.mktemp("size_api_check") / "size_api_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "size_api_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_cpp_survey_and_compress_to_size(exe, tmp_path):
    import torch
    from sperr_amd.api import SperrHip
    v = np.fromfile(os.path.join(ROOT, "tests", "golden", "vort_crop.f32"), dtype=np.float32).reshape(33, 36, 40)
    dz, dy, dx = v.shape
    chunks, target = (20, 18, 16), 9000
    v.tofile(tmp_path / "vol.f32")
    names = ["c.bin", "budgets.u64", "survey.bin"]
    p = subprocess.run([str(exe), str(tmp_path / "vol.f32"), str(dx), str(dy), str(dz)] + [str(c) for c in chunks] +
                       [str(target)] + [str(tmp_path / nm) for nm in names], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    eng = SperrHip()
    d = torch.from_numpy(v).cuda()
    sv = eng.size_survey(d, chunks)
    container, budgets = eng.compress_to_size(d, chunks, target, return_plan=True)
    n = len(budgets)
    assert n == 8
    assert (tmp_path / "c.bin").read_bytes() == bytes(container.cpu().numpy())
    assert np.array_equal(np.fromfile(tmp_path / "budgets.u64", dtype=np.uint64), budgets)
    raw = (tmp_path / "survey.bin").read_bytes()
    assert len(raw) == n * (8 + 4 + 32 * 8 + 1)
    assert raw[:8 * n] == sv["q"].tobytes() and raw[8 * n:12 * n] == sv["nbp"].tobytes()
    assert raw[12 * n:12 * n + 256 * n] == sv["end"].tobytes() and raw[268 * n:] == sv["is_const"].astype(np.uint8).tobytes()
    eng.release()
