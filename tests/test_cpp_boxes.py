"""GPU: sperr::decompress_boxes_dev of the C++ header (include/sperr_hip.hpp), driven by tests/cpp/boxes_api_check.cpp
on three containers that it puts into device allocations of their own: the same box of every container as floats (the
direct form), three boxes of which two overlap as doubles (the staged form) and one sample of the coarsest level per
container are the oracle's decodes cut with numpy, bit for bit; the program itself checks the refusals and that
nothing behind the result is written."""
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
    path = tmp_path_factory.mktemp("boxes_api_check") / "boxes_api_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "boxes_api_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_cpp_boxes_direct_staged_and_level(oracle, exe, tmp_path):
    vols = [turbulence((64, 64, 64), seed=s) for s in (21, 22, 23)]
    containers = [oracle.comp_3d(vols[0], (32, 32, 32), 1, 2.0), oracle.comp_3d(vols[1], (32, 32, 32), 1, 3.0),
                  oracle.comp_3d(vols[2], (32, 32, 32), 3, 1e-3)]
    offs = np.cumsum([0] + [len(c) for c in containers]).astype(np.uint64)
    (tmp_path / "c.bin").write_bytes(b"".join(containers))
    offs.tofile(tmp_path / "offs.u64")
    p = subprocess.run([str(exe), str(tmp_path / "c.bin"), str(tmp_path / "offs.u64"), str(tmp_path / "direct.f32"),
                        str(tmp_path / "staged.f64"), str(tmp_path / "level.f64")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr

    def crop(full, lo, dims=(20, 10, 9)):
        return np.ascontiguousarray(full[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]])

    f32 = [oracle.decomp_3d(c, True) for c in containers]
    f64 = [oracle.decomp_3d(c, False) for c in containers]
    direct = np.fromfile(tmp_path / "direct.f32", dtype=np.float32)
    want = np.stack([crop(f, (5, 6, 7)) for f in f32])
    assert np.array_equal(direct.view(np.uint32), want.view(np.uint32).ravel()), "the direct form's boxes differ"
    staged = np.fromfile(tmp_path / "staged.f64", dtype=np.float64)
    want = np.stack([crop(f64[0], (5, 6, 7)), crop(f64[0], (6, 7, 8)), crop(f64[2], (0, 0, 0))])
    assert np.array_equal(staged.view(np.uint64), want.view(np.uint64).ravel()), "the staged form's boxes differ"
    level = np.fromfile(tmp_path / "level.f64", dtype=np.float64)
    want = np.array([oracle.decomp_3d_multi_res(c)[1][0][1, 0, 1] for c in containers])
    assert np.array_equal(level.view(np.uint64), want.view(np.uint64)), "the level's samples differ"
