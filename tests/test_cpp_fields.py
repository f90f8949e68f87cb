"""GPU: the fields calls of the C++ header (include/sperr_hip.hpp: compress_fields_dev, decompress_fields_dev,
quality_fields_dev), driven by tests/cpp/fields_api_check.cpp on a device array of three interleaved fields: the
containers are the oracle's of every packed field byte for byte, the decode into fields 1..3 of a five-wide record with
padded rows and slices is the Python decode bit for bit with everything else untouched, and the figures are those of
SperrHip.quality on the packed arrays."""
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
    path = tmp_path_factory.mktemp("fields_api_check") / "fields_api_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "fields_api_check.cpp"), "-o", str(path),
                           "-L" + os.path.dirname(api.LIB_PATH), "-lsperr_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(api.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_cpp_fields_compress_decode_and_quality(oracle, exe, tmp_path):
    import torch
    from sperr_amd.api import SperrHip
    t = turbulence((30, 44, 37), dtype=np.float64)
    fields = np.stack([t.astype(np.float32), (100.0 * t).astype(np.float32), np.full(t.shape, 2.75, dtype=np.float32)])
    dz, dy, dx = t.shape
    np.ascontiguousarray(fields.transpose(1, 2, 3, 0)).tofile(tmp_path / "orig.f32")
    p = subprocess.run([str(exe), str(tmp_path / "orig.f32"), str(dx), str(dy), str(dz), str(tmp_path / "c.bin"),
                        str(tmp_path / "offs.u64"), str(tmp_path / "parent.f32"), str(tmp_path / "fig.f64")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    streams = (tmp_path / "c.bin").read_bytes()
    offs = np.fromfile(tmp_path / "offs.u64", dtype=np.uint64)
    assert len(offs) == 4 and offs[0] == 0 and offs[3] == len(streams)
    eng = SperrHip()
    pitch_y, pitch_z = (dx + 2) * 5, (dx + 2) * 5 * (dy + 1) + 3
    parent = np.fromfile(tmp_path / "parent.f32", dtype=np.float32).view(np.uint32)
    assert parent.size == pitch_z * dz
    want = np.full(parent.size, 0x7FC0BEEF, dtype=np.uint32)
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    figs = np.fromfile(tmp_path / "fig.f64", dtype=np.float64).reshape(3, 8)
    for f in range(3):
        c = streams[int(offs[f]):int(offs[f + 1])]
        assert c == oracle.comp_3d(fields[f], (32, 32, 32), 1, 2.5), f"container of field {f} differs"
        dev = torch.from_numpy(np.frombuffer(c, dtype=np.uint8).copy()).cuda()
        back = eng.decompress(dev, output_float=True)
        want[6 + z * pitch_z + y * pitch_y + x * 5 + f] = back.cpu().numpy().view(np.uint32)
        q = eng.quality(torch.from_numpy(fields[f]).cuda(), back)
        ref = np.array([q.rmse, q.linfty, q.psnr, q.min, q.max, q.mean, q.var, q.mse])
        assert np.array_equal(figs[f].view(np.uint64), ref.view(np.uint64)), (f, figs[f], ref)
    assert np.array_equal(parent, want), "the decoded fields differ, or something else was written"
