"""CPU: the quality figures' host half.  The two entry points exist and refuse without a GPU; quality_plan /
quality_finish (sperr_amd/csrc/quality.h), fed with partials from plain loops by tests/cpp/quality_check.cpp under
the address and undefined sanitizers, give the reference's bits (include/compat/sperr_helper.h inside the program,
tests/golden/quality_ref.json here); and where the reference is built, it still returns the fixture's bits."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_cases as qc   # noqa: E402

NAMES = ("sperrhip_quality_dev", "sperrhip_quality_batch_dev")
# every path of the finish: block edges, tails, the early return, range 0, subnormal squares, real decodes
HOST_CASES = ["size_1_f32", "size_8191_f64", "size_8192_f32", "size_8193_f64", "size_16384_f32", "size_16385_f64",
              "size_57349_f32", "size_57349_f64", "identical_f32", "identical_f64", "diff_first_f32", "diff_last_f64",
              "diff_tail_first_f32", "const_a_f32", "const_a_f64", "subnormal_f32", "batch3_v1_f32", "wmag17_bpp2_f32",
              "vort_crop_bpp2_f32", "smoke_bpp2_f32"]


def test_entry_points_declared_listed_exported():
    from sperr_amd import api
    header = open(os.path.join(ROOT, "include", "sperr_hip.h")).read()
    lib = api.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/sperr_hip.h"
        assert name in api.EXPORTS
        assert hasattr(lib, name)
    assert hasattr(api.SperrHip, "quality") and hasattr(api.SperrHip, "quality_batch")


def test_refusals_leave_out_untouched():
    """n == 0, a NULL pointer and nvol == 0 are refused before anything is leased or launched -- with or without a
    GPU; without one, a well-formed call fails as loudly."""
    import torch
    from sperr_amd import api
    lib = api.load_library()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    calls = [lambda o: lib.sperrhip_quality_dev(p, p, 1, 0, o, None),
             lambda o: lib.sperrhip_quality_dev(None, p, 1, 64, o, None),
             lambda o: lib.sperrhip_quality_dev(p, None, 1, 64, o, None),
             lambda o: lib.sperrhip_quality_batch_dev(p, p, 1, 0, 64, o, None),
             lambda o: lib.sperrhip_quality_batch_dev(p, p, 1, 2, 0, o, None)]
    if not torch.cuda.is_available():
        calls += [lambda o: lib.sperrhip_quality_dev(p, p, 1, 64, o, None),
                  lambda o: lib.sperrhip_quality_batch_dev(p, p, 0, 2, 16, o, None)]
    for call in calls:
        out = (ctypes.c_double * 16)(*([7.5] * 16))
        assert call(out) == -1
        assert list(out) == [7.5] * 16
    assert lib.sperrhip_quality_dev(p, p, 1, 64, None, None) == -1


def test_cpp_wrapper_compiles_and_refuses(tmp_path):
    """sperr::quality_dev (include/sperr_hip.hpp) for both types: n == 0 is RTNType::Error and `out` stays"""
    from sperr_amd import api
    src = '#include "sperr_hip.hpp"\nint main(){ std::array<double, 8> o; o.fill(7.5); const float* p = nullptr; ' \
          'const double* q = nullptr; float x = 1; bool bad = sperr::quality_dev(p, p, 4, o) != sperr::RTNType::Error || ' \
          'sperr::quality_dev(q, q, 4, o, nullptr) != sperr::RTNType::Error || ' \
          'sperr::quality_dev(&x, &x, 0, o) != sperr::RTNType::Error; for (double v : o) bad |= v != 7.5; return bad; }\n'
    (tmp_path / "caller.cpp").write_text(src)
    libdir = os.path.dirname(api.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / "caller.cpp"), "-o", str(tmp_path / "caller"), "-L" + libdir, "-lsperr_hip",
                           "-L/opt/rocm/lib", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([str(tmp_path / "caller")], timeout=120).returncode == 0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("quality_check") / "quality_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include", "compat"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "sperr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "quality_check.cpp"), "-o", str(path)])
    return path


def test_plan_at_the_block_edges(exe):
    p = subprocess.run([str(exe), "plan"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


@pytest.mark.parametrize("name", HOST_CASES)
def test_finish_gives_the_reference_bits(exe, oracle, tmp_path, name):
    rec = qc.load_fixture()[name]
    a, b = qc.cases(oracle)[name]()
    a.tofile(tmp_path / "a.bin")
    b.tofile(tmp_path / "b.bin")
    p = subprocess.run([str(exe), rec["dtype"], str(tmp_path / "a.bin"), str(tmp_path / "b.bin")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr      # (the program compared with include/compat itself)
    got = dict(zip(qc.FIGURES, p.stdout.split()))
    dt = qc.DTYPES[rec["dtype"]]
    for f in qc.FIGURES:
        if f == "psnr":      # the fixture's log10 ran in the reference build, this one in the program: the same libm
            assert qc.ulp_distance(qc.from_hex(got[f], dt), qc.from_hex(rec[f], dt), dt) <= 8
        elif f in ("min", "max"):
            assert qc.from_hex(got[f], dt) == qc.from_hex(rec[f], dt)
        else:
            assert int(got[f], 16) == int(rec[f], 16), f


def test_live_reference_returns_the_fixture(oracle):
    from oracle import pyoracle
    if not pyoracle.have_ref_library():   # (calls libSPERR_ref.so alone: the probe's age does not matter here)
        pytest.skip("oracle/_ref is not built here")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_quality_ref as gen
    ref = gen.RefStats()
    fx = qc.load_fixture()
    made = qc.cases(oracle, big=False)
    assert set(made) <= set(fx) and set(fx) - set(made) == {f"size_{(1 << 24) + 8197}_{k}" for k in qc.DTYPES}
    for name, make in made.items():
        a, b = make()
        assert gen.record(ref, a, b) == fx[name], name
