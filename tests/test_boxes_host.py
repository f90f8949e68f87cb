"""CPU: sperr_amd/csrc/boxes.h -- which chunks a boxes call decodes, what each writes and where, in both of its forms,
and what it refuses -- checked by tests/cpp/boxes_check.cpp, a program of its own built with the address and undefined
sanitizers and run directly.  The header is plain C++, so the host compiler builds it.  Then the boundary: both names are
declared, listed and exported, the header compiles as C, the plan answers through ctypes, and without a GPU the decode
returns -1 and writes nothing."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")
NAMES = ("sperrhip_boxes_plan", "sperrhip_decompress_boxes_dev")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
_sz = C.c_size_t


@needs_gxx
def test_boxes_rule_tiling_geometry_and_refusals_under_sanitizers(tmp_path):
    exe = tmp_path / "boxes_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "boxes_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "boxes_check ok" in r.stdout and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-3000:]


def test_boxes_names_are_declared_listed_and_exported():
    from sperr_amd import api
    header = open(os.path.join(ROOT, "include", "sperr_hip.h")).read()
    lib = api.load_library()
    for name in NAMES:
        assert name + "(" in header, f"{name} is not declared in include/sperr_hip.h"
        assert name in api.EXPORTS, f"{name} is not in api.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not on PATH")
def test_header_with_the_boxes_section_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "sperr_hip.h"\n'
                   "int use(const void* const* p, const size_t* n, const size_t* lo, const size_t* d, void* o, size_t* r)\n"
                   "{\n"
                   "  return sperrhip_boxes_plan(1, d, d, 0, lo, 1, d, 0, r) +\n"
                   "         sperrhip_decompress_boxes_dev(p, n, 1, 0, lo, 1, d, 0, 0, 1, o, 0, 0);\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        "-c", str(src), "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _plan(lib, ncont, vol, chunks, which, los, box, level=None):
    out = (_sz * 5)()
    nbox = len(los)
    rc = lib.sperrhip_boxes_plan(ncont, (_sz * 3)(*vol), (_sz * (3 * len(chunks)))(*[v for c in chunks for v in c]),
                                 None if which is None else (C.c_uint32 * nbox)(*which),
                                 (_sz * (3 * nbox))(*[v for o in los for v in o]), nbox, (_sz * 3)(*box),
                                 None if level is None else C.byref(_sz(level)), out)
    return rc, list(out)


def test_boxes_plan_answers_through_ctypes():
    from sperr_amd import api
    lib = api.load_library()
    c32 = (32, 32, 32)
    # a time series: the same box of three containers, no chunk shared -- direct, 8 chunks per container
    rc, out = _plan(lib, 3, (64, 64, 64), [c32] * 3, None, [(20, 20, 20)] * 3, (24, 24, 24))
    assert rc == 0 and out == [24, 24, 0, 0, 3 * 24 ** 3]
    # crops of one container that overlap: staged, fewer slots than pairs, the slots whole in the staging array
    rc, out = _plan(lib, 1, (64, 64, 64), [c32], [0, 0], [(0, 0, 0), (8, 8, 8)], (24, 20, 17))
    assert rc == 0 and out == [1, 2, 1, 32 ** 3, 2 * 24 * 20 * 17]
    # merged remainders: 56 x 48 x 40 in 32^3 is 2 x 1 x 1 chunks, (32, 48, 40) and (24, 48, 40)
    rc, out = _plan(lib, 1, (56, 48, 40), [c32], [0, 0], [(30, 0, 0), (31, 1, 1)], (4, 4, 4))
    assert rc == 0 and out == [2, 4, 1, 32 * 48 * 80, 128]
    # a level: the grid is the chunks' corners of that level (sperrhip_multires_levels), 2 x 2 x 2 of them here; a box
    # of the corner's size one sample off the origin meets all eight, in either container
    nlev, ld = _sz(0), (_sz * 48)()
    lib.sperrhip_multires_levels.argtypes = [_sz] * 6 + [C.POINTER(_sz), C.POINTER(_sz)]
    assert lib.sperrhip_multires_levels(64, 64, 64, 32, 32, 32, C.byref(nlev), ld) == 0 and nlev.value >= 2
    for h in range(nlev.value):
        cr = ld[3 * h] // 2
        assert ld[3 * h] == ld[3 * h + 1] == ld[3 * h + 2] and cr >= 1
        rc, out = _plan(lib, 2, (64, 64, 64), [c32] * 2, None, [(1, 1, 1)] * 2, (cr, cr, cr), level=h)
        met = 2 * (8 if cr >= 2 else 1)   # (a corner of one sample: the box is that one sample of chunk (1, 1, 1))
        assert rc == 0 and out == [met, met, 0, 0, 2 * cr ** 3], (h, out)
        assert _plan(lib, 2, (64, 64, 64), [c32] * 2, None, [(cr + 1, 0, 0)] * 2, (cr, 1, 1), level=h)[0] == -1
    assert _plan(lib, 1, (64, 64, 64), [c32], None, [(0, 0, 0)], (1, 1, 1), level=nlev.value)[0] == -1
    # refusals known from dims alone
    assert _plan(lib, 2, (64, 64, 64), [c32, (16, 16, 16)], None, [(0, 0, 0)] * 2, (2, 2, 2), level=0)[0] == -1
    assert _plan(lib, 1, (64, 64, 64), [c32], None, [(0, 0, 0)], (2, 2, 2), level=99)[0] == -1
    assert _plan(lib, 1, (40, 48, 56), [c32], None, [(0, 0, 0)], (2, 2, 2), level=0)[0] == -1   # chunks do not tile it
    assert _plan(lib, 1, (64, 64, 64), [c32], [1], [(0, 0, 0)], (2, 2, 2))[0] == -1
    assert _plan(lib, 1, (64, 64, 64), [c32], [0], [(60, 0, 0)], (5, 2, 2))[0] == -1
    assert _plan(lib, 1, (64, 64, 64), [c32], [0], [(0, 0, 0)], (5, 0, 2))[0] == -1
    assert _plan(lib, 2, (64, 64, 64), [c32] * 2, None, [(0, 0, 0)], (5, 5, 2))[0] == -1
    assert lib.sperrhip_boxes_plan(0, None, None, None, None, 0, None, None, None) == -1


def test_decompress_boxes_without_a_gpu_returns_minus_one_and_writes_nothing():
    """in a child process that sees no device: the call has no CPU path, fails loudly and leaves the output alone"""
    code = (
        "import ctypes as C, numpy as np, sys\n"
        "from sperr_amd import api\n"
        "lib = api.load_library()\n"
        "sz = C.c_size_t\n"
        "src = np.zeros(64, dtype=np.uint8)\n"
        "out = np.full(64, 0x7FC0BEEF, dtype=np.uint32)\n"
        "ptrs = (C.c_void_p * 1)(src.ctypes.data)\n"
        "rc = lib.sperrhip_decompress_boxes_dev(ptrs, (sz * 1)(64), 1, None, (sz * 3)(0, 0, 0), 1, (sz * 3)(2, 2, 2),\n"
        "                                       None, 0, 1, out.ctypes.data, out.nbytes, None)\n"
        "assert rc == -1, rc\n"
        "assert (out == 0x7FC0BEEF).all()\n"
        "print('refused')\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert p.returncode == 0 and "refused" in p.stdout, p.stdout + p.stderr
