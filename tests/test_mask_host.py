"""CPU: sperr_amd/csrc/mask.h -- the rules of missing values: the predicate, the order of the valid samples and the fill
value, the mask stream's header with every refusal, the kind rule at its boundary, words <-> toggles both ways, the
ballot interleave of the 16-byte forms -- checked by tests/cpp/mask_check.cpp, a program of its own built with the
address and undefined sanitizers and run directly.  The header is plain C++, so the host compiler builds it.  The
program's streams of the four masks of a (30, 44, 37) volume are compared with tests/mask_model.py, the numpy statement
of the same rules."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mask_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")
SHAPE = (30, 44, 37)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("mask_check") / "mask_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "mask_check.cpp"), "-o", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def test_mask_rules_header_kinds_and_refusals_under_sanitizers(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "mask_check ok" in r.stdout and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-3000:]


MASKS = {
    # name: (mask, kind, count, stream bytes) -- the table of the rule's statement
    "ball": (lambda: M.ball_mask(SHAPE, 12), M.KIND_TOGGLES, 874, 3528),
    "slab": (lambda: M.slab_mask(SHAPE, 30), M.KIND_BITS, 764, 6144),
    "density": (lambda: M.density_mask(SHAPE, 0.1, 7), M.KIND_BITS, 764, 6144),
    "all": (lambda: np.ones(SHAPE, dtype=bool), M.KIND_TOGGLES, 1, 36),
}


@pytest.mark.parametrize("name", sorted(MASKS))
def test_mask_streams_of_the_program_are_the_models(exe, tmp_path, name):
    make, kind, count, nbytes = MASKS[name]
    mask = make()
    want = M.stream(mask)
    assert M.parse(want) == (kind, mask.size, int(mask.sum()), count) and len(want) == nbytes
    assert np.array_equal(M.bits_of_stream(want), mask.reshape(-1))
    mask.reshape(-1).astype(np.uint8).tofile(tmp_path / "bits.u8")
    r = subprocess.run([str(exe), "stream", str(tmp_path / "bits.u8"), str(tmp_path / "stream.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    assert (tmp_path / "stream.bin").read_bytes() == want


def test_model_boundary_of_the_kind_rule():
    for nt, kind, nbytes in ((15, M.KIND_TOGGLES, 92), (16, M.KIND_BITS, 96)):
        b = np.zeros(512, dtype=bool)
        for i in range(nt):
            b[3 * i + 1:] ^= True
        s = M.stream(b)
        assert M.toggles(b).size == nt and M.parse(s)[0] == kind and len(s) == nbytes
    assert M.max_size(48840) == 32 + 8 * 764
