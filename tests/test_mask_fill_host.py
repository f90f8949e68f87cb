"""CPU: sperr_amd/csrc/mask_fill.h -- the smooth in-fill of missing values.  tests/cpp/mask_fill_check.cpp, a program of
its own built with the address and undefined sanitizers and run directly, runs the header's host statement of the rule
(plain loops) on volumes read from files; its output is compared bit for bit with tests/mask_fill_model.py, the numpy
statement of the same rule, for fp32 and fp64, six shapes and seven masks.  Beside that: the levels and the pyramid's
byte count against the model, the P / Q index rule, the refusal of a sum that is not finite, and -- with the model and the
CPU oracle alone -- that the container of the smooth in-fill is smaller than that of the midrange in-fill."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mask_fill_model as F
import mask_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")
SHAPES = [(1, 1, 1), (2, 2, 2), (5, 3, 2), (1, 1, 70), (70, 1, 1), (30, 44, 37)]      # (z, y, x)
MASKS = ["ball", "slab", "density_0.1", "density_0.9", "single_valid", "all", "none"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")


def top_cells():
    text = open(os.path.join(CSRC, "mask_fill.h")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+kMaskTopCells\s*=\s*(\d+)\s*;", text).group(1))


def make_mask(name, shape):
    if name == "ball":
        return M.ball_mask(shape, 0.4 * max(shape))
    if name == "slab":
        return M.slab_mask(shape, (3 * shape[2]) // 4)
    if name.startswith("density"):
        return M.density_mask(shape, float(name.split("_")[1]), 3 + len(name))
    if name == "single_valid":
        m = np.ones(shape, dtype=bool)
        m.reshape(-1)[(2 * m.size) // 3] = False
        return m
    return np.ones(shape, dtype=bool) if name == "all" else np.zeros(shape, dtype=bool)


def make_volume(shape, dtype, mask, seed):
    z, y, x = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in shape), indexing="ij")
    rng = np.random.default_rng(seed)
    v = (280.0 + 9.0 * np.sin(0.21 * x + 0.4) * np.cos(0.17 * y) + 0.3 * z + 0.05 * rng.standard_normal(shape)).astype(dtype)
    v[mask] = np.nan
    return v


def ibits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("mask_fill_check") / "mask_fill_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "mask_fill_check.cpp"), "-o", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def run_fill(exe, tmp_path, v, mask):
    """the program's in-filled volume, or None when it refuses"""
    dz, dy, dx = v.shape
    v.tofile(tmp_path / "vol.bin")
    mask.reshape(-1).astype(np.uint8).tofile(tmp_path / "bits.u8")
    out = tmp_path / "out.bin"
    if out.exists():
        out.unlink()
    r = subprocess.run([str(exe), "fill", "f32" if v.dtype == np.float32 else "f64", str(dx), str(dy), str(dz),
                        str(tmp_path / "vol.bin"), str(tmp_path / "bits.u8"), str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    if "refused" in r.stdout:
        assert not out.exists()
        return None
    return np.fromfile(out, dtype=v.dtype).reshape(v.shape)


def test_index_rule_levels_kinds_and_refusal_under_sanitizers(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "mask_fill_check ok" in r.stdout and "runtime error" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_headers_loops_equal_the_model_bit_for_bit(exe, tmp_path, shape, dtype):
    for k, name in enumerate(MASKS):
        mask = make_mask(name, shape)
        v = make_volume(shape, dtype, mask, 10 * len(shape) + k)
        want = F.smooth_filled(v, mask)
        got = run_fill(exe, tmp_path, v, mask)
        assert got is not None and want is not None, name
        assert np.array_equal(ibits(got), ibits(want)), name
        assert np.array_equal(ibits(got)[~mask], ibits(v)[~mask]), name + ": a valid sample changed"
        assert np.isfinite(got).all(), name
        if name == "all":
            assert not ibits(got).any()
        if name == "single_valid":
            assert np.array_equal(ibits(got), ibits(np.full(shape, v[~mask][0], dtype=dtype)))


@pytest.mark.parametrize("shape", SHAPES + [(65, 66, 70), (512, 512, 512), (1, 1, 1000003)],
                         ids=lambda s: "x".join(map(str, s)))
def test_levels_and_pyramid_bytes_equal_the_model(exe, shape):
    dz, dy, dx = shape
    r = subprocess.run([str(exe), "plan", str(dx), str(dy), str(dz)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    lines = [tuple(int(t) for t in ln.split()) for ln in r.stdout.strip().splitlines()]
    levels = F.level_shapes(shape)
    nlev, g, nbytes, lds = lines[0]
    assert nlev == len(levels) - 1
    assert lines[1:] == [(s[2], s[1], s[0]) for s in levels]
    assert g == F.global_levels(shape, top_cells())
    assert nbytes == F.pyramid_bytes(shape, top_cells())
    assert lds == sum(s[0] * s[1] * s[2] for s in levels[g + 1:])


def test_model_index_rule_at_both_ends():
    assert [F.pq(i, 4) for i in range(8)] == [(0, 0), (0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (3, 3)]
    assert F.pq(6, 4) == (3, 2) and F.pq(4, 3) == (2, 1) and F.pq(0, 1) == (0, 0) and F.pq(1, 1) == (0, 0)
    assert F.level_shapes((30, 44, 37))[1:3] == [(15, 22, 19), (8, 11, 10)]
    assert F.launches((30, 44, 37), 2048) == {"k_mask_pull0": 1, "k_mask_pull": 0, "k_mask_top": 1, "k_mask_push": 0,
                                              "k_mask_fill_smooth": 1}
    assert F.launches((65, 66, 70), 2048)["k_mask_pull"] == 1


def test_a_sum_that_is_not_finite_is_refused(exe, tmp_path):
    v = np.zeros((1, 3, 5), dtype=np.float64)
    mask = np.zeros(v.shape, dtype=bool)
    mask[0, 2, :] = True
    v[0, 0, 2] = v[0, 0, 3] = 1.7e308          # children of one cell of level 1
    assert F.smooth_filled(v, mask) is None and run_fill(exe, tmp_path, v, mask) is None
    v[0, 0, 2] = 0.0                           # ... one of them alone is fine
    want = F.smooth_filled(v, mask)
    got = run_fill(exe, tmp_path, v, mask)
    assert want is not None and got is not None and np.array_equal(ibits(got), ibits(want))
    # the same magnitudes as floats are nowhere near the doubles' range
    f = np.full((2, 2, 2), 3.0e38, dtype=np.float32)
    m = np.zeros(f.shape, dtype=bool)
    m[1, 1, 1] = True
    got = run_fill(exe, tmp_path, f, m)
    assert got is not None and np.array_equal(ibits(got), ibits(F.smooth_filled(f, m)))


# ---- what the smooth fill is for: the container's size ----------------------------------------------------------------
SIZE_SHAPE = (48, 64, 56)           # (z, y, x): 56 x 64 x 48 in x, y, z
SIZE_CHUNKS = (64, 64, 64)
SIZE_CASES = [(3, 0.1), (3, 0.01), (2, 80.0)]


def size_field():
    z, y, x = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in SIZE_SHAPE), indexing="ij")
    smooth = 6.0 * np.sin(2 * np.pi * x / 56.0 + 0.3) * np.cos(2 * np.pi * y / 64.0) + 4.0 * np.sin(2 * np.pi * z / 48.0 + 1.1) \
        + 2.0 * np.cos(2 * np.pi * (x + y + z) / 40.0)
    noise = np.random.default_rng(2024).standard_normal(SIZE_SHAPE)
    return (280.0 + smooth + 0.05 * noise).astype(np.float32)


@pytest.mark.parametrize("which", ["ball", "density"])
def test_smooth_infill_gives_the_smaller_container(oracle, which):
    mask = M.ball_mask(SIZE_SHAPE, 20) if which == "ball" else M.density_mask(SIZE_SHAPE, 0.3, 3)
    v = size_field()
    v[mask] = np.nan
    mid, sm = M.filled(v, mask), F.smooth_filled(v, mask)
    assert np.array_equal(ibits(mid)[~mask], ibits(sm)[~mask])
    for mode, q in SIZE_CASES:
        a, b = len(oracle.comp_3d(mid, SIZE_CHUNKS, mode, q)), len(oracle.comp_3d(sm, SIZE_CHUNKS, mode, q))
        print(f"{which} mode {mode} quality {q}: midrange {a} bytes, smooth {b} bytes, ratio {b / a:.3f}")
        assert b < a, (which, mode, q, a, b)
