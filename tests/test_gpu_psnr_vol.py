"""GPU (-m gpu): compression to a PSNR of the whole volume (psnr_vol.h) -- the range kernel, the
ladder kernels through the public call, the container.  The yardsticks are numpy and the CPU oracle; every compare is on
bytes or bit patterns, nothing has a tolerance.

  range      value_range against numpy: fp32 and fp64; 16^3, 17 x 19 x 23, 64^3; a ghost-cell view with an odd x origin;
             the extreme in the first element, the last, and in a ghost cell (ignored); a NaN refused; an infinity an
             extreme, refused at compress
  ladder     one-chunk volumes built so that the oracle's search stops at every rung 0 .. 4 (tests/psnr_vol_model.py):
             the q in the chunk header is the oracle's, the stream is the one composed from the oracle's stages
  plume      the 64^3 field of tests/test_gpu_size.py, fp32 and fp64, at 40 / 60 / 80 / 100 dB in 32^3 chunks and as one
             64^3 chunk (64 strides and the empty 65th, which a second workgroup takes): every chunk stream is the oracle's
             composed stream; decompress, decompress_box and decompress(pct=50) are the oracle's bits; the container is
             strictly shorter than mode 2's
  widths     fp64 at 200 and 225 dB: chunks of 32-bit and of 64-bit coefficients in one batch; 400 dB refused
  range=     the volume's own given explicitly: the same bytes; twice that: the oracle's streams at that range
  shapes     a ragged volume of two chunk shapes; a constant chunk; a constant volume; a ghost-cell view against the
             packed copy
  witnesses  k_mse_ladder once per batch and never k_mse_strides; mode 2 launches no k_mse_ladder
  children   a split workspace (a chunk per batch) and a poisoned workspace, each in a process of its own"""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import psnr_vol_model as pm
from sperr_amd.farm import chunk_grid, split_container
from test_gpu_size import CHUNKS, bits, chunk_of, cuda, host, plume

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    return SperrHip()


@pytest.fixture(scope="module")
def est(oracle):
    f = oracle.lib.orc_estimate_q_psnr
    f.restype = C.c_double
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_double]
    return f


# ---- the oracle's side: a chunk's stream at a common range, composed from its stage calls ---------------------------------

def oracle_chunk(oracle, est, ck, rng, psnr):
    """(stream, q, coefficient width, all coefficients zero) of one chunk: condition, dwt3d, the q of the oracle's own
    search started from `rng`, quantize, speck3d_encode"""
    v, hdr, const = oracle.condition(np.ascontiguousarray(ck, dtype=np.float64))
    if const:
        return hdr, None, None, None
    w = np.ascontiguousarray(oracle.dwt3d(v))
    q = est(w.ctypes.data, w.size, rng, psnr)
    coef, sign, width = oracle.quantize(w, q)
    return hdr[:9] + struct.pack("<d", q) + oracle.speck3d_encode(coef, sign, 0), q, width, not coef.any()


def oracle_chunks(oracle, est, vol, chunks, rng, psnr):
    return [oracle_chunk(oracle, est, chunk_of(vol, box), rng, psnr) for box in chunk_grid(vol.shape, chunks)]


def check_streams(container, want):
    _, _, _, parts = split_container(container)
    assert len(parts) == len(want)
    for c, (part, (stream, q, _, _)) in enumerate(zip(parts, want)):
        if q is not None:
            assert struct.unpack_from("<d", part, 9)[0] == q, (c, struct.unpack_from("<d", part, 9)[0], q)
        assert bytes(part) == stream, c


# ---- a. the range ------------------------------------------------------------------------------------------------------

RANGE_SHAPES = {"16": (16, 16, 16), "17x19x23": (23, 19, 17), "64": (64, 64, 64)}   # (z, y, x)


def range_field(shape, dtype, where):
    rng = np.random.default_rng(3)
    v = rng.standard_normal(shape).astype(dtype)
    if where == "first":
        v.flat[0], v.flat[1] = 9.5, -7.25
    elif where == "last":
        v.flat[-1], v.flat[-2] = -9.5, 7.25
    return v


@pytest.mark.parametrize("where", ["inside", "first", "last"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", sorted(RANGE_SHAPES))
def test_value_range_is_numpys(eng, shape, dtype, where):
    v = range_field(RANGE_SHAPES[shape], dtype, where)
    lo, hi = eng.value_range(cuda(v))
    assert (lo, hi) == (float(v.min()), float(v.max()))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", sorted(RANGE_SHAPES))
def test_value_range_of_a_ghost_cell_view(eng, shape, dtype):
    dz, dy, dx = RANGE_SHAPES[shape]
    big = np.random.default_rng(5).standard_normal((dz + 3, dy + 2, dx + 6)).astype(dtype)
    big[0, 0, 0], big[-1, -1, -1] = 100.0, -100.0          # ghost cells: ignored
    big[2, 1, 2], big[2 + dz - 1, 1 + dy - 1, 3 + dx] = 50.0, -50.0   # ... also the ones next to a row's ends
    inner = big[2:2 + dz, 1:1 + dy, 3:3 + dx]              # (an odd x origin: rows start off a 16-byte boundary)
    lo, hi = eng.value_range(cuda(big)[2:2 + dz, 1:1 + dy, 3:3 + dx])
    assert (lo, hi) == (float(inner.min()), float(inner.max())) and hi < 50.0 and lo > -50.0


def test_value_range_refuses_a_nan_and_shows_an_infinity(eng):
    from sperr_amd.api import SperrHipError
    v = range_field((17, 19, 23), np.float32, "inside")
    for pos in (0, 4321, v.size - 1):
        w = v.copy()
        w.flat[pos] = np.nan
        with pytest.raises(SperrHipError):
            eng.value_range(cuda(w))
        with pytest.raises(SperrHipError):
            eng.compress_to_psnr(cuda(w), (16, 16, 16), 60.0)
        with pytest.raises(SperrHipError):
            eng.compress_to_psnr(cuda(w), (16, 16, 16), 60.0, range=2.0)
    w = v.copy()
    w.flat[77] = -np.inf
    assert eng.value_range(cuda(w)) == (-np.inf, float(v.max()))
    import torch
    out = torch.full((eng.max_compressed_size(w.shape, (16, 16, 16), 60.0, 2),), 0xA5, dtype=torch.uint8, device="cuda")
    n = C.c_size_t(12345)
    d = cuda(w)
    rtn = eng.lib.sperrhip_compress_psnr_dev(d.data_ptr(), None, 1, 23, 19, 17, 16, 16, 16, 60.0, 0.0, out.data_ptr(),
                                             out.numel(), C.byref(n), eng._stream())
    assert rtn == -1 and n.value == 12345 and bool((out == 0xA5).all())


def test_arguments_refused_before_anything_is_launched(eng):
    d = cuda(range_field((16, 16, 16), np.float32, "inside"))
    import torch
    out = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    n = C.c_size_t(0)
    call = eng.lib.sperrhip_compress_psnr_dev
    st = eng._stream()
    ok = (d.data_ptr(), None, 1, 16, 16, 16, 16, 16, 16, 60.0, 0.0, out.data_ptr(), out.numel(), C.byref(n), st)

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return call(*a)
    assert with_(0, None) == -1 and with_(11, None) == -1 and with_(13, None) == -1
    assert with_(3, 0) == -1 and with_(4, 0) == -1 and with_(5, 0) == -1
    assert with_(9, float("nan")) == -1 and with_(9, float("inf")) == -1 and with_(9, float("-inf")) == -1
    assert with_(10, -1.0) == -1 and with_(10, float("inf")) == -1 and with_(10, float("nan")) == -1
    from sperr_amd.api import View
    assert with_(1, C.byref(View(15, 16 * 16))) == -1 and with_(1, C.byref(View(16, 16 * 16 + 8))) == -1
    assert n.value == 0
    assert call(*ok) == 0 and n.value > 0


# ---- b. the ladder through the public call -----------------------------------------------------------------------------

@pytest.mark.parametrize("rung,inv_q0", list(enumerate(pm.LADDER_INV_Q0)))
@pytest.mark.parametrize("shape", sorted(pm.LADDER_SHAPES))
def test_every_rung_of_the_ladder(eng, oracle, est, shape, rung, inv_q0):
    vol = cached(("ladder", shape), lambda: pm.ladder_chunk(oracle, pm.LADDER_SHAPES[shape]))
    dz, dy, dx = vol.shape
    rng = pm.range_for(inv_q0, pm.LADDER_PSNR)
    t, qs = eng.psnr_ladder(rng, pm.LADDER_PSNR)
    mt, mqs = pm.ladder(rng, pm.LADDER_PSNR)
    assert t == mt and list(qs) == mqs
    want = oracle_chunk(oracle, est, vol, rng, pm.LADDER_PSNR)
    assert mqs.index(want[1]) == rung   # (the condition: the oracle stops at this rung)
    c = host(eng.compress_to_psnr(cuda(vol), (dx, dy, dz), pm.LADDER_PSNR, range=rng))
    check_streams(c, [want])


# ---- c. the plume -------------------------------------------------------------------------------------------------------

def coded(eng, vol, chunks, psnr, rng=None):
    return cached(("coded", id(vol), chunks, psnr, rng), lambda: host(eng.compress_to_psnr(cuda(vol), chunks, psnr, range=rng)))


@pytest.mark.parametrize("psnr", [40.0, 60.0, 80.0, 100.0])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_plume(eng, oracle, est, dtype, psnr):
    vol = plume(dtype)
    as_float = dtype == np.float32
    rng = pm.value_range(vol)
    container = coded(eng, vol, CHUNKS, psnr)
    want = oracle_chunks(oracle, est, vol, CHUNKS, rng, psnr)
    check_streams(container, want)
    print(np.dtype(dtype).name, psnr, "bytes", len(container), "q", [w[1] for w in want])
    if psnr == 40.0:   # (a chunk of nothing but zeros is coded, and coded right)
        assert any(w[3] for w in want), [w[3] for w in want]
    ref_vol = oracle.decomp_3d(container, as_float)
    dev = cuda(np.frombuffer(container, dtype=np.uint8))
    got = eng.decompress(dev, output_float=as_float)
    assert np.array_equal(bits(got.cpu().numpy()), bits(ref_vol))
    lo, dims = (5, 20, 30), (40, 30, 9)   # (x, y, z): a box that meets all eight chunks
    box = eng.decompress_box(dev, lo, dims, output_float=as_float).cpu().numpy()
    assert np.array_equal(bits(box), bits(np.ascontiguousarray(ref_vol[30:39, 20:50, 5:45])))
    half = eng.decompress(dev, output_float=as_float, pct=50).cpu().numpy()
    assert np.array_equal(bits(half), bits(oracle.decomp_3d(oracle.trunc_3d(container, 50), as_float)))
    mode2 = eng.compress(cuda(vol), CHUNKS, psnr, mode=2)
    print("mode 2", mode2.numel())
    assert len(container) < mode2.numel()
    if psnr in (60.0, 80.0):   # (the reference's estimate, not a guarantee: 66.93 and 85.99 dB here)
        qual = eng.quality(cuda(vol), got)
        print("psnr of the volume", qual.psnr)
        assert qual.psnr >= psnr


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_plume_as_one_chunk_of_65_strides(eng, oracle, est, dtype):
    vol = plume(dtype)
    container = coded(eng, vol, (64, 64, 64), 60.0)
    check_streams(container, oracle_chunks(oracle, est, vol, (64, 64, 64), pm.value_range(vol), 60.0))
    got = eng.decompress(cuda(np.frombuffer(container, dtype=np.uint8)), output_float=dtype == np.float32).cpu().numpy()
    assert np.array_equal(bits(got), bits(oracle.decomp_3d(container, dtype == np.float32)))


# ---- d. mixed widths, and the refusal -------------------------------------------------------------------------------------

@pytest.mark.parametrize("psnr,widths", [(200.0, [8, 4, 4, 4, 4, 4, 4, 4]), (225.0, [8, 4, 4, 4, 4, 4, 8, 4])])
def test_mixed_coefficient_widths(eng, oracle, est, psnr, widths):
    vol = plume(np.float64)
    want = oracle_chunks(oracle, est, vol, CHUNKS, pm.value_range(vol), psnr)
    assert [w[2] for w in want] == widths   # (the condition)
    container = coded(eng, vol, CHUNKS, psnr)
    check_streams(container, want)
    got = eng.decompress(cuda(np.frombuffer(container, dtype=np.uint8)), output_float=False).cpu().numpy()
    assert np.array_equal(bits(got), bits(oracle.decomp_3d(container, False)))


def test_a_target_beyond_the_coefficients_is_refused(eng):
    import torch
    vol = plume(np.float64)
    d = cuda(vol)
    out = torch.full((eng.max_compressed_size(vol.shape, CHUNKS, 400.0, 2),), 0xA5, dtype=torch.uint8, device="cuda")
    n = C.c_size_t(777)
    rtn = eng.lib.sperrhip_compress_psnr_dev(d.data_ptr(), None, 0, 64, 64, 64, 32, 32, 32, 400.0, 0.0, out.data_ptr(),
                                             out.numel(), C.byref(n), eng._stream())
    assert rtn == -1 and n.value == 777 and bool((out == 0xA5).all())
    # (the engine is fit for the next call)
    assert host(eng.compress_to_psnr(d, CHUNKS, 60.0)) == coded(eng, vol, CHUNKS, 60.0)


# ---- e. a range of the caller's ----------------------------------------------------------------------------------------------

def test_a_given_range(eng, oracle, est):
    vol = plume(np.float32)
    rng = pm.value_range(vol)
    lo, hi = eng.value_range(cuda(vol))
    assert hi - lo == rng
    assert host(eng.compress_to_psnr(cuda(vol), CHUNKS, 60.0, range=rng)) == coded(eng, vol, CHUNKS, 60.0)
    twice = coded(eng, vol, CHUNKS, 60.0, 2.0 * rng)
    check_streams(twice, oracle_chunks(oracle, est, vol, CHUNKS, 2.0 * rng, 60.0))
    assert len(twice) < len(coded(eng, vol, CHUNKS, 60.0))


# ---- f. shapes -------------------------------------------------------------------------------------------------------------

def test_a_ragged_volume_of_two_chunk_shapes(eng, oracle, est):
    vol = np.fromfile(os.path.join(GOLD, "vort_crop.f32"), dtype=np.float32).reshape(33, 36, 40)
    chunks = (20, 18, 16)
    assert len({(b[1], b[3], b[5]) for b in chunk_grid(vol.shape, chunks)}) == 2
    for psnr in (50.0, 80.0):
        container = host(eng.compress_to_psnr(cuda(vol), chunks, psnr))
        check_streams(container, oracle_chunks(oracle, est, vol, chunks, pm.value_range(vol), psnr))
        got = eng.decompress(cuda(np.frombuffer(container, dtype=np.uint8))).cpu().numpy()
        assert np.array_equal(bits(got), bits(oracle.decomp_3d(container, True)))


def test_a_constant_chunk_and_a_constant_volume(eng, oracle, est):
    vol = plume(np.float32, const_chunk=True)
    container = host(eng.compress_to_psnr(cuda(vol), CHUNKS, 60.0))
    want = oracle_chunks(oracle, est, vol, CHUNKS, pm.value_range(vol), 60.0)
    assert [w[1] is None for w in want] == [False] * 7 + [True]
    check_streams(container, want)
    flat = np.full((64, 64, 64), 3.5, dtype=np.float32)
    assert host(eng.compress_to_psnr(cuda(flat), CHUNKS, 60.0)) == oracle.comp_3d(flat, CHUNKS, 2, 60.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_ghost_cell_view_is_the_packed_copy(eng, dtype):
    vol = plume(dtype)
    big = np.zeros((64 + 2, 64 + 4, 64 + 6), dtype=dtype)
    big[:] = 1e6   # (ghost cells that would change the range)
    big[1:65, 2:66, 3:67] = vol
    got = host(eng.compress_to_psnr(cuda(big)[1:65, 2:66, 3:67], CHUNKS, 60.0))
    assert got == coded(eng, vol, CHUNKS, 60.0)


# ---- g. witnesses ---------------------------------------------------------------------------------------------------------------

def count_of(counts, name):
    return sum(n for k, n in counts.items() if name in k)


def launches(eng, call):
    import torch
    eng.profile(True)
    try:
        call()
        torch.cuda.synchronize()
        return {k: n for k, (_, n) in eng.profile_report().items() if n > 0}
    finally:
        eng.profile(False)


def test_the_q_search_is_the_ladder_pair(eng):
    d = cuda(plume(np.float32))
    counts = launches(eng, lambda: eng.compress_to_psnr(d, CHUNKS, 60.0))
    assert count_of(counts, "k_mse_ladder_pick") == 1 and count_of(counts, "k_mse_ladder") == 2, sorted(counts)
    assert count_of(counts, "k_mse_strides") == 0 and count_of(counts, "k_mse_final") == 0 and count_of(counts, "k_vol_range") == 1
    counts = launches(eng, lambda: eng.compress(d, CHUNKS, 60.0, mode=2))
    assert count_of(counts, "k_mse_ladder") == 0 and count_of(counts, "k_vol_range") == 0 and count_of(counts, "k_mse_strides") > 0
    ragged = cuda(np.fromfile(os.path.join(GOLD, "vort_crop.f32"), dtype=np.float32).reshape(33, 36, 40))
    counts = launches(eng, lambda: eng.compress_to_psnr(ragged, (20, 18, 16), 60.0))
    assert count_of(counts, "k_mse_ladder_pick") == 2 and count_of(counts, "k_mse_strides") == 0   # a batch per shape group


# ---- h. a split workspace, a poisoned workspace: in processes of their own --------------------------------------------------

CHILD = r"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from sperr_amd.api import SperrHip
import test_gpu_size as T
eng = SperrHip()
vol = T.plume(np.float32)
d = torch.from_numpy(np.array(vol)).cuda()
eng.profile(True)
c = eng.compress_to_psnr(d, T.CHUNKS, 60.0)
torch.cuda.synchronize()
counts = {k: n for k, (_, n) in eng.profile_report().items() if n > 0}
eng.profile(False)
back = eng.decompress(c).cpu().numpy()
json.dump({"container": bytes(c.cpu().numpy()).hex(), "counts": counts, "back": back.view(np.uint32).tobytes().hex()},
          open(sys.argv[2], "w"))
"""


@pytest.mark.parametrize("env", [{"SPERR_HIP_ARENA_MAX_MB": "1"}, {"SPERR_HIP_POISON": "0xFF"}], ids=["split", "poison"])
def test_children_make_the_same_container(eng, oracle, tmp_path, env):
    vol = plume(np.float32)
    container = coded(eng, vol, CHUNKS, 60.0)
    out = tmp_path / "child.json"
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(ROOT), str(out)], env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = json.load(open(out))
    assert bytes.fromhex(got["container"]) == container
    assert bytes.fromhex(got["back"]) == oracle.decomp_3d(container, True).view(np.uint32).tobytes()
    picks = count_of(got["counts"], "k_mse_ladder_pick")
    print(env, "k_mse_ladder_pick", picks)
    assert picks == (8 if "SPERR_HIP_ARENA_MAX_MB" in env else 1)   # (split: a chunk per batch)
    assert count_of(got["counts"], "k_mse_ladder") == 2 * picks
