"""GPU: the fill kinds of missing values (include/sperr_hip.h SPERRHIP_FILL_*, sperr_amd/csrc/mask_fill.h, mask_fill.hip)
-- the in-filled volume carries the midrange of the valid samples, a value of the caller's, or the smooth pull-push fill.

Every comparison is bit for bit, through integer views; tests/mask_fill_model.py is the numpy statement of the smooth
rule, tests/mask_model.py that of the predicate and the stream.

  smooth       mask_make(fill="smooth") against the model: (z, y, x) in {1x1x1, 2x2x2, 5x3x2, 1x1x70, 70x1x1, 30x44x37,
               70x66x65 -- two levels above k_mask_top's}, seven masks, both rules, fp32 and fp64, out of place and in
               place, a source at the start of its allocation and one element into it; the stream is the midrange call's
  value        mask_make(fill=3.5) and a value that is not a float
  end to end   (30, 44, 37) in 16^3 chunks, modes 1, 2, 3, fp32 and fp64: the container is compress() of the model's
               in-filled volume and the oracle's; the decode whole, as a box and at pct=50; the figures
  refusals     leave every output bitwise as it was
  launches     the counts of the header's formula; no kernel of mask_fill.hip from the other fills or the dense calls"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mask_fill_model as F
import mask_model as M
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = {4: 0x7FC0BEEF, 8: 0x7FF80000DEADBEEF}
_sz = C.c_size_t
THRESHOLD = 1e20
SHAPES = [(1, 1, 1), (2, 2, 2), (5, 3, 2), (1, 1, 70), (70, 1, 1), (30, 44, 37), (70, 66, 65)]      # (z, y, x)
MASKS = ["ball", "slab", "density_0.1", "density_0.9", "single_valid", "all", "none"]
FILL_FAMILY = ["k_mask_pull0", "k_mask_pull", "k_mask_top", "k_mask_push", "k_mask_fill_smooth"]


def _top_cells():
    text = open(os.path.join(ROOT, "sperr_amd", "csrc", "mask_fill.h")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+kMaskTopCells\s*=\s*(\d+)\s*;", text).group(1))


TOP_CELLS = _top_cells()


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    yield e
    e.release()


def _ibits(a):
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_ibits(np.ascontiguousarray(a)),
                                                                        _ibits(np.ascontiguousarray(b)))


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


def make_source(mask, dtype, rule, seed):
    """a smooth field with noise; NaNs of several payloads at the missing samples, and under the threshold rule also the
    infinities and +-1e20"""
    shape = mask.shape
    z, y, x = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in shape), indexing="ij")
    rng = np.random.default_rng(seed)
    a = (280.0 + 9.0 * np.sin(0.21 * x + 0.4) * np.cos(0.17 * y) + 0.3 * z + 0.05 * rng.standard_normal(shape)).astype(dtype)
    if np.dtype(dtype).itemsize == 4:
        pool = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    else:
        pool = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001,
                         0x7FFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
    if rule == M.RULE_ABS_GE:
        pool = np.concatenate([pool, np.array([np.inf, -np.inf, 1e20, -1e20, 3e25], dtype=dtype)])
    a[mask] = pool[(np.arange(int(mask.sum())) + seed) % pool.size]
    assert np.array_equal(M.missing(a, rule, THRESHOLD), mask)
    return a


def dev_at(a, lead):
    """the array on the device, its first element `lead` elements into an allocation"""
    import torch
    buf = torch.zeros(a.size + lead, dtype=torch.from_numpy(a).dtype, device="cuda")
    buf[lead:] = torch.from_numpy(a).cuda().reshape(-1)
    return buf[lead:].view(a.shape)


def sentinel_like(shape, dtype):
    import torch
    esz = np.dtype(dtype).itemsize
    p = torch.full(tuple(shape), SENTINEL[esz], dtype=torch.int32 if esz == 4 else torch.int64, device="cuda")
    return p.view(torch.float32 if esz == 4 else torch.float64)


def to_dev(container):
    import torch
    return torch.from_numpy(np.frombuffer(container, dtype=np.uint8).copy()).cuda()


# ---- the smooth fill against the model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_make_smooth_equals_the_model(eng, shape, name):
    k = SHAPES.index(shape) * len(MASKS) + MASKS.index(name)
    mask = make_mask(name, shape)
    want_stream = M.stream(mask)
    for j, (dtype, rule) in enumerate([(np.float32, M.RULE_NAN), (np.float64, M.RULE_ABS_GE), (np.float32, M.RULE_ABS_GE),
                                       (np.float64, M.RULE_NAN)]):
        lead = (k + j // 2) % 2     # a source at the start of its allocation and one element into it
        a = make_source(mask, dtype, rule, k)
        want = F.smooth_filled(a, mask)
        assert want is not None and same_bits(want[~mask], a[~mask])
        missing = "nan" if rule == M.RULE_NAN else THRESHOLD
        src = dev_at(a, lead)
        filled = dev_at(np.zeros_like(a), lead)
        stream, nmiss = eng.mask_make(src, missing, filled_out=filled, fill="smooth")
        assert nmiss == int(mask.sum())
        assert bytes(stream.cpu().numpy()) == want_stream
        got = filled.cpu().numpy()
        assert same_bits(got, want), (dtype, rule, lead, int((_ibits(got) != _ibits(want)).sum()))
        assert same_bits(src.cpu().numpy(), a), "the source was written"
        mid, _ = eng.mask_make(src, missing, fill="midrange")
        assert bytes(mid.cpu().numpy()) == want_stream
        # in place
        again, _ = eng.mask_make(src, missing, filled_out=src, fill="smooth")
        assert bytes(again.cpu().numpy()) == want_stream and same_bits(src.cpu().numpy(), want)


def test_fewer_dimensions_lead_with_ones(eng):
    mask = make_mask("density_0.1", (1, 9, 70))
    a = make_source(mask, np.float32, M.RULE_NAN, 5)
    want = F.smooth_filled(a, mask)
    for shape in ((9, 70), (1, 9, 70)):
        filled = dev_at(np.zeros(shape, dtype=np.float32), 0)
        eng.mask_make(dev_at(a.reshape(shape), 0), filled_out=filled, fill="smooth")
        assert same_bits(filled.cpu().numpy().reshape(a.shape), want)
    line = a.reshape(-1)
    filled = dev_at(np.zeros_like(line), 0)
    eng.mask_make(dev_at(line, 0), filled_out=filled, fill="smooth")
    assert same_bits(filled.cpu().numpy(), F.smooth_filled(line, mask.reshape(-1)))


# ---- a value of the caller's -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("lead", [0, 1])
def test_mask_make_with_a_value_is_the_models_where(eng, dtype, lead):
    shape = (30, 44, 37)
    mask = make_mask("ball", shape)
    a = make_source(mask, dtype, M.RULE_NAN, 9)
    for value in (3.5, 0.1, -0.0):          # (0.1 is no float: narrowed once for fp32 data)
        src = dev_at(a, lead)
        filled = dev_at(np.zeros_like(a), lead)
        stream, nmiss = eng.mask_make(src, "nan", filled_out=filled, fill=value)
        want = np.where(mask, np.dtype(dtype).type(value), a)
        assert same_bits(want, F.value_filled(a, mask, value))
        assert nmiss == int(mask.sum()) and bytes(stream.cpu().numpy()) == M.stream(mask)
        assert same_bits(filled.cpu().numpy(), want)
        eng.mask_make(src, "nan", filled_out=src, fill=value)
        assert same_bits(src.cpu().numpy(), want)
    # a 4-D tensor is fine for a value and for the midrange
    four = dev_at(a.reshape(2, 15, 44, 37), 0)
    eng.mask_make(four, "nan", filled_out=four, fill=3.5)
    assert same_bits(four.cpu().numpy().reshape(shape), np.where(mask, np.dtype(dtype).type(3.5), a))


# ---- end to end --------------------------------------------------------------------------------------------------------
VOL_ZYX = (30, 44, 37)
CHUNKS = (16, 16, 16)
QUALITY = {1: 2.5, 2: 70.0, 3: 1e-3}
BOX_LO, BOX_DIMS = (20, 9, 7), (15, 30, 20)        # (x, y, z)
VALUE_FILL = 3.5


@pytest.fixture(scope="module")
def volumes():
    """{dtype name: (masked volume, bool mask, {fill: the model's in-filled volume})}"""
    t = turbulence(VOL_ZYX, dtype=np.float64)
    mask = M.ball_mask(VOL_ZYX, 12)
    out = {}
    for dt in ("float32", "float64"):
        v = t.astype(dt)
        v[mask] = np.nan
        out[dt] = (v, mask, {"smooth": F.smooth_filled(v, mask), VALUE_FILL: F.value_filled(v, mask, VALUE_FILL)})
    return out


@pytest.fixture(scope="module")
def oracle_containers(oracle, volumes):
    out = {(dt, mode, "smooth"): oracle.comp_3d(fills["smooth"], CHUNKS, mode, q)
           for dt, (_, _, fills) in volumes.items() for mode, q in QUALITY.items()}
    out[("float32", 1, VALUE_FILL)] = oracle.comp_3d(volumes["float32"][2][VALUE_FILL], CHUNKS, 1, QUALITY[1])
    return out


def check_end_to_end(eng, oracle, volumes, oracle_containers, dt, mode, fill):
    import torch
    v, mask, fills = volumes[dt]
    dv = torch.from_numpy(v).cuda()
    container, stream = eng.compress_masked(dv, CHUNKS, QUALITY[mode], mode=mode, fill=fill)
    want = oracle_containers[(dt, mode, fill)]
    assert bytes(stream.cpu().numpy()) == M.stream(mask)
    assert bytes(container.cpu().numpy()) == want, "the container differs from the oracle's"
    assert same_bits(dv.cpu().numpy(), v), "the source was written"
    dense = eng.compress(torch.from_numpy(fills[fill]).cuda(), CHUNKS, QUALITY[mode], mode=mode)
    assert bytes(dense.cpu().numpy()) == want
    of = dt == "float32"
    whole = oracle.decomp_3d(want, of)
    half = oracle.decomp_3d(oracle.trunc_3d(want, 50), of)
    (lx, ly, lz), (bx, by, bz) = BOX_LO, BOX_DIMS
    box = (slice(lz, lz + bz), slice(ly, ly + by), slice(lx, lx + bx))
    for value in (float("nan"), 1e20):
        ref = whole.copy()
        ref[mask] = whole.dtype.type(value)
        got = eng.decompress_masked(container, stream, value, output_float=of)
        assert same_bits(got.cpu().numpy(), ref)
        got = eng.decompress_masked(container, stream, value, BOX_LO, BOX_DIMS, output_float=of)
        assert same_bits(got.cpu().numpy(), np.ascontiguousarray(ref[box]))
        ref = half.copy()
        ref[mask] = half.dtype.type(value)
        got = eng.decompress_masked(container, stream, value, pct=50, output_float=of)
        assert same_bits(got.cpu().numpy(), ref)
    recon = eng.decompress_masked(container, stream, float("nan"), output_float=of)
    keep = torch.from_numpy(~mask).cuda()
    q, ref_q = eng.quality_masked(dv, recon, stream), eng.quality(dv[keep].contiguous(), recon[keep].contiguous())
    fig = lambda f: np.array([f.rmse, f.linfty, f.psnr, f.min, f.max, f.mean, f.var, f.mse]).view(np.uint64)
    assert np.array_equal(fig(q), fig(ref_q)), (q, ref_q)
    assert np.isfinite([q.rmse, q.linfty, q.psnr, q.mean, q.var]).all() and q.rmse > 0


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_compress_masked_smooth_end_to_end(eng, oracle, volumes, oracle_containers, dt, mode):
    check_end_to_end(eng, oracle, volumes, oracle_containers, dt, mode, "smooth")


def test_compress_masked_with_a_value_end_to_end(eng, oracle, volumes, oracle_containers):
    check_end_to_end(eng, oracle, volumes, oracle_containers, "float32", 1, VALUE_FILL)


def test_smooth_container_is_smaller_on_the_device_too(eng, volumes):
    """(the CPU test asserts it with the oracle; this is the same claim through the device calls)"""
    import torch
    v, _, _ = volumes["float32"]
    dv = torch.from_numpy(v).cuda()
    a, _ = eng.compress_masked(dv, CHUNKS, QUALITY[3], mode=3)
    b, _ = eng.compress_masked(dv, CHUNKS, QUALITY[3], mode=3, fill="smooth")
    print(f"mode 3 tolerance {QUALITY[3]}: midrange {a.numel()} bytes, smooth {b.numel()} bytes")
    assert b.numel() < a.numel()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_default_fill_is_the_midrange(eng, oracle, volumes, mode):
    import torch
    v, mask, _ = volumes["float32"]
    dv = torch.from_numpy(v).cuda()
    a, sa = eng.compress_masked(dv, CHUNKS, QUALITY[mode], mode=mode)
    b, sb = eng.compress_masked(dv, CHUNKS, QUALITY[mode], mode=mode, fill="midrange")
    assert bytes(a.cpu().numpy()) == bytes(b.cpu().numpy()) and bytes(sa.cpu().numpy()) == bytes(sb.cpu().numpy())
    assert bytes(a.cpu().numpy()) == oracle.comp_3d(M.filled(v, mask), CHUNKS, mode, QUALITY[mode])
    # ... and through the C call with the kind spelled out
    cap = eng.max_compressed_size(VOL_ZYX, CHUNKS, QUALITY[mode], mode)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    buf = torch.zeros(eng.mask_max_size(v.size), dtype=torch.uint8, device="cuda")
    dlen, mlen, nmiss = _sz(0), _sz(0), _sz(0)
    rtn = eng.lib.sperrhip_compress_masked_fill_dev(dv.data_ptr(), 1, VOL_ZYX[2], VOL_ZYX[1], VOL_ZYX[0], *CHUNKS, mode,
                                                    QUALITY[mode], M.RULE_NAN, 0.0, F.FILL_MIDRANGE, float("nan"),
                                                    dst.data_ptr(), cap, C.byref(dlen), buf.data_ptr(), buf.numel(),
                                                    C.byref(mlen), C.byref(nmiss), None)
    torch.cuda.synchronize()
    assert rtn == 0 and bytes(dst[:dlen.value].cpu().numpy()) == bytes(a.cpu().numpy())
    assert bytes(buf[:mlen.value].cpu().numpy()) == M.stream(mask) and nmiss.value == int(mask.sum())


# ---- refusals ----------------------------------------------------------------------------------------------------------
def make_vol_call(eng, src, shape, fill, value, filled, mask, cap=None, rule=M.RULE_NAN):
    import torch
    mlen, nmiss = _sz(77), _sz(78)
    dz, dy, dx = shape
    rtn = eng.lib.sperrhip_mask_make_vol_dev(src.data_ptr(), int(src.dtype == torch.float32), dx, dy, dz, rule, 0.0, fill,
                                             value, None if filled is None else filled.data_ptr(), mask.data_ptr(),
                                             mask.numel() if cap is None else cap, C.byref(mlen), C.byref(nmiss), None)
    torch.cuda.synchronize()
    return rtn, mlen.value, nmiss.value


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refusals_write_nothing(eng, dtype):
    import torch
    from sperr_amd.api import SperrHipError
    shape = (30, 44, 37)
    bits = make_mask("ball", shape)
    a = make_source(bits, dtype, M.RULE_NAN, 4)
    src = dev_at(a, 0)
    filled = sentinel_like(shape, dtype)
    keep = sentinel_like(shape, dtype).cpu().numpy()
    mask = torch.full((eng.mask_max_size(a.size),), 0xA5, dtype=torch.uint8, device="cuda")

    def untouched():
        return bool((mask == 0xA5).all()) and same_bits(filled.cpu().numpy(), keep)

    # an unknown kind; a value that is not finite; for fp32 data one that is not finite as a float
    bad = [(3, 0.0), (-1, 0.0), (F.FILL_VALUE, float("nan")), (F.FILL_VALUE, float("inf")), (F.FILL_VALUE, float("-inf"))]
    if dtype == np.float32:
        bad.append((F.FILL_VALUE, 1e39))
    for kind, value in bad:
        assert make_vol_call(eng, src, shape, kind, value, filled, mask) == (-1, 77, 78), (kind, value)
        assert untouched(), (kind, value)
    if dtype == np.float64:
        assert make_vol_call(eng, src, shape, F.FILL_VALUE, 1e39, filled, mask)[0] == 0
        filled.copy_(sentinel_like(shape, dtype))
        mask.fill_(0xA5)
    for value in (float("nan"), float("inf"), 1e39 if dtype == np.float32 else float("-inf")):
        with pytest.raises(SperrHipError):
            eng.mask_make(src, filled_out=filled, fill=value)
        with pytest.raises(SperrHipError):
            eng.compress_masked(src, CHUNKS, 2.5, fill=value)
    with pytest.raises(ValueError):
        eng.mask_make(src, filled_out=filled, fill="plateau")
    # more than three dimensions with the smooth fill
    with pytest.raises(SperrHipError):
        eng.mask_make(src.view(2, 15, 44, 37), filled_out=filled, fill="smooth")
    assert untouched()
    # a capacity one byte short: 1, the size, and nothing written -- for every kind
    need = len(M.stream(bits))
    for kind in (F.FILL_MIDRANGE, F.FILL_VALUE, F.FILL_SMOOTH):
        assert make_vol_call(eng, src, shape, kind, 3.5, filled, mask, cap=need - 1) == (1, need, 78), kind
        assert untouched(), kind
    rtn, mlen, nmiss = make_vol_call(eng, src, shape, F.FILL_SMOOTH, 0.0, filled, mask, cap=need)
    assert (rtn, mlen, nmiss) == (0, need, int(bits.sum())) and bytes(mask[:need].cpu().numpy()) == M.stream(bits)
    assert bool((mask[need:] == 0xA5).all()) and same_bits(filled.cpu().numpy(), F.smooth_filled(a, bits))


def test_a_sum_that_is_not_finite_fails_and_writes_nothing(eng):
    import torch
    shape = (30, 44, 37)
    bits = make_mask("ball", shape)
    a = make_source(bits, np.float64, M.RULE_NAN, 6)
    assert not bits[3, 4, 6] and not bits[3, 4, 7]
    a[3, 4, 6] = a[3, 4, 7] = 1.7e308           # two children of one cell of level 1
    assert F.smooth_filled(a, bits) is None
    src = dev_at(a, 0)
    filled = sentinel_like(shape, np.float64)
    mask = torch.full((eng.mask_max_size(a.size),), 0xA5, dtype=torch.uint8, device="cuda")
    assert make_vol_call(eng, src, shape, F.FILL_SMOOTH, 0.0, filled, mask) == (-1, 77, 78)
    assert bool((mask == 0xA5).all())
    assert same_bits(filled.cpu().numpy(), sentinel_like(shape, np.float64).cpu().numpy())
    assert same_bits(src.cpu().numpy(), a)
    # The only two valid samples, far apart: each is the one known child of its cells, so its value climbs unchanged
    # until the two meet -- in the LDS levels of k_mask_top here, and for 70 x 66 x 65 with neighbouring cells of
    # level 1 in k_mask_pull: the same refusal from each of the three kernels that sum
    for shp, second in (((30, 44, 37), (20, 40, 30)), ((70, 66, 65), (0, 0, 2))):
        b = np.full(shp, np.nan, dtype=np.float64)
        b[0, 0, 0] = b[second] = 1.7e308
        assert F.smooth_filled(b, np.isnan(b)) is None
        out = sentinel_like(shp, np.float64)
        buf = torch.full((eng.mask_max_size(b.size),), 0xA5, dtype=torch.uint8, device="cuda")
        assert make_vol_call(eng, dev_at(b, 0), shp, F.FILL_SMOOTH, 0.0, out, buf) == (-1, 77, 78), shp
        assert bool((buf == 0xA5).all()) and same_bits(out.cpu().numpy(), sentinel_like(shp, np.float64).cpu().numpy())
        b[second] = -1.5                          # ... and with one of them small the call succeeds
        assert make_vol_call(eng, dev_at(b, 0), shp, F.FILL_SMOOTH, 0.0, out, buf)[0] == 0
        assert same_bits(out.cpu().numpy(), F.smooth_filled(b, np.isnan(b)))
    # the midrange of the same samples is finite (the halves are taken first), and so is a caller's value
    assert make_vol_call(eng, src, shape, F.FILL_MIDRANGE, 0.0, filled, mask)[0] == 0
    assert same_bits(filled.cpu().numpy(), M.filled(a, bits))
    # an infinity that the NaN rule calls valid: the smooth rule refuses it as the midrange does, a value does not
    c = make_source(bits, np.float64, M.RULE_NAN, 6)
    c[3, 4, 6] = np.inf
    assert F.smooth_filled(c, bits) is None and M.fill_value(c, bits) is None
    assert make_vol_call(eng, dev_at(c, 0), shape, F.FILL_SMOOTH, 0.0, filled, mask)[0] == -1
    assert make_vol_call(eng, dev_at(c, 0), shape, F.FILL_MIDRANGE, 0.0, filled, mask)[0] == -1
    assert make_vol_call(eng, dev_at(c, 0), shape, F.FILL_VALUE, 3.5, filled, mask)[0] == 0
    assert same_bits(filled.cpu().numpy(), F.value_filled(c, bits, 3.5))


# ---- launch tables -----------------------------------------------------------------------------------------------------
def launched(eng, fn):
    """(what fn returns, {kernel name: launches})"""
    import torch
    torch.cuda.synchronize()
    eng.profile(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {k: n for k, (_, n) in eng.profile_report().items() if n > 0}
    finally:
        eng.profile(False)


def _name(k):
    """the kernel's name without template arguments, brackets or a namespace"""
    return re.split(r"[<(\s]", k.strip("() "))[0].split("::")[-1]


def _count(table, name):
    return sum(n for k, n in table.items() if _name(k) == name)


@pytest.mark.parametrize("shape", [(30, 44, 37), (70, 66, 65)], ids=lambda s: "x".join(map(str, s)))
def test_smooth_fill_launches_the_formulas_counts(eng, shape):
    want = F.launches(shape, TOP_CELLS)
    if shape == (30, 44, 37):
        assert want["k_mask_pull"] == 0 and want["k_mask_push"] == 0
    else:
        assert want["k_mask_pull"] == 1 and want["k_mask_push"] == 1, "two levels above k_mask_top's"
    mask = make_mask("ball", shape)
    a = make_source(mask, np.float32, M.RULE_NAN, 2)
    src, filled = dev_at(a, 0), dev_at(np.zeros_like(a), 0)
    _, table = launched(eng, lambda: eng.mask_make(src, filled_out=filled, fill="smooth"))
    assert {k: _count(table, k) for k in FILL_FAMILY} == want, table
    assert [_count(table, k) for k in ("k_mask_survey", "k_mask_finish", "k_mask_pack", "k_mask_fill")] == [1, 1, 1, 0], table
    assert same_bits(filled.cpu().numpy(), F.smooth_filled(a, mask))
    _, table = launched(eng, lambda: eng.compress_masked(src, (32, 32, 32), 2.5, fill="smooth"))
    assert {k: _count(table, k) for k in FILL_FAMILY} == want, table
    assert [_count(table, k) for k in ("k_mask_survey", "k_mask_finish", "k_mask_pack", "k_mask_fill")] == [1, 1, 1, 0], table


def test_other_fills_and_dense_calls_launch_no_kernel_of_the_smooth_fill(eng, volumes):
    import torch
    v, mask, fills = volumes["float32"]
    dv, df = torch.from_numpy(v).cuda(), torch.from_numpy(fills["smooth"]).cuda()
    filled = torch.zeros_like(dv)
    none = lambda table: table and all(_count(table, k) == 0 for k in FILL_FAMILY)
    for fill in ("midrange", VALUE_FILL):
        _, table = launched(eng, lambda: eng.mask_make(dv, filled_out=filled, fill=fill))
        assert none(table) and _count(table, "k_mask_fill") == 1, table
        (container, stream), table = launched(eng, lambda: eng.compress_masked(dv, CHUNKS, 2.5, fill=fill))
        assert none(table) and _count(table, "k_mask_fill") == 1, table
    _, table = launched(eng, lambda: eng.decompress_masked(container, stream, 0.0))
    assert none(table), table
    dense, table = launched(eng, lambda: eng.compress(df, CHUNKS, 2.5))
    assert none(table), table
    _, table = launched(eng, lambda: eng.decompress(dense))
    assert none(table), table
    _, table = launched(eng, lambda: eng.decompress_box(dense, BOX_LO, BOX_DIMS))
    assert none(table), table
