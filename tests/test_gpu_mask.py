"""GPU: missing values (include/sperr_hip.h "masked volumes", sperr_amd/csrc/mask.h, mask.hip) -- a volume with NaNs or
a sentinel becomes an ordinary container of the in-filled volume and a mask stream, and the decode puts a value of the
caller's back at the missing samples.

Every comparison is bit for bit, through integer views; tests/mask_model.py is the numpy statement of the rules.

  kernels      mask_make (stream, count, in-filled samples), mask_bits and mask_apply against the model: n in
               {1, 63, 64, 65, T - 1, T, T + 1, 3T + 5} with T the tile constant parsed from mask.h, seven masks, both
               rules, fp32 and fp64, a source at the start of its allocation (the 16-byte form) and one element into it
               (the element form); NaNs of different payloads, both infinities and 1e20 as the missing samples
  end to end   (30, 44, 37) in (32, 32, 32) chunks -- remainder chunks, k_lis_mx -- of turbulence with a ball of NaNs and
               with the slab x >= 30 of 9.96921e36: containers against the oracle's of the model's in-filled volume in
               modes 1, 2 and 3, fp32 and fp64; the decode whole, as a box and at pct=30; the figures
  refusals     leave every output bitwise as it was
  launches     the dense calls launch no kernel of mask.hip, compress_masked launches survey, finish, pack and fill once"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mask_model as M
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = {4: 0x7FC0BEEF, 8: 0x7FF80000DEADBEEF}
_sz = C.c_size_t


def _const(name):
    text = open(os.path.join(ROOT, "sperr_amd", "csrc", "mask.h")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)\s*;", text).group(1))


T = _const("kMaskTile")
SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]
MASKS = ["none", "all", "last", "tile_edge", "alternating", "density", "runs"]
THRESHOLD = 1e20


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


def make_mask(kind, n, seed=0):
    m = np.zeros(n, dtype=bool)
    if kind == "all":
        m[:] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "tile_edge":
        # a run that ends on a tile's last sample and one that starts on the next tile's first: no toggle between them
        if n > T:
            m[max(0, T - 5):min(n, T + 7)] = True
        else:
            m[n // 2:] = True
    elif kind == "alternating":
        m[1:min(n, 64):2] = True
    elif kind == "density":
        m = np.random.default_rng(1000 + n + seed).random(n) < 0.1
    elif kind == "runs":
        m[np.arange(n) // 61 % 2 == 1] = True
    return m


def missing_values(dtype, rule, count, seed):
    """what stands at the missing samples: NaNs of different payloads, and under rule 2 also the infinities and +-1e20"""
    u = np.dtype(dtype).itemsize
    if u == 4:
        nans = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFFC12345], dtype=np.uint32)
    else:
        nans = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001,
                         0x7FFFFFFFFFFFFFFF, 0xFFF8000012345678], dtype=np.uint64)
    pool = nans.view(dtype)
    if rule == M.RULE_ABS_GE:
        pool = np.concatenate([pool, np.array([np.inf, -np.inf, 1e20, -1e20, 3e25], dtype=dtype)])
    return pool[(np.arange(count) + seed) % pool.size]


def make_source(mask, dtype, rule, seed):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(mask.size) * 50.0).astype(dtype)
    a[mask] = missing_values(dtype, rule, int(mask.sum()), seed)
    assert np.array_equal(M.missing(a, rule, THRESHOLD), mask)
    return a


def dev_at(a, lead):
    """the array on the device, its first element `lead` elements into an allocation"""
    import torch
    buf = torch.zeros(a.size + lead, dtype=torch.from_numpy(a).dtype, device="cuda")
    buf[lead:] = torch.from_numpy(a).cuda()
    return buf[lead:]


def sentinel_like(shape, dtype):
    import torch
    tdt = torch.float32 if np.dtype(dtype).itemsize == 4 else torch.float64
    esz = np.dtype(dtype).itemsize
    p = torch.full(tuple(shape), SENTINEL[esz], dtype=torch.int32 if esz == 4 else torch.int64, device="cuda")
    return p.view(tdt)


def check_make_bits_apply(eng, a, mask, rule, lead):
    import torch
    src = dev_at(a, lead)
    missing = "nan" if rule == M.RULE_NAN else THRESHOLD
    filled = dev_at(np.zeros_like(a), lead)
    stream, nmiss = eng.mask_make(src, missing, filled_out=filled)
    want = M.stream(mask)
    assert nmiss == int(mask.sum())
    assert bytes(stream.cpu().numpy()) == want
    assert same_bits(filled.cpu().numpy(), M.filled(a, mask))
    assert same_bits(src.cpu().numpy(), a), "the source was written"
    # in place
    again, _ = eng.mask_make(src, missing, filled_out=src)
    assert bytes(again.cpu().numpy()) == want and same_bits(src.cpu().numpy(), M.filled(a, mask))
    assert eng.mask_parse(stream) == (a.size, int(mask.sum()), M.parse(want)[0])
    assert np.array_equal(eng.mask_bits(stream).cpu().numpy(), mask)
    # apply: every other sample keeps the sentinel
    for value in (float("nan"), 1e20):
        dst = sentinel_like((a.size,), a.dtype)
        eng.mask_apply(dst, stream, value)
        ref = sentinel_like((a.size,), a.dtype).cpu().numpy()
        ref[mask] = a.dtype.type(value)
        assert same_bits(dst.cpu().numpy(), ref)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", SIZES)
def test_mask_make_bits_and_apply_equal_the_model(eng, n, kind):
    k = SIZES.index(n) * len(MASKS) + MASKS.index(kind)
    mask = make_mask(kind, n)
    for j, (dtype, rule) in enumerate([(np.float32, M.RULE_NAN), (np.float64, M.RULE_ABS_GE), (np.float32, M.RULE_ABS_GE),
                                       (np.float64, M.RULE_NAN)]):
        lead = (k + j // 2) % 2     # both forms for every (dtype, rule) over the cases
        check_make_bits_apply(eng, make_source(mask, dtype, rule, k), mask, rule, lead)


BIG = 12 * 1000 * 1000 + 5      # 11719 tiles: more than any grid holds (8192), more than one round of the tile scan (8192)


@pytest.mark.parametrize("kind,lead", [("runs", 0), ("density", 1)])
def test_more_tiles_than_the_grid_and_than_one_round_of_the_tile_scan(eng, kind, lead):
    """a fault of the tile walk or of the scan's second round can show only at such a size: toggles ("runs", the
    16-byte form) and bits ("density", the element form); make, bits, apply and the compaction against the model"""
    import torch
    assert BIG // T > 8192
    mask = make_mask(kind, BIG)
    a = make_source(mask, np.float32, M.RULE_NAN, 11)
    want = M.stream(mask)
    assert M.parse(want)[0] == (M.KIND_TOGGLES if kind == "runs" else M.KIND_BITS)
    src = dev_at(a, lead)
    filled = dev_at(np.zeros_like(a), lead)
    stream, nmiss = eng.mask_make(src, "nan", filled_out=filled)
    assert nmiss == int(mask.sum()) and bytes(stream.cpu().numpy()) == want
    assert same_bits(filled.cpu().numpy(), M.filled(a, mask))
    assert np.array_equal(eng.mask_bits(stream).cpu().numpy(), mask)
    dst = sentinel_like((BIG,), np.float32)
    eng.mask_apply(dst, stream, 1e20)
    ref = sentinel_like((BIG,), np.float32).cpu().numpy()
    ref[mask] = np.float32(1e20)
    assert same_bits(dst.cpu().numpy(), ref)
    # the compaction: the figures of the valid samples against a shifted copy
    recon = torch.where(torch.isnan(src), src, src + 0.25)
    keep = torch.from_numpy(~mask).cuda()
    got, ref_q = eng.quality_masked(src, recon, stream), eng.quality(src[keep].contiguous(), recon[keep].contiguous())
    fig = lambda q: np.array([q.rmse, q.linfty, q.psnr, q.min, q.max, q.mean, q.var, q.mse]).view(np.uint64)
    assert np.array_equal(fig(got), fig(ref_q)), (got, ref_q)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_kind_rule_boundary_fifteen_and_sixteen_toggles(eng, dtype, lead):
    for nt, kind, nbytes in ((15, M.KIND_TOGGLES, 92), (16, M.KIND_BITS, 96)):
        mask = np.zeros(512, dtype=bool)
        for i in range(nt):
            mask[3 * i + 1:] ^= True
        a = make_source(mask, dtype, M.RULE_NAN, nt)
        stream, _ = eng.mask_make(dev_at(a, lead))
        assert stream.numel() == nbytes and M.parse(bytes(stream.cpu().numpy()))[0] == kind
        check_make_bits_apply(eng, a, mask, M.RULE_NAN, lead)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_signed_zeros_as_the_extremes_give_one_fill(eng, dtype):
    fills = []
    for order in ((-0.0, 0.0), (0.0, -0.0)):
        a = np.full(3 * T + 5, np.nan, dtype=dtype)
        a[7], a[2 * T + 3] = order
        mask = np.isnan(a)
        filled = dev_at(np.zeros_like(a), 0)
        stream, nmiss = eng.mask_make(dev_at(a, 0), "nan", filled_out=filled)
        assert nmiss == a.size - 2 and bytes(stream.cpu().numpy()) == M.stream(mask)
        got = filled.cpu().numpy()
        assert same_bits(got, M.filled(a, mask))
        fills.append(_ibits(got)[0])
    assert fills[0] == fills[1] == 0     # 0.5 * -0.0 + 0.5 * +0.0 = +0.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_valid_sample_fills_with_zero(eng, dtype):
    a = np.full(T + 9, np.nan, dtype=dtype)
    filled = dev_at(np.ones_like(a), 1)
    stream, nmiss = eng.mask_make(dev_at(a, 1), "nan", filled_out=filled)
    assert nmiss == a.size and bytes(stream.cpu().numpy()) == M.stream(np.ones(a.size, dtype=bool))
    assert not _ibits(filled.cpu().numpy()).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("bad", [np.inf, -np.inf])
def test_an_infinity_under_the_nan_rule_fails_and_writes_nothing(eng, dtype, bad):
    import torch
    a = make_source(make_mask("density", 2 * T + 1), dtype, M.RULE_NAN, 3)
    a[T + 3] = bad
    assert M.fill_value(a, np.isnan(a)) is None
    src = dev_at(a, 0)
    filled = sentinel_like((a.size,), dtype)
    mask = torch.full((eng.mask_max_size(a.size),), 0xA5, dtype=torch.uint8, device="cuda")
    mlen, nmiss = _sz(77), _sz(78)
    rtn = eng.lib.sperrhip_mask_make_dev(src.data_ptr(), int(dtype == np.float32), a.size, M.RULE_NAN, 0.0,
                                         filled.data_ptr(), mask.data_ptr(), mask.numel(), C.byref(mlen),
                                         C.byref(nmiss), None)
    torch.cuda.synchronize()
    assert rtn == -1 and (mlen.value, nmiss.value) == (77, 78)
    assert bool((mask == 0xA5).all()) and same_bits(filled.cpu().numpy(), sentinel_like((a.size,), dtype).cpu().numpy())
    # the same samples under the other rule: the infinity is missing, the call succeeds
    stream, n2 = eng.mask_make(src, THRESHOLD)
    assert n2 == int(np.isnan(a).sum()) + 1


def test_bad_arguments_of_mask_make_are_refused(eng):
    import torch
    src = torch.zeros(100, dtype=torch.float32, device="cuda")
    mask = torch.full((eng.mask_max_size(100),), 0xA5, dtype=torch.uint8, device="cuda")
    mlen, nmiss = _sz(0), _sz(0)

    def call(p=src.data_ptr(), n=100, rule=1, thr=0.0, m=mask.data_ptr()):
        return eng.lib.sperrhip_mask_make_dev(p, 1, n, rule, thr, None, m, mask.numel(), C.byref(mlen), C.byref(nmiss),
                                              None)
    assert call() == 0
    mask.fill_(0xA5)
    for kw in (dict(p=None), dict(n=0), dict(rule=0), dict(rule=3), dict(rule=2, thr=0.0), dict(rule=2, thr=-1.0),
               dict(rule=2, thr=float("inf")), dict(rule=2, thr=float("nan")), dict(m=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((mask == 0xA5).all())


# ---- a box of a volume -----------------------------------------------------------------------------------------------
VOL_ZYX = (30, 44, 37)
BOX_LO, BOX_DIMS = (20, 9, 7), (15, 30, 20)        # (x, y, z), of the end-to-end volume: four chunks
APPLY_ZYX = (37, 44, 30)                           # mask_apply alone: another volume, a box that ends on its last slice
APPLY_LO, APPLY_DIMS = (3, 5, 7), (20, 9, 30)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("which", ["ball", "slab"])
def test_mask_apply_on_a_box_with_both_kinds_of_stream(eng, which, dtype):
    mask = M.ball_mask(APPLY_ZYX, 12) if which == "ball" else M.slab_mask(APPLY_ZYX, 20)
    a = make_source(mask.reshape(-1), dtype, M.RULE_NAN, 5)
    stream, _ = eng.mask_make(dev_at(a, 0))
    assert M.parse(bytes(stream.cpu().numpy()))[0] == (M.KIND_TOGGLES if which == "ball" else M.KIND_BITS)
    (lx, ly, lz), (bx, by, bz) = APPLY_LO, APPLY_DIMS
    sub = mask[lz:lz + bz, ly:ly + by, lx:lx + bx]
    assert sub.any() and not sub.all()
    for value in (float("nan"), 1e20):
        dst = sentinel_like((bz, by, bx), dtype)
        eng.mask_apply(dst, stream, value, APPLY_LO, APPLY_DIMS, vol_shape_zyx=APPLY_ZYX)
        ref = sentinel_like((bz, by, bx), dtype).cpu().numpy()
        ref[sub] = np.dtype(dtype).type(value)
        assert same_bits(dst.cpu().numpy(), ref)
    # a box that leaves the volume, and a volume that is not the stream's
    from sperr_amd.api import SperrHipError
    dst = sentinel_like((bz, by, bx), dtype)
    with pytest.raises(SperrHipError):
        eng.mask_apply(dst, stream, 0.0, (11, 5, 7), APPLY_DIMS, vol_shape_zyx=APPLY_ZYX)
    with pytest.raises(SperrHipError):
        eng.mask_apply(dst, stream, 0.0, APPLY_LO, APPLY_DIMS, vol_shape_zyx=(37, 44, 31))
    assert same_bits(dst.cpu().numpy(), sentinel_like((bz, by, bx), dtype).cpu().numpy())


# ---- end to end ------------------------------------------------------------------------------------------------------
CHUNKS = (32, 32, 32)
QUALITY = {1: 2.5, 2: 70.0, 3: 1e-3}
SENT = 9.96921e36
CASES = {"ball": ("nan", M.RULE_NAN, 0.0), "slab": (1e30, M.RULE_ABS_GE, 1e30)}


def to_dev(container):
    import torch
    return torch.from_numpy(np.frombuffer(container, dtype=np.uint8).copy()).cuda()


@pytest.fixture(scope="module")
def volumes():
    """{(case, dtype name): (masked volume, bool mask, the model's in-filled volume)}"""
    t = turbulence(VOL_ZYX, dtype=np.float64)
    out = {}
    for case in CASES:
        mask = M.ball_mask(VOL_ZYX, 12) if case == "ball" else M.slab_mask(VOL_ZYX, 30)
        for dt in ("float32", "float64"):
            v = t.astype(dt)
            v[mask] = np.nan if case == "ball" else np.dtype(dt).type(SENT)
            assert np.array_equal(M.missing(v, CASES[case][1], CASES[case][2]), mask)
            out[(case, dt)] = (v, mask, M.filled(v, mask))
    return out


@pytest.fixture(scope="module")
def oracle_containers(oracle, volumes):
    return {key + (mode,): oracle.comp_3d(filled, CHUNKS, mode, q)
            for key, (_, _, filled) in volumes.items() for mode, q in QUALITY.items()}


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_compress_masked_equals_the_oracle_on_the_infilled_volume(eng, volumes, oracle_containers, case, dt, mode):
    import torch
    v, mask, filled = volumes[(case, dt)]
    dv = torch.from_numpy(v).cuda()
    container, stream = eng.compress_masked(dv, CHUNKS, QUALITY[mode], mode=mode, missing=CASES[case][0])
    assert bytes(stream.cpu().numpy()) == M.stream(mask)
    assert bytes(container.cpu().numpy()) == oracle_containers[(case, dt, mode)], "the container differs from the oracle's"
    assert same_bits(dv.cpu().numpy(), v), "the source was written"
    dense = eng.compress(torch.from_numpy(filled).cuda(), CHUNKS, QUALITY[mode], mode=mode)
    assert bytes(dense.cpu().numpy()) == bytes(container.cpu().numpy())


@pytest.mark.parametrize("output_float", [True, False])
@pytest.mark.parametrize("case", sorted(CASES))
def test_decompress_masked_is_the_dense_decode_with_the_value_put_in(eng, volumes, oracle_containers, case, output_float):
    _, mask, _ = volumes[(case, "float32")]
    container = to_dev(oracle_containers[(case, "float32", 1)])
    stream = to_dev(M.stream(mask))
    (lx, ly, lz), (bx, by, bz) = BOX_LO, BOX_DIMS
    sub = mask[lz:lz + bz, ly:ly + by, lx:lx + bx]
    for pct in (0, 30):
        whole = eng.decompress(container, output_float=output_float, pct=pct).cpu().numpy()
        box = eng.decompress_box(container, BOX_LO, BOX_DIMS, output_float=output_float, pct=pct).cpu().numpy()
        for value in (float("nan"), 1e20, -0.0):
            want = whole.copy()
            want[mask] = whole.dtype.type(value)
            got = eng.decompress_masked(container, stream, value, pct=pct, output_float=output_float)
            assert same_bits(got.cpu().numpy(), want), (pct, value)
            want = box.copy()
            want[sub] = box.dtype.type(value)
            got = eng.decompress_masked(container, stream, value, BOX_LO, BOX_DIMS, pct=pct, output_float=output_float)
            assert same_bits(got.cpu().numpy(), want), (pct, value)


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_quality_masked_equals_quality_of_the_compacted_arrays(eng, volumes, oracle_containers, case, dt):
    import torch
    v, mask, _ = volumes[(case, dt)]
    container = to_dev(oracle_containers[(case, dt, 1)])
    stream = to_dev(M.stream(mask))
    orig = torch.from_numpy(v).cuda()
    recon = eng.decompress_masked(container, stream, float("nan"), output_float=dt == "float32")
    keep = torch.from_numpy(~mask).cuda()
    want = eng.quality(orig[keep].contiguous(), recon[keep].contiguous())
    got = eng.quality_masked(orig, recon, stream)
    fig = lambda q: np.array([q.rmse, q.linfty, q.psnr, q.min, q.max, q.mean, q.var, q.mse]).view(np.uint64)
    assert np.array_equal(fig(got), fig(want)), (got, want)
    assert np.isfinite(got.rmse) and got.rmse > 0


def test_nothing_missing_gives_the_dense_container_and_a_header(eng, oracle):
    import torch
    v = turbulence(VOL_ZYX, dtype=np.float64).astype(np.float32)
    dv = torch.from_numpy(v).cuda()
    container, stream = eng.compress_masked(dv, CHUNKS, 2.5)
    assert stream.numel() == 32 and bytes(stream.cpu().numpy()) == M.stream(np.zeros(v.size, dtype=bool))
    assert bytes(container.cpu().numpy()) == bytes(eng.compress(dv, CHUNKS, 2.5).cpu().numpy())
    assert bytes(container.cpu().numpy()) == oracle.comp_3d(v, CHUNKS, 1, 2.5)
    back = eng.decompress_masked(container, stream, 1e20)
    assert same_bits(back.cpu().numpy(), eng.decompress(container).cpu().numpy())
    q, want = eng.quality_masked(dv, back, stream), eng.quality(dv, back)
    assert (q.rmse, q.linfty, q.psnr, q.mean, q.var) == (want.rmse, want.linfty, want.psnr, want.mean, want.var)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_as_it_was(eng, volumes, oracle_containers):
    import torch
    from sperr_amd.api import SperrHipError
    v, mask, _ = volumes[("ball", "float32")]
    container = to_dev(oracle_containers[("ball", "float32", 1)])
    good = M.stream(mask)
    out = sentinel_like(VOL_ZYX, np.float32)
    keep = sentinel_like(VOL_ZYX, np.float32).cpu().numpy()

    def refused(stream_bytes, length=None, **kw):
        s = to_dev(stream_bytes + b"\0" * 8)[:len(stream_bytes) if length is None else length]
        with pytest.raises(SperrHipError):
            eng.decompress_masked(container, s, 0.0, out=out, **kw)
        with pytest.raises(SperrHipError):
            eng.mask_apply(out, s, 0.0)
        torch.cuda.synchronize()
        assert same_bits(out.cpu().numpy(), keep)

    refused(b"SPMX" + good[4:])                                       # bad magic
    refused(good[:4] + b"\x02" + good[5:])                            # a version this library does not know
    refused(M.stream(np.concatenate([mask.reshape(-1), [False]])))    # wrong n
    refused(good, length=len(good) - 1)                               # one byte short
    with pytest.raises(SperrHipError):                                # a level: a mask has no coarser level
        eng.decompress_masked(container, to_dev(good), 0.0, out=out, level=0)
    with pytest.raises(SperrHipError):                                # a box that leaves the volume
        eng.decompress_masked(container, to_dev(good), 0.0, (30, 5, 7), BOX_DIMS,
                              out=sentinel_like(tuple(reversed(BOX_DIMS)), np.float32))
    small = sentinel_like((VOL_ZYX[0], VOL_ZYX[1], VOL_ZYX[2] - 1), np.float32)
    with pytest.raises(SperrHipError):                                # an output that does not hold the volume
        eng.decompress_masked(container, to_dev(good), 0.0, out=small)
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), keep)
    assert same_bits(small.cpu().numpy(), sentinel_like(tuple(small.shape), np.float32).cpu().numpy())
    # quality: a stream of another n, and no valid sample
    dv = torch.from_numpy(v).cuda()
    with pytest.raises(SperrHipError):
        eng.quality_masked(dv.reshape(-1)[:-1].contiguous(), dv.reshape(-1)[:-1].contiguous(), to_dev(good))
    with pytest.raises(SperrHipError):
        eng.quality_masked(dv, dv, to_dev(M.stream(np.ones(v.size, dtype=bool))))


def test_a_mask_capacity_one_byte_short_returns_one_and_the_size(eng, volumes):
    import torch
    v, mask, _ = volumes[("ball", "float32")]
    need = len(M.stream(mask))
    dv = torch.from_numpy(v).cuda()
    buf = torch.full((need + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    filled = sentinel_like(VOL_ZYX, np.float32)
    mlen, nmiss = _sz(0), _sz(99)
    rtn = eng.lib.sperrhip_mask_make_dev(dv.data_ptr(), 1, v.size, M.RULE_NAN, 0.0, filled.data_ptr(), buf.data_ptr(),
                                         need - 1, C.byref(mlen), C.byref(nmiss), None)
    torch.cuda.synchronize()
    assert rtn == 1 and mlen.value == need and nmiss.value == 99
    assert bool((buf == 0xA5).all()) and same_bits(filled.cpu().numpy(), sentinel_like(VOL_ZYX, np.float32).cpu().numpy())
    # ... and compress_masked: neither the mask nor the container is written
    cap = eng.max_compressed_size(VOL_ZYX, CHUNKS, 2.5, 1)
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    dlen, mlen = _sz(55), _sz(0)
    rtn = eng.lib.sperrhip_compress_masked_dev(dv.data_ptr(), 1, VOL_ZYX[2], VOL_ZYX[1], VOL_ZYX[0], *CHUNKS, 1, 2.5,
                                               M.RULE_NAN, 0.0, dst.data_ptr(), cap, C.byref(dlen), buf.data_ptr(),
                                               need - 1, C.byref(mlen), C.byref(nmiss), None)
    torch.cuda.synchronize()
    assert rtn == 1 and mlen.value == need and dlen.value == 55 and nmiss.value == 99
    assert bool((buf == 0xA5).all()) and bool((dst == 0xA5).all())
    # the exact size is enough
    rtn = eng.lib.sperrhip_mask_make_dev(dv.data_ptr(), 1, v.size, M.RULE_NAN, 0.0, None, buf.data_ptr(), need,
                                         C.byref(mlen), C.byref(nmiss), None)
    torch.cuda.synchronize()
    assert rtn == 0 and mlen.value == need and nmiss.value == int(mask.sum())
    assert bytes(buf[:need].cpu().numpy()) == M.stream(mask) and bool((buf[need:] == 0xA5).all())
    # a mode that is none of the three answers 2 before anything else
    assert eng.lib.sperrhip_compress_masked_dev(None, 1, 0, 0, 0, *CHUNKS, 4, 2.5, M.RULE_NAN, 0.0, None, 0, None, None,
                                                0, None, None, None) == 2


# ---- launch tables -------------------------------------------------------------------------------------------------
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


# the kernels of mask.hip (k_mask_scan is none of them: it is the encoder's, speck_enc.hip)
FAMILY = ["k_mask_survey", "k_mask_finish", "k_mask_pack", "k_mask_fill", "k_mask_apply", "k_mask_expand",
          "k_mask_unpack", "k_mask_count", "k_mask_offsets", "k_mask_compact"]


def _count(table, name):
    names = FAMILY if name == "k_mask_" else [name]
    return sum(n for k, n in table.items() if any(nm in k for nm in names))


def test_launch_tables(eng, volumes, oracle_containers):
    import torch
    v, mask, filled = volumes[("ball", "float32")]
    dv, df = torch.from_numpy(v).cuda(), torch.from_numpy(filled).cuda()
    container, table = launched(eng, lambda: eng.compress(df, CHUNKS, 2.5))
    assert table and _count(table, "k_mask_") == 0, table
    _, table = launched(eng, lambda: eng.decompress(container))
    assert table and _count(table, "k_mask_") == 0, table
    _, table = launched(eng, lambda: eng.decompress_box(container, BOX_LO, BOX_DIMS))
    assert table and _count(table, "k_mask_") == 0, table
    (c2, stream), table = launched(eng, lambda: eng.compress_masked(dv, CHUNKS, 2.5))
    assert [_count(table, k) for k in ("k_mask_survey", "k_mask_finish", "k_mask_pack", "k_mask_fill")] == [1, 1, 1, 1], table
    assert _count(table, "k_mask_") == 4 and bytes(c2.cpu().numpy()) == bytes(container.cpu().numpy())
    _, table = launched(eng, lambda: eng.decompress_masked(container, stream, 0.0))
    assert _count(table, "k_mask_apply") == 1 and _count(table, "k_mask_") == 1, table
    # a stream of kind 0 launches no k_mask_apply
    none = to_dev(M.stream(np.zeros(v.size, dtype=bool)))
    _, table = launched(eng, lambda: eng.decompress_masked(container, none, 0.0))
    assert table and _count(table, "k_mask_") == 0, table
    out = torch.zeros(v.size, dtype=torch.float32, device="cuda")
    _, table = launched(eng, lambda: eng.mask_apply(out, none, 1.0))
    assert _count(table, "k_mask_") == 0, table
