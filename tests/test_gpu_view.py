"""GPU: strided views of device arrays (include/sperr_hip.h "strided views", sperr_amd/csrc/view.h) -- the interior of
an array with ghost cells goes into compress, a decode goes into the interior of another, and quality() compares two
interiors, with no packed copy anywhere.

Every comparison is bit for bit, against the same call on the packed copy (which the other test files pin to the
oracle and the reference) and, for containers, against the CPU oracle as well.  Every parent is filled with a
sentinel, a NaN with a payload, and whatever lies outside a view has to hold it afterwards.

  compress     40 x 48 x 56 (x, y, z) in 32^3 chunks -- merged remainders, several shape groups -- inside a parent with
               a halo of (3 + 4, 2 + 2, 1 + 1): the row pitch is 47, odd, and the first element misaligned; fp32 and
               fp64, fixed rate, PSNR and PWE.  A 64^3 chunk in a 96 x 80 x 70 parent at an origin that is a multiple of
               four floats takes k_stride_sums_rows and the x-y-z head with pitch != dimx, and the fallback one element
               further; one shape each for the x-y head and the per-axis head; an 8^3 chunk that is not transformed;
               a constant chunk beside one that takes the 64-bit retry
  decompress   those containers into views, fp32 and fp64, and a 50 % portion
  box          box (5, 6, 7) + (40, 30, 20) of 64 x 60 x 50 into the interior of a padded parent, whole and at 50 %
  quality      six windows (two rows of 16384 and a tail past 8192 with a pack across every x-row's end; dimx 1; a tiny
               one; 130 x 129 x 3; an x-row longer than a block; whole packs only), both sides views of different
               pitches, one side only, and pitches equal to the dims; identical arrays
  refusals     every invalid view, a destination that is too small, and the calls that take no views
  launches     a call through a view with pitch == dims launches what the dense call launches"""
import ctypes as C

import numpy as np
import pytest

from fields import smooth_field
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu

SENTINEL = {np.dtype(np.float32): 0x7FC0BEEF, np.dtype(np.float64): 0x7FF80000DEADBEEF}
_sz = C.c_size_t


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    yield e
    e.release()


# ---- parents, windows and what lies around them ------------------------------------------------------------------
def _bits(t):
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def parent_of(shape_zyx, dtype):
    """a cuda tensor of the sentinel"""
    import torch
    dt = np.dtype(dtype)
    it = torch.int32 if dt == np.float32 else torch.int64
    p = torch.full(tuple(shape_zyx), SENTINEL[dt], dtype=it, device="cuda")
    return p.view(torch.float32 if dt == np.float32 else torch.float64)


def window_in(parent, lo_zyx, shape_zyx):
    return parent[tuple(slice(o, o + n) for o, n in zip(lo_zyx, shape_zyx))]


def halo_parent(v, lo_zyx=(1, 2, 3), hi_zyx=(1, 2, 4)):
    """(parent, window): numpy volume v inside a sentinel parent with `lo` cells before and `hi` cells behind it"""
    import torch
    p = parent_of([a + n + b for a, n, b in zip(lo_zyx, v.shape, hi_zyx)], v.dtype)
    w = window_in(p, lo_zyx, v.shape)
    w.copy_(torch.from_numpy(np.array(v)).cuda())
    assert not w.is_contiguous() or v.size == 1
    return p, w


def assert_halo_untouched(parent, lo_zyx, shape_zyx):
    """everything outside the window still holds the sentinel"""
    b = _bits(parent).clone()
    s = SENTINEL[np.dtype(np.float32 if parent.element_size() == 4 else np.float64)]
    window_in(b, lo_zyx, shape_zyx).fill_(s)
    assert bool((b == s).all()), "elements outside the view were written"


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((_bits(a.contiguous()) == _bits(b.contiguous())).all())


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


def ran(names, kernel):
    return any(k == kernel or k.startswith(kernel + "<") or k.startswith("(" + kernel + "<") for k in names)


def chunk_streams(container):
    """the chunks' streams of a container (one chunk: the short header, without chunk dims)"""
    multi = bool(container[1] & 0x10)
    pos = 20 if multi else 14
    vol = np.frombuffer(container, dtype=np.uint32, count=3, offset=2)
    ch = np.frombuffer(container, dtype=np.uint16, count=3, offset=14) if multi else vol
    nch = int(np.prod([(int(v) + int(c) - 1) // int(c) for v, c in zip(vol, ch)]))
    lens = np.frombuffer(container, dtype=np.uint32, count=nch, offset=pos)
    offs = pos + 4 * nch + np.concatenate([[0], np.cumsum(lens.astype(np.int64))[:-1]])
    return [container[int(o):int(o) + int(n)] for o, n in zip(offs, lens)]


def to_dev(container):
    import torch
    return torch.from_numpy(np.frombuffer(container, dtype=np.uint8).copy()).cuda()


# ---- the volumes and their containers, made once -----------------------------------------------------------------
HALO_SHAPE = (56, 48, 40)   # 40 x 48 x 56 as (z, y, x)
_VOLS, _WANT = {}, {}


def halo_volume(dtype):
    key = np.dtype(dtype).name
    if key not in _VOLS:
        v = turbulence(HALO_SHAPE, dtype=np.dtype(dtype).type)
        v.setflags(write=False)
        _VOLS[key] = v
    return _VOLS[key]


def halo_setting(dtype, mode):
    v = halo_volume(dtype)
    return {1: 2.0, 2: 80.0, 3: 1e-3 * float(v.astype(np.float64).max() - v.astype(np.float64).min())}[mode]


def oracle_container(oracle, key, v, chunks, mode, q):
    if key not in _WANT:
        _WANT[key] = oracle.comp_3d(np.ascontiguousarray(v), chunks, mode, q)
    return _WANT[key]


def wide_and_constant():
    """(32, 32, 64): a constant 32^3 chunk beside a smooth one, which at 40 bpp and at 230 dB has more than 32 bit planes"""
    v = smooth_field((32, 32, 64), dtype=np.float32)
    v[:, :, :32] = 0.75
    return v


def compress_both_ways(eng, oracle, key, v, chunks, mode, q, lo=(1, 2, 3), hi=(1, 2, 4)):
    """the container of v read through a view: it equals the dense call's on the packed copy and the oracle's, and the
    parent is as it was.  Returns (container bytes, launches of the view call)."""
    parent, w = halo_parent(v, lo, hi)
    before = _bits(parent).clone()
    got, names = launched(eng, lambda: bytes(eng.compress(w, chunks, q, mode=mode).cpu().numpy()))
    dense = bytes(eng.compress(w.contiguous(), chunks, q, mode=mode).cpu().numpy())
    assert got == dense, (key, "the view's container differs from the packed copy's")
    assert got == oracle_container(oracle, key, v, chunks, mode, q), (key, "the container differs from the oracle's")
    assert bool((_bits(parent) == before).all()), (key, "compress wrote to its source")
    return got, names


# ---- compress ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_compress_view_with_odd_pitch(eng, oracle, dtype, mode):
    v = halo_volume(dtype)
    parent, w = halo_parent(v)
    assert w.stride() == (52 * 47, 47, 1) and w.data_ptr() % 16 != 0
    _, names = compress_both_ways(eng, oracle, ("halo", dtype, mode), v, (32, 32, 32), mode, halo_setting(dtype, mode))
    assert ran(names, "k_stride_sums") and not ran(names, "k_stride_sums_rows")


@pytest.mark.parametrize("shift,rows", [(0, True), (1, False)])
def test_compress_view_aligned_paths(eng, oracle, shift, rows):
    """a 64^3 chunk in a 96 x 80 x 70 parent: with the origin at a multiple of four floats the rows kernel and the
    x-y-z head run although pitch != dimx; one element further the conditioner falls back"""
    v = turbulence((64, 64, 64))
    lo = (3, 8, 16 + shift)
    hi = tuple(p - o - 64 for p, o in zip((70, 80, 96), lo))
    _, w = halo_parent(v, lo, hi)
    assert w.stride() == (80 * 96, 96, 1) and (w.data_ptr() % 16 == 0) == rows
    _, names = compress_both_ways(eng, oracle, ("aligned",), v, (64, 64, 64), 1, 2.0, lo, hi)
    assert ran(names, "k_stride_sums_rows") == rows and ran(names, "k_stride_sums") == (not rows), names
    assert ran(names, "k_lift_xyz_fwd"), names


@pytest.mark.parametrize("name,shape_zyx,chunks,kernel", [
    ("xy_head", (20, 20, 512), (512, 20, 20), "k_lift_xy"),       # rows too long for the x-y-z head
    ("axis_head", (20, 23, 2), (2, 23, 20), "k_lift_axis<true, 1>"),   # a wavelet-packet chunk: per-axis passes
    ("untransformed", (8, 8, 8), (8, 8, 8), "k_gather_condition"),
])
def test_compress_view_other_heads(eng, oracle, name, shape_zyx, chunks, kernel):
    v = turbulence(shape_zyx)
    got, names = compress_both_ways(eng, oracle, (name,), v, chunks, 1, 2.0)
    assert any(kernel in k for k in names), names
    if name == "untransformed":
        assert not any("k_lift" in k for k in names), names


@pytest.mark.parametrize("mode,q", [(1, 40.0), (2, 230.0)])
def test_compress_view_constant_and_wide_chunks(eng, oracle, mode, q):
    v = wide_and_constant()
    got, _ = compress_both_ways(eng, oracle, ("wide", mode), v, (32, 32, 32), mode, q)
    streams = chunk_streams(got)
    assert any(len(s) >= 26 and not (s[0] & 1) and s[17] > 32 for s in streams), "no chunk with 64-bit coefficients"
    assert any(s[0] & 1 for s in streams) or any(len(s) < 26 for s in streams), "no constant chunk"


# ---- decompress into a view --------------------------------------------------------------------------------------
def decode_into_view(eng, container, shape_zyx, output_float, pct=0, lo=(2, 1, 5), hi=(1, 3, 2)):
    import torch
    dev = to_dev(container)
    dt = np.float32 if output_float else np.float64
    parent = parent_of([a + n + b for a, n, b in zip(lo, shape_zyx, hi)], dt)
    w = window_in(parent, lo, shape_zyx)
    ret = eng.decompress(dev, output_float=output_float, out=w, pct=pct)
    torch.cuda.synchronize()
    assert ret.data_ptr() == w.data_ptr()
    want = eng.decompress(dev, output_float=output_float, pct=pct)
    assert same_bits(w, want), "the view's interior differs from the dense decode"
    assert_halo_untouched(parent, lo, shape_zyx)


@pytest.mark.parametrize("output_float", [True, False])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_decompress_into_view(eng, oracle, mode, output_float):
    v = halo_volume("float32")
    c = oracle_container(oracle, ("halo", "float32", mode), v, (32, 32, 32), mode, halo_setting("float32", mode))
    decode_into_view(eng, c, HALO_SHAPE, output_float)


def test_decompress_fp64_container_into_view(eng, oracle):
    v = halo_volume("float64")
    c = oracle_container(oracle, ("halo", "float64", 3), v, (32, 32, 32), 3, halo_setting("float64", 3))
    decode_into_view(eng, c, HALO_SHAPE, False)
    decode_into_view(eng, c, HALO_SHAPE, True)


def test_decompress_portion_into_view(eng, oracle):
    v = halo_volume("float32")
    c = oracle_container(oracle, ("halo", "float32", 1), v, (32, 32, 32), 1, halo_setting("float32", 1))
    decode_into_view(eng, c, HALO_SHAPE, True, pct=50)


@pytest.mark.parametrize("output_float", [True, False])
def test_decompress_special_chunks_into_view(eng, oracle, output_float):
    w = wide_and_constant()
    for mode, q in ((1, 40.0), (2, 230.0)):
        decode_into_view(eng, oracle_container(oracle, ("wide", mode), w, (32, 32, 32), mode, q), w.shape, output_float)
    t = turbulence((8, 8, 8))
    decode_into_view(eng, oracle_container(oracle, ("untransformed",), t, (8, 8, 8), 1, 2.0), t.shape, output_float)


@pytest.mark.parametrize("pct", [0, 50])
@pytest.mark.parametrize("output_float", [True, False])
def test_box_into_view(eng, oracle, output_float, pct):
    import torch
    v = turbulence((50, 60, 64))
    dev = to_dev(oracle_container(oracle, ("box",), v, (32, 32, 32), 1, 4.0))
    lo_xyz, dims_xyz = (5, 6, 7), (40, 30, 20)
    shape = tuple(reversed(dims_xyz))
    lo = (2, 3, 4)
    parent = parent_of([a + n + b for a, n, b in zip(lo, shape, (2, 2, 5))], np.float32 if output_float else np.float64)
    w = window_in(parent, lo, shape)
    eng.decompress_box(dev, lo_xyz, dims_xyz, output_float=output_float, out=w, pct=pct)
    torch.cuda.synchronize()
    want = eng.decompress_box(dev, lo_xyz, dims_xyz, output_float=output_float, pct=pct)
    assert same_bits(w, want), "the box in the view differs from the dense box"
    assert_halo_untouched(parent, lo, shape)


# ---- quality -----------------------------------------------------------------------------------------------------
QUALITY_WINDOWS = [(37, 29, 41), (1, 300, 60), (3, 5, 7), (130, 129, 3), (20000, 3, 1), (128, 128, 2)]   # (x, y, z)
HALO_A = ((1, 2, 3), (1, 1, 4))   # (cells before, cells behind) per (z, y, x): two different parents
HALO_B = ((0, 1, 0), (2, 0, 5))


def figures(q):
    return np.array([q.rmse, q.linfty, q.psnr, q.min, q.max, q.mean, q.var, q.mse], dtype=np.float64).view(np.uint64)


def quality_c(eng, a, va, b, vb):
    """sperrhip_quality_view_dev itself: va / vb are (pitch_y, pitch_z) or None for a NULL view"""
    import torch
    from sperr_amd.api import View
    dz, dy, dx = a.shape
    out = (C.c_double * 8)()
    rtn = eng.lib.sperrhip_quality_view_dev(a.data_ptr(), None if va is None else C.byref(View(*va)), b.data_ptr(),
                                            None if vb is None else C.byref(View(*vb)),
                                            int(a.dtype == torch.float32), dx, dy, dz, out, eng._stream())
    return rtn, np.array(out[:8], dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("dims_xyz", QUALITY_WINDOWS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_quality_of_views(eng, dtype, dims_xyz):
    shape = tuple(reversed(dims_xyz))
    rng = np.random.default_rng(1234 + dims_xyz[0])
    a = (rng.standard_normal(shape) * 3.0 + 0.25).astype(dtype)
    b = (a + rng.standard_normal(shape).astype(dtype) * np.dtype(dtype).type(1e-3)).astype(dtype)
    _, wa = halo_parent(a, *HALO_A)
    _, wb = halo_parent(b, *HALO_B)
    ca, cb = wa.contiguous(), wb.contiguous()
    want = figures(eng.quality(ca, cb))
    assert np.isfinite(want.view(np.float64)).all() and want.view(np.float64)[0] > 0
    assert np.array_equal(figures(eng.quality(wa, wb)), want), "both sides views"
    assert np.array_equal(figures(eng.quality(wa, cb)), want), "only orig a view"
    assert np.array_equal(figures(eng.quality(ca, wb)), want), "only recon a view"
    # pitches equal to the dims, through the view kernel: as a view, and as NULL
    dx, dy = dims_xyz[0], dims_xyz[1]
    for va, vb in (((dx, dx * dy), (dx, dx * dy)), (None, None), ((dx, dx * dy), None)):
        rtn, got = quality_c(eng, ca, va, cb, vb)
        assert rtn == 0 and np.array_equal(got, want), ("dense pitches", va, vb)


def test_quality_of_identical_views(eng):
    a = turbulence((41, 29, 37))
    _, wa = halo_parent(a, *HALO_A)
    _, wb = halo_parent(a, *HALO_B)
    q = eng.quality(wa, wb)
    assert q.psnr == float("inf") and q.rmse == 0.0 and q.linfty == 0.0 and q.mse == 0.0
    assert np.array_equal(figures(q), figures(eng.quality(wa.contiguous(), wb.contiguous())))


# ---- refusals ----------------------------------------------------------------------------------------------------
BAD_VIEWS = [(39, 48 * 39), (0, 0), (47, 47 * 47), (47, 47 * 52 + 1), (47, 47 * 48 - 47), (2 ** 63, 2 ** 63)]


def test_invalid_views_are_refused(eng):
    import torch
    from sperr_amd.api import View
    v = halo_volume("float32")
    parent, w = halo_parent(v)
    dz, dy, dx = HALO_SHAPE
    out = torch.zeros(eng.max_compressed_size(HALO_SHAPE, (32, 32, 32), 2.0), dtype=torch.uint8, device="cuda")
    n = _sz(0)
    good = eng.compress(w, (32, 32, 32), 2.0)
    dst = parent_of(parent.shape, np.float32)
    room = dst.numel() * 4
    fig = (C.c_double * 8)(*([-1.0] * 8))
    for py, pz in BAD_VIEWS:
        bad = C.byref(View(py, pz))
        assert eng.lib.sperrhip_compress_view_dev(w.data_ptr(), bad, 1, dx, dy, dz, 32, 32, 32, 1, 2.0, out.data_ptr(),
                                                  out.numel(), C.byref(n), eng._stream()) == -1, (py, pz)
        assert eng.lib.sperrhip_decompress_view_dev(good.data_ptr(), good.numel(), 0, 1, None, None, dst.data_ptr(), bad,
                                                    room, eng._stream()) == -1, (py, pz)
        assert eng.lib.sperrhip_quality_view_dev(w.data_ptr(), bad, w.data_ptr(), None, 1, dx, dy, dz, fig,
                                                 eng._stream()) == -1, (py, pz)
        assert eng.lib.sperrhip_quality_view_dev(w.data_ptr(), None, w.data_ptr(), bad, 1, dx, dy, dz, fig,
                                                 eng._stream()) == -1, (py, pz)
    ok = C.byref(View(47, 47 * 52))
    # NULL pointers
    assert eng.lib.sperrhip_compress_view_dev(w.data_ptr(), None, 1, dx, dy, dz, 32, 32, 32, 1, 2.0, out.data_ptr(),
                                              out.numel(), C.byref(n), eng._stream()) == -1
    assert eng.lib.sperrhip_compress_view_dev(None, ok, 1, dx, dy, dz, 32, 32, 32, 1, 2.0, out.data_ptr(),
                                              out.numel(), C.byref(n), eng._stream()) == -1
    assert eng.lib.sperrhip_decompress_view_dev(good.data_ptr(), good.numel(), 0, 1, None, None, dst.data_ptr(), None,
                                                room, eng._stream()) == -1
    assert eng.lib.sperrhip_decompress_view_dev(good.data_ptr(), good.numel(), 0, 1, None, None, None, ok,
                                                room, eng._stream()) == -1
    assert eng.lib.sperrhip_quality_view_dev(None, ok, w.data_ptr(), ok, 1, dx, dy, dz, fig, eng._stream()) == -1
    assert eng.lib.sperrhip_quality_view_dev(w.data_ptr(), ok, w.data_ptr(), ok, 1, dx, dy, 0, fig, eng._stream()) == -1
    # a box with only one of lo / dims
    lo3 = (_sz * 3)(0, 0, 0)
    assert eng.lib.sperrhip_decompress_view_dev(good.data_ptr(), good.numel(), 0, 1, lo3, None, dst.data_ptr(), ok,
                                                room, eng._stream()) == -1
    torch.cuda.synchronize()
    assert not bool(out.any()) and list(fig) == [-1.0] * 8
    assert bool((_bits(dst) == SENTINEL[np.dtype(np.float32)]).all()), "a refused call wrote to its destination"


def test_too_small_destination_is_refused_untouched(eng):
    import torch
    from sperr_amd.api import View
    v = halo_volume("float32")
    good = eng.compress(torch.from_numpy(np.array(v)).cuda(), (32, 32, 32), 2.0)
    dz, dy, dx = HALO_SHAPE
    extent = (dz - 1) * 47 * 52 + (dy - 1) * 47 + dx
    dst = parent_of((extent,), np.float32)
    view = C.byref(View(47, 47 * 52))
    assert eng.lib.sperrhip_decompress_view_dev(good.data_ptr(), good.numel(), 0, 1, None, None, dst.data_ptr(), view,
                                                extent * 4 - 1, eng._stream()) == -1
    lo3, d3 = (_sz * 3)(1, 1, 1), (_sz * 3)(30, 30, 30)
    box_extent = 29 * 47 * 52 + 29 * 47 + 30
    assert eng.lib.sperrhip_decompress_view_dev(good.data_ptr(), good.numel(), 0, 1, lo3, d3, dst.data_ptr(), view,
                                                box_extent * 4 - 4, eng._stream()) == -1
    torch.cuda.synchronize()
    assert bool((_bits(dst) == SENTINEL[np.dtype(np.float32)]).all()), "a refused call wrote to its destination"
    # ... and with exactly the extent it is taken
    assert eng.lib.sperrhip_decompress_view_dev(good.data_ptr(), good.numel(), 0, 1, None, None, dst.data_ptr(), view,
                                                extent * 4, eng._stream()) == 0
    torch.cuda.synchronize()
    w = torch.as_strided(dst, HALO_SHAPE, (47 * 52, 47, 1))
    assert same_bits(w, eng.decompress(good))


def test_tensors_that_are_no_views_raise(eng):
    import torch
    from sperr_amd.api import SperrHipError
    p = torch.zeros((20, 24, 48), dtype=torch.float32, device="cuda")
    flat = torch.zeros(4096, dtype=torch.float32, device="cuda")
    no_views = [p[:, :, ::2],                                    # x stride 2
                p.permute(0, 2, 1),                              # x stride is the row pitch
                torch.as_strided(flat, (3, 4, 5), (50, 7, 1)),   # slice pitch no multiple of the row pitch
                torch.as_strided(flat, (3, 4, 5), (20, 4, 1)),   # rows overlap
                torch.as_strided(flat, (3, 4, 5), (14, 7, 1)),   # slices overlap
                p.flip(2).as_strided((4, 4, 4), (0, 8, 1))]      # all slices are one
    good = eng.compress(torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda") + 1.5, (4, 4, 4), 2.0)
    for t in no_views:
        with pytest.raises(SperrHipError):
            eng.compress(t, (32, 32, 32), 2.0)
        with pytest.raises(SperrHipError):
            eng.quality(t, t.contiguous())
    for strides in ((50, 7, 1), (14, 7, 1), (16, 3, 1)):
        with pytest.raises(SperrHipError):
            eng.decompress(good, out=torch.as_strided(flat, (4, 4, 4), strides), shape_zyx=(4, 4, 4))
    # a view of the wrong shape, and calls that take no views
    w = p[1:5, 2:6, 3:7]
    with pytest.raises(SperrHipError):
        eng.decompress(good, out=p[1:5, 2:6, 3:8])
    with pytest.raises(SperrHipError):
        eng.decompress_box(good, (0, 0, 0), (2, 2, 2), out=w)
    with pytest.raises(SperrHipError):
        eng.quality(w, p[1:5, 2:6, 3:8])
    with pytest.raises(SperrHipError):
        eng.decompress_level(good, 0, output_float=True, out=w)
    with pytest.raises(SperrHipError):
        eng.compress_batch(p[None, :, :, 8:40].expand(2, 20, 24, 32), (16, 16, 16), 2.0)
    with pytest.raises(SperrHipError):
        eng.compress_2d(p[3, :, 8:40], 2.0)
    assert same_bits(eng.decompress(good, out=w), eng.decompress(good))


# ---- a view with the dims' own pitches launches what the dense call launches ------------------------------------
def test_dense_pitches_launch_the_dense_kernels(eng, oracle):
    import torch
    from sperr_amd.api import View
    v = halo_volume("float32")
    dz, dy, dx = HALO_SHAPE
    dv = torch.from_numpy(np.array(v)).cuda()
    view = View(dx, dx * dy)
    cap = eng.max_compressed_size(HALO_SHAPE, (32, 32, 32), 2.0)

    def compress_view():
        out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        n = _sz(0)
        assert eng.lib.sperrhip_compress_view_dev(dv.data_ptr(), C.byref(view), 1, dx, dy, dz, 32, 32, 32, 1, 2.0,
                                                  out.data_ptr(), cap, C.byref(n), eng._stream()) == 0
        return out[:n.value]

    def decompress_view(c):
        out = torch.empty(HALO_SHAPE, dtype=torch.float32, device="cuda")
        assert eng.lib.sperrhip_decompress_view_dev(c.data_ptr(), c.numel(), 0, 1, None, None, out.data_ptr(),
                                                    C.byref(view), out.numel() * 4, eng._stream()) == 0
        return out

    eng.decompress(eng.compress(dv, (32, 32, 32), 2.0))   # (the plans are made: no first-call launches in the tables)
    c, dense_c = launched(eng, lambda: eng.compress(dv, (32, 32, 32), 2.0))
    cv, view_c = launched(eng, compress_view)
    assert bytes(c.cpu().numpy()) == bytes(cv.cpu().numpy()) and dense_c == view_c, (dense_c, view_c)
    back, dense_d = launched(eng, lambda: eng.decompress(c))
    backv, view_d = launched(eng, lambda: decompress_view(c))
    assert same_bits(back, backv) and dense_d == view_d, (dense_d, view_d)
    q, dense_q = launched(eng, lambda: figures(eng.quality(dv, back)))
    (rtn, qv), view_q = launched(eng, lambda: quality_c(eng, dv, (dx, dx * dy), back, (dx, dx * dy)))
    assert rtn == 0 and np.array_equal(q, qv) and dense_q == view_q, (dense_q, view_q)
    assert sorted(dense_q.values()) == [1, 1, 1] and ran(dense_q, "k_quality_rows"), dense_q
