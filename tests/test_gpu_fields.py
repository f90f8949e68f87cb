"""GPU: interleaved fields of a device array (include/sperr_hip.h "interleaved fields", sperr_amd/csrc/fields.h,
fields.hip) -- a (z, y, x, nvar) array goes into compress_fields, containers are decoded into some fields of another,
and quality_fields compares two, with no packed copy of the caller's making.

Every comparison is bit for bit, through integer views.  Every parent is filled with a sentinel, a NaN with a payload,
and whatever is not a selected field of a sample inside the dims has to hold it afterwards.

  kernels      k_fields_gather / k_fields_scatter alone (fields_gather, fields_scatter) against torch indexing: every
               (stride_x, nfields, first) of CASES with every dimx of DIMX (1, 3 and the sizes around a tile, the
               constant parsed from fields.h), dimy and dimz in {1, 2, 3}, row and slice padding of 0, 1 and 5 elements
               (a slice pitch that is no multiple of the row pitch), an odd first element, fp32 and fp64: 54 cases.
               One aligned and one misaligned case shown by the profiler to run the kVec and the element form
  end to end   (30, 44, 37) in (32, 32, 32) chunks -- remainder chunks, k_lis_mx -- of three fields: turbulence, the
               same a hundred times as large, a constant.  Containers against the oracle in modes 1, 2 and 3, fp32 and
               fp64; a decode of fields 1..2 of a four-field parent with halo from containers of different modes and
               precisions; a decode at field_dim=0 into a channels-last tensor; the figures
  refusals     leave the destination bitwise as it was
  launches     compress_batch launches no k_fields_* kernel"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = {4: 0x7FC0BEEF, 8: 0x7FF80000DEADBEEF}
_sz = C.c_size_t


def _const(name):
    text = open(os.path.join(ROOT, "sperr_amd", "csrc", "fields.h")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)\s*;", text).group(1))


TILE = _const("kFieldsTileX")
MAXLDS = _const("kFieldsMaxLdsStride")
CASES = [(1, 1, 0), (2, 2, 0), (3, 3, 0), (4, 4, 0), (5, 2, 1), (8, 8, 0), (8, 3, 5), (17, 17, 0), (MAXLDS + 1, 1, 0)]
DIMX = [1, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]


def _kernel_cases():
    """CASES x DIMX, with dimy, dimz, the paddings, the first element and the precision cycling at different periods"""
    out = []
    for ci, (stride, nf, first) in enumerate(CASES):
        for xi, dimx in enumerate(DIMX):
            k = ci * len(DIMX) + xi
            dimy, dimz = 1 + k % 3, 1 + (k // 3 + ci) % 3
            rowpad, slicepad = (0, 1, 5)[(k + ci) % 3], (0, 1, 5)[(k // 2) % 3]
            lead = (0, 1, 4, 3)[k % 4]          # elements before the record of sample (0, 0, 0): odd, or whole packs
            dt = ("float32", "float64")[(k + k // 6) % 2]
            out.append((stride, nf, first, dimx, dimy, dimz, rowpad, slicepad, lead, dt))
    return out


KERNEL_CASES = _kernel_cases()
assert len(KERNEL_CASES) <= 60


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    yield e
    e.release()


def _bits(t):
    import torch
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def sentinel_parent(numel, dtype):
    """a 1-D cuda tensor of the sentinel"""
    import torch
    esz = 4 if dtype == torch.float32 else 8
    p = torch.full((numel,), SENTINEL[esz], dtype=torch.int32 if esz == 4 else torch.int64, device="cuda")
    return p.view(dtype)


def fields_view(parent, at, nf, dims_zyx, stride_x, pitch_y, pitch_z):
    """the (z, y, x, f) view of the 1-D parent whose first selected field of sample (0, 0, 0) is element `at`"""
    import torch
    return torch.as_strided(parent, tuple(dims_zyx) + (nf,), (pitch_z, pitch_y, stride_x, 1), at)


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


def to_dev(container):
    import torch
    return torch.from_numpy(np.frombuffer(container, dtype=np.uint8).copy()).cuda()


# ---- the two kernels alone ----------------------------------------------------------------------------------------
def _layout(stride, dimx, dimy, dimz, rowpad, slicepad):
    pitch_y = dimx * stride + rowpad
    pitch_z = pitch_y * dimy + slicepad
    return pitch_y, pitch_z


@pytest.mark.parametrize("stride,nf,first,dimx,dimy,dimz,rowpad,slicepad,lead,dt", KERNEL_CASES)
def test_gather_and_scatter_against_torch_indexing(eng, stride, nf, first, dimx, dimy, dimz, rowpad, slicepad, lead, dt):
    import torch
    dtype = getattr(torch, dt)
    pitch_y, pitch_z = _layout(stride, dimx, dimy, dimz, rowpad, slicepad)
    extent = (dimz - 1) * pitch_z + (dimy - 1) * pitch_y + (dimx - 1) * stride + nf
    at = lead + first
    numel = at + extent + 7
    g = torch.Generator(device="cpu").manual_seed(1000 * stride + 10 * dimx + nf)
    vals = torch.randn((nf, dimz, dimy, dimx), generator=g, dtype=torch.float64).to(dtype).cuda()
    # gather: the parent holds the values where torch's indexing puts them, the sentinel elsewhere
    parent = sentinel_parent(numel, dtype)
    view = fields_view(parent, at, nf, (dimz, dimy, dimx), stride, pitch_y, pitch_z)
    view.copy_(vals.permute(1, 2, 3, 0))
    before = parent.clone()
    stacked = eng.fields_gather(view)
    assert same_bits(stacked, vals), "gathered volumes differ"
    assert same_bits(parent, before), "the gather wrote its source"
    # scatter: into a parent of the sentinel; the whole parent is then the one above, the sentinel included
    target = sentinel_parent(numel, dtype)
    eng.fields_scatter(vals, fields_view(target, at, nf, (dimz, dimy, dimx), stride, pitch_y, pitch_z))
    assert same_bits(target, before), "the scatter differs, or wrote an element that is no selected field"


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_profiler_shows_the_form_that_ran(eng, dt):
    import torch
    dtype = getattr(torch, dt)
    dimx, dimy, dimz, stride = TILE + 8, 2, 2, 4
    vals = torch.randn((stride, dimz, dimy, dimx), dtype=torch.float64).to(dtype).cuda()

    def forms(names, kernel):
        return {f for f in ("true", "false") if any(f"{kernel}<T, {f}>" in k for k in names)}

    for lead, want in ((0, "true"), (1, "false")):
        parent = sentinel_parent(lead + stride * vals[0].numel() + 3, dtype)
        view = fields_view(parent, lead, stride, (dimz, dimy, dimx), stride, dimx * stride, dimx * dimy * stride)
        view.copy_(vals.permute(1, 2, 3, 0))
        got, names = launched(eng, lambda: eng.fields_gather(view))
        assert same_bits(got, vals) and forms(names, "k_fields_gather") == {want}, names
        target = sentinel_parent(parent.numel(), dtype)
        tv = fields_view(target, lead, stride, (dimz, dimy, dimx), stride, dimx * stride, dimx * dimy * stride)
        _, names = launched(eng, lambda: eng.fields_scatter(vals, tv))
        assert same_bits(target, parent) and forms(names, "k_fields_scatter") == {want}, names
    # a subset of an aligned record: the gather may load packs, the scatter must not store them
    parent = sentinel_parent(stride * vals[0].numel(), dtype)
    view = fields_view(parent, 0, 2, (dimz, dimy, dimx), stride, dimx * stride, dimx * dimy * stride)
    view.copy_(vals[:2].permute(1, 2, 3, 0))
    got, names = launched(eng, lambda: eng.fields_gather(view))
    assert same_bits(got, vals[:2]) and forms(names, "k_fields_gather") == {"true"}, names
    target = sentinel_parent(parent.numel(), dtype)
    tv = fields_view(target, 0, 2, (dimz, dimy, dimx), stride, dimx * stride, dimx * dimy * stride)
    _, names = launched(eng, lambda: eng.fields_scatter(vals[:2].contiguous(), tv))
    assert same_bits(target, parent) and forms(names, "k_fields_scatter") == {"false"}, names


# ---- end to end ---------------------------------------------------------------------------------------------------
SHAPE, CHUNKS = (30, 44, 37), (32, 32, 32)
QUALITY = {1: 2.5, 2: 70.0, 3: 1e-3}


@pytest.fixture(scope="module")
def three_fields():
    """{dtype name: numpy (3, z, y, x)}: turbulence, the same a hundred times as large, a constant"""
    t = turbulence(SHAPE, dtype=np.float64)
    out = {}
    for dt in (np.float32, np.float64):
        out[np.dtype(dt).name] = np.stack([t.astype(dt), (100.0 * t).astype(dt), np.full(SHAPE, 2.75, dtype=dt)])
    return out


@pytest.fixture(scope="module")
def oracle_containers(oracle, three_fields):
    """{(dtype name, mode): [container bytes of every packed field]}, computed once"""
    return {(dt, mode): [oracle.comp_3d(v[f], CHUNKS, mode, q) for f in range(3)]
            for dt, v in three_fields.items() for mode, q in QUALITY.items()}


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_compress_fields_equals_the_oracle_on_every_packed_field(eng, three_fields, oracle_containers, dt, mode):
    import torch
    v = three_fields[dt]
    inter = torch.from_numpy(np.ascontiguousarray(v.transpose(1, 2, 3, 0))).cuda()   # (z, y, x, 3)
    before = inter.clone()
    got = eng.compress_fields(inter, CHUNKS, QUALITY[mode], mode=mode)
    assert len(got) == 3
    for f in range(3):
        assert bytes(got[f].cpu().numpy()) == oracle_containers[(dt, mode)][f], f"container of field {f} differs"
    assert same_bits(inter, before)
    # ... and fields 1..2 of it alone, read where they lie
    sub = eng.compress_fields(inter[..., 1:3], CHUNKS, QUALITY[mode], mode=mode)
    assert [bytes(c.cpu().numpy()) for c in sub] == oracle_containers[(dt, mode)][1:3]


def _halo_fields_parent(nrec, dtype, lo=(1, 2, 3), hi=(1, 2, 4)):
    """(1-D sentinel parent, its (z, y, x, nrec) tensor, the interior of SHAPE inside the halo)"""
    shape = tuple(a + n + b for a, n, b in zip(lo, SHAPE, hi)) + (nrec,)
    parent = sentinel_parent(int(np.prod(shape)), dtype)
    whole = parent.view(shape)
    return parent, whole, whole[tuple(slice(a, a + n) for a, n in zip(lo, SHAPE))]


def test_decompress_fields_into_two_of_four_fields_of_a_halo_parent(eng, oracle_containers):
    """containers of different modes and precisions, decoded as fp32 into fields 1..2: each is decompress() of its
    container, and fields 0 and 3 and the halo are untouched"""
    import torch
    cs = [to_dev(oracle_containers[("float32", 1)][0]), to_dev(oracle_containers[("float64", 3)][1])]
    parent, _, interior = _halo_fields_parent(4, torch.float32)
    out = interior[..., 1:3]
    assert eng.decompress_fields(cs, out=out) is out
    want_parent, _, want_interior = _halo_fields_parent(4, torch.float32)
    for f, c in enumerate(cs):
        want_interior[..., 1 + f].copy_(eng.decompress(c, output_float=True))
    assert same_bits(parent, want_parent)
    # out=None: a contiguous (z, y, x, c) tensor
    made = eng.decompress_fields(cs)
    assert made.is_contiguous() and tuple(made.shape) == SHAPE + (2,) and same_bits(made, want_interior[..., 1:3])


def test_decompress_fields_at_field_dim_0_into_channels_last(eng, oracle_containers):
    import torch
    cs = [to_dev(c) for c in oracle_containers[("float64", 2)]]
    parent = sentinel_parent(3 * int(np.prod(SHAPE)), torch.float64)
    nchw = parent.view(SHAPE + (3,)).permute(3, 0, 1, 2)   # (c, z, y, x) with the channels innermost in memory
    eng.decompress_fields(cs, out=nchw, field_dim=0, output_float=False)
    for f, c in enumerate(cs):
        assert same_bits(nchw[f], eng.decompress(c, output_float=False)), f
    got = eng.compress_fields(nchw, CHUNKS, QUALITY[1], field_dim=0)
    want = eng.compress_batch(nchw.contiguous(), CHUNKS, QUALITY[1])
    assert [bytes(c.cpu().numpy()) for c in got] == [bytes(c.cpu().numpy()) for c in want]


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_quality_fields_equals_quality_on_packed_copies(eng, three_fields, oracle_containers, dt):
    import torch
    dtype = getattr(torch, dt)
    v = three_fields[dt]
    _, _, orig = _halo_fields_parent(5, dtype)
    orig = orig[..., 1:4]
    orig.copy_(torch.from_numpy(np.ascontiguousarray(v.transpose(1, 2, 3, 0))).cuda())
    cs = [to_dev(c) for c in oracle_containers[(dt, 1)]]
    recon = eng.decompress_fields(cs, output_float=dt == "float32")   # (dense, another layout than orig's)
    got = eng.quality_fields(orig, recon)
    assert len(got) == 3
    for f in range(3):
        want = eng.quality(orig[..., f].contiguous(), recon[..., f].contiguous())
        a = np.array([getattr(got[f], k) for k in ("rmse", "linfty", "psnr", "min", "max", "mean", "var", "mse")])
        b = np.array([getattr(want, k) for k in ("rmse", "linfty", "psnr", "min", "max", "mean", "var", "mse")])
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (f, a, b)


# ---- refusals and launches ----------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_as_it_was(eng, oracle_containers):
    import torch
    from sperr_amd.api import Fields, SperrHipError
    lib = eng.lib
    dz, dy, dx = SHAPE
    cs = [to_dev(c) for c in oracle_containers[("float32", 1)][:2]]
    src = torch.cat(cs)
    offs = (_sz * 3)(0, cs[0].numel(), cs[0].numel() + cs[1].numel())
    parent, _, interior = _halo_fields_parent(4, torch.float32)
    out = interior[..., 1:3]
    good, nf, _ = eng.fields_of(out)
    before = parent.clone()
    room = eng._room_bytes(out)
    extent = (dz - 1) * good.pitch_z + (dy - 1) * good.pitch_y + (dx - 1) * good.stride_x + nf

    def decode(lay, nfields=2, cap=room, dims=(dx, dy, dz)):
        return lib.sperrhip_decompress_fields_dev(src.data_ptr(), offs, nfields, 1, *dims, out.data_ptr(), C.byref(lay),
                                                  cap, None)

    assert decode(Fields(1, good.pitch_y, good.pitch_z)) == -1                       # nfields > stride_x
    assert decode(Fields(good.stride_x, dx * good.stride_x - 1, good.pitch_z)) == -1   # a short row pitch
    assert decode(Fields(good.stride_x, good.pitch_y, good.pitch_y * dy - 1)) == -1    # a short slice pitch
    assert decode(good, cap=extent * 4 - 1) == -1                                    # an output below the extent
    assert decode(good, dims=(dx, dy, dz + 1), cap=1 << 40) == -1                    # dims that differ from a container's
    assert decode(good, dims=(dy, dx, dz)) == -1
    torch.cuda.synchronize()
    assert same_bits(parent, before), "a refused decode wrote"
    assert decode(good, cap=extent * 4) == 0                                        # ... and the extent exactly is enough
    torch.cuda.synchronize()
    assert not same_bits(parent, before)

    # the same refusals of the compressor and the stage calls, before anything is launched
    cap = eng.max_compressed_size_batch(2, SHAPE, CHUNKS, 2.5)
    cbuf = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    offs2 = (_sz * 3)()
    for lay in (Fields(1, good.pitch_y, good.pitch_z), Fields(good.stride_x, dx * good.stride_x - 1, good.pitch_z)):
        rtn, names = launched(eng, lambda: lib.sperrhip_compress_fields_dev(
            out.data_ptr(), C.byref(lay), 2, 1, dx, dy, dz, *CHUNKS, 1, 2.5, cbuf.data_ptr(), cap, offs2, None))
        assert rtn == -1 and not names, names
        stacked = torch.full((2,) + SHAPE, 7.0, dtype=torch.float32, device="cuda")
        assert lib.sperrhip_fields_gather_dev(out.data_ptr(), C.byref(lay), 2, 1, dx, dy, dz, stacked.data_ptr(),
                                              stacked.numel() * 4, None) == -1
        assert bool((stacked == 7.0).all())
    assert bool((cbuf == 0xA5).all())
    assert lib.sperrhip_fields_gather_dev(out.data_ptr(), C.byref(good), 2, 1, dx, dy, dz, stacked.data_ptr(),
                                          stacked.numel() * 4 - 1, None) == -1           # a stacked buffer too small
    assert bool((stacked == 7.0).all())

    # Python: a field axis that is not innermost in memory, a record narrower than the fields, the calls that take none
    t = torch.zeros((3,) + SHAPE, dtype=torch.float32, device="cuda")
    with pytest.raises(SperrHipError):
        eng.fields_of(t.permute(1, 2, 3, 0))            # planar: the field stride is a volume
    with pytest.raises(SperrHipError):
        eng.fields_of(torch.zeros(SHAPE + (4,), device="cuda")[..., ::2])
    with pytest.raises(SperrHipError):
        eng.fields_of(torch.zeros(SHAPE + (4,), device="cuda").permute(0, 2, 1, 3))   # rows and x exchanged: they overlap
    with pytest.raises(SperrHipError):
        eng.compress_fields(torch.zeros(SHAPE, device="cuda"), CHUNKS, 2.5)
    inter = torch.zeros(SHAPE + (2,), dtype=torch.float32, device="cuda")
    with pytest.raises(SperrHipError):
        eng.compress(inter[..., 0], CHUNKS, 2.5)        # (an x stride of 2: still no view)
    with pytest.raises(SperrHipError):
        eng.compress_batch(inter.permute(3, 0, 1, 2), CHUNKS, 2.5)
    with pytest.raises(SperrHipError):
        eng.decompress_fields(cs, out=interior[..., 1:4])   # two containers, three fields


def test_compress_batch_launches_no_fields_kernel(eng, three_fields):
    import torch
    vols = torch.from_numpy(three_fields["float32"]).cuda()
    _, names = launched(eng, lambda: eng.compress_batch(vols, CHUNKS, 2.5))
    assert names and not any("k_fields_" in k for k in names), names
    inter = vols.permute(1, 2, 3, 0).contiguous()
    _, names2 = launched(eng, lambda: eng.compress_fields(inter, CHUNKS, 2.5))
    assert sum(n for k, n in names2.items() if "k_fields_gather" in k) == 1
    assert {k: n for k, n in names2.items() if "k_fields_" not in k} == names
