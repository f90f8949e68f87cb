"""GPU: one level of a 3D container's resolution hierarchy, whole or a box of it
(sperrhip_decompress_level_dev, sperrhip_decomp_3d_level).

The expected values are always the oracle's hierarchy, oracle.decomp_3d_multi_res(container)[1][h], cut to the
box with numpy and narrowed with astype(float32) for float output -- never the library's own multires call.  All
compares are on the bit patterns.  Beside parity the tests pin that a level call does only the level's work: no
other chunk's stream and no outlier stream is read, the finest level's kernels, the scatter pass and the outlier
kernels are not launched, and the calls that existed before launch what they launched."""
import ctypes as C

import numpy as np
import pytest

from fields import smooth_field
from outlier_cases import outlier_start
from sperr_amd import api
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu
_sz = C.c_size_t


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    return SperrHip()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_of(container):
    return cuda(np.frombuffer(container, dtype=np.uint8))


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def crop(full, lo, dims):
    return np.ascontiguousarray(full[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]])


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def as_out(level, of):
    """the level as the call hands it out: doubles, or floats each narrowed once (round to nearest)"""
    return level.astype(np.float32) if of else level


def make(eng, v, ch, q, mode=1):
    return bytes(eng.compress(cuda(v), ch, q, mode=mode).cpu().numpy())


def xyz(a):
    return (a.shape[2], a.shape[1], a.shape[0])


def grid_of(vol, ch):
    return tuple(vol[a] // ch[a] for a in range(3))


def boxes_for(ld, grid):
    """(lo, dims), x y z order, in the coordinates of a level of dims `ld` made of `grid` chunk corners: the whole
    level, one sample at the far corner, a box with odd origins that straddles the first chunk corner on every axis
    that has one, a box inside the last chunk's corner"""
    r = tuple(ld[a] // grid[a] for a in range(3))
    out = [((0, 0, 0), tuple(ld)), (tuple(d - 1 for d in ld), (1, 1, 1))]
    lo, dims = [], []
    for a in range(3):
        if grid[a] > 1:
            l = r[a] - 1 if (r[a] - 1) % 2 == 1 else (r[a] - 3 if r[a] >= 3 else r[a] - 1)
            d = min(ld[a] - l, (r[a] - l) + min(r[a], 3))
            assert l + d > r[a] > l   # on both sides of the corner
        else:
            l = 1 if ld[a] > 1 else 0
            d = max(1, ld[a] - l - 1)
        lo.append(l)
        dims.append(d)
    out.append((tuple(lo), tuple(dims)))
    lo = tuple(ld[a] - r[a] + (1 if r[a] > 2 else 0) for a in range(3))
    out.append((lo, tuple(max(1, r[a] - 2) for a in range(3))))
    return out


def check_levels(eng, oracle, container, vol, ch, boxes=True):
    """every level, both output types: the whole level, and the boxes"""
    want_levels = oracle.decomp_3d_multi_res(container)[1]
    assert len(want_levels) > 0
    assert eng.multires_levels((vol[2], vol[1], vol[0]), ch) == [lv.shape for lv in want_levels]
    dev = dev_of(container)
    grid = grid_of(vol, ch)
    for h, lv in enumerate(want_levels):
        for of in (False, True):
            want = as_out(lv, of)
            got = eng.decompress_level(dev, h, output_float=of).cpu().numpy()
            assert same(got, want), (vol, ch, h, of)
            if not boxes:
                continue
            for lo, dims in boxes_for(xyz(lv), grid):
                got = eng.decompress_level(dev, h, lo, dims, output_float=of).cpu().numpy()
                assert same(got, crop(want, lo, dims)), (vol, ch, h, of, lo, dims)
    return want_levels


# ---- parity -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,chunks", [((64, 64, 64), (32, 32, 32)), ((48, 64, 32), (32, 32, 24)),
                                          ((40, 40, 40), (40, 40, 40)), ((128, 128, 128), (128, 128, 128))])
def test_level_parity_multires_shapes(eng, oracle, shape, chunks):
    """the shapes of test_gpu_parity.py::test_multi_resolution_decode, with its constant chunk"""
    v = turbulence(shape)
    v[: shape[0] // 2, : chunks[1], : chunks[0]] = 0.25
    check_levels(eng, oracle, oracle.comp_3d(v, chunks, 1, 3.0), xyz(v), chunks)


def test_level_parity_two_256_chunks(eng, oracle):
    """256^3 chunks take the fused passes in the compact buffer; the finest of their levels is the plain decode
    without its last kernel"""
    v = turbulence((256, 256, 512))
    levels = check_levels(eng, oracle, make(eng, v, (256, 256, 256), 2.0), xyz(v), (256, 256, 256))
    assert levels[-1].shape == (128, 128, 256)


@pytest.mark.parametrize("tol", [2e-2, 1e-4])
def test_level_parity_pwe(eng, oracle, tol):
    """the container of test_pwe_container_through_both_inverse_paths: a level is taken before the correctors are
    added, so the levels are the same with every outlier stream overwritten"""
    v = turbulence((64, 128, 128))
    c = oracle.comp_3d(v, (64, 64, 64), 3, tol)
    want_levels = check_levels(eng, oracle, c, xyz(v), (64, 64, 64))
    offs, lens = chunk_table(c, 4)
    rng = np.random.default_rng(3)
    bad, tails = bytearray(c), 0
    for o, n in zip(offs, lens):
        first = outlier_start(c[o:o + n])
        if first is not None:
            bad[o + first:o + n] = rng.integers(0, 256, n - first, dtype=np.uint8).tobytes()
            tails += 1
    assert tails > 0 and bytes(bad) != c
    dev = dev_of(bytes(bad))
    for h, lv in enumerate(want_levels):
        for of in (False, True):
            assert same(eng.decompress_level(dev, h, output_float=of).cpu().numpy(), as_out(lv, of)), (h, of)


def test_level_parity_truncated(eng, oracle):
    v = turbulence((64, 64, 64))
    c = eng.trunc_3d(make(eng, v, (32, 32, 32), 4.0), 40)
    check_levels(eng, oracle, c, xyz(v), (32, 32, 32))


def test_level_parity_fp64(eng, oracle):
    v = smooth_field((32, 48, 48), dtype=np.float64)
    check_levels(eng, oracle, make(eng, v, (16, 16, 16), 3.0), xyz(v), (16, 16, 16))


def test_level_parity_psnr_wide_coefficients(eng, oracle):
    v = smooth_field((32, 32, 64), dtype=np.float64)
    v[:, :, :32] = 0.75
    c = make(eng, v, (32, 32, 32), 230.0, mode=2)
    assert c[20 + 8 + 17 + 17] > 32   # the second chunk has more than 32 bit planes
    check_levels(eng, oracle, c, xyz(v), (32, 32, 32))


def test_level_parity_sub_batches(eng, oracle):
    v = turbulence((128, 128, 128))
    check_levels(eng, oracle, make(eng, v, (16, 16, 16), 2.0), (128, 128, 128), (16, 16, 16))


# ---- only the level's work ------------------------------------------------------------------------------------------

def chunk_table(container, nch):
    lens = np.frombuffer(container, dtype=np.uint32, count=nch, offset=20)
    offs = 20 + 4 * nch + np.concatenate([[0], np.cumsum(lens.astype(np.int64))[:-1]])
    return [int(o) for o in offs], [int(n) for n in lens]


@pytest.mark.parametrize("mode,q", [(1, 2.0), (3, 1e-3)])
def test_level_reads_only_its_chunks_and_no_outlier_stream(eng, oracle, mode, q):
    """Every byte of every chunk stream outside the box's chunks is garbage (the length table is kept), and so is
    every byte of the outlier streams behind the kept chunks' SPECK streams."""
    v = turbulence((64, 128, 128))
    ch = (32, 32, 32)
    vol, grid = xyz(v), (4, 4, 2)
    clean = make(eng, v, ch, q, mode=mode)
    want_levels = oracle.decomp_3d_multi_res(clean)[1]
    assert len(want_levels) > 0
    nch = grid[0] * grid[1] * grid[2]
    offs, lens = chunk_table(clean, nch)
    rng = np.random.default_rng(11)
    tails = 0
    for h, lv in enumerate(want_levels):
        ld = xyz(lv)
        r = tuple(ld[a] // grid[a] for a in range(3))
        for lo, dims in boxes_for(ld, grid)[1:] + [((0, 0, 0), (1, 1, 1)), ((r[0], r[1], 0), (r[0], r[1], r[2]))]:
            keep = set(api.box_chunks(eng.lib, ld, r, lo, dims))
            assert 0 < len(keep) < nch
            bad = bytearray(clean)
            for i in range(nch):
                first = 0
                if i in keep:
                    first = outlier_start(clean[offs[i]:offs[i] + lens[i]])
                    if first is None:
                        continue
                    tails += 1
                bad[offs[i] + first:offs[i] + lens[i]] = rng.integers(0, 256, lens[i] - first, dtype=np.uint8).tobytes()
            bad = bytes(bad)
            assert bad != clean
            for of in (False, True):
                want = crop(as_out(lv, of), lo, dims)
                got = eng.decompress_level(dev_of(bad), h, lo, dims, output_float=of).cpu().numpy()
                assert same(got, want), (h, lo, dims, of)
                assert same(eng.decomp_3d_level(bad, h, lo, dims, output_float=of), want), (h, lo, dims, of)
    assert (tails > 0) == (mode == 3)   # the point-wise-error container had outlier streams to overwrite


def profile_names(eng, fn):
    import torch
    torch.cuda.synchronize()
    eng.profile(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {k: n for k, (_, n) in eng.profile_report().items() if n > 0}
    finally:
        eng.profile(False)


@pytest.mark.parametrize("mode,q,shape,ch", [(1, 2.0, (64, 64, 64), (32, 32, 32)),
                                             (3, 1e-3, (64, 128, 128), (64, 64, 64)),
                                             (1, 2.0, (256, 256, 256), (256, 256, 256))])
def test_level_launches_only_the_levels_kernels(eng, oracle, mode, q, shape, ch):
    v = turbulence(shape)
    dev = dev_of(make(eng, v, ch, q, mode=mode))
    nlev = len(eng.multires_levels(shape, ch))
    assert nlev > 0
    plain = profile_names(eng, lambda: eng.decompress(dev, False))
    if mode == 3:   # (the plain decode of this container does decode outliers: the check below can fail)
        assert any("outlier" in k or "speck1d" in k for k in plain)
    for h in range(nlev):
        for box in (None, ((1, 1, 1), (1, 1, 1))):
            lo, dims = box if box else (None, None)
            rep = profile_names(eng, lambda: eng.decompress_level(dev, h, lo, dims))
            assert any("k_level_write" in k for k in rep), rep
            for k in rep:
                assert "k_lift_xy" not in k, (h, k)   # (k_lift_xyz_inv as well)
                assert "k_scatter_uncondition" not in k, (h, k)
                assert "outlier" not in k and "speck1d" not in k, (h, k)
                assert "k_sub_volume" not in k, (h, k)
            # the passes of the h levels coarser than the level, and one writer, per sub-batch
            lifts = sum(n for k, n in rep.items() if "k_lift_axis" in k)
            writers = sum(n for k, n in rep.items() if "k_level_write" in k)
            assert lifts == 3 * h * writers, (h, rep)
            assert any("k_dequant_corner" in k for k in rep) == (h == 0), (h, rep)


def test_level_exact_output_size_suffices(eng, oracle):
    import torch
    v = turbulence((64, 64, 64))
    c = oracle.comp_3d(v, (32, 32, 32), 1, 3.0)
    dev = dev_of(c)
    want_levels = oracle.decomp_3d_multi_res(c)[1]
    assert len(want_levels) > 0
    for h, lv in enumerate(want_levels):
        for of in (False, True):
            esz = 4 if of else 8
            dt = torch.float32 if of else torch.float64
            ld = xyz(lv)
            for lo, dims in [(None, ld), ((1, 0, 1), (ld[0] - 1, ld[1], 1))]:
                n = dims[0] * dims[1] * dims[2]
                out = torch.full((n + 16,), 7.0, dtype=dt, device="cuda")
                rc = eng.lib.sperrhip_decompress_level_dev(dev.data_ptr(), dev.numel(), int(of), h,
                                                           (_sz * 3)(*lo) if lo else None,
                                                           (_sz * 3)(*dims) if lo else None, out.data_ptr(), n * esz,
                                                           None)
                assert rc == 0
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                want = as_out(lv, of) if lo is None else crop(as_out(lv, of), lo, dims)
                assert np.array_equal(bits(got[:n]), bits(want.reshape(-1)))
                assert (got[n:] == 7.0).all(), "the call wrote past the capacity it was given"


# Launches (kernel name -> count) of the three calls that existed before, on the container of
# test_level_exact_output_size_suffices, measured with the library built from the parent commit
# 84c7dc6 ("Retire the quadtree-walk 2D coder; slices always use the 2D forest").
PARENT_LAUNCHES = {
    "decompress": {
        "(k_lift_axis<false, 0>)": 12, "(k_lift_xyz_inv<2, true>)": 4, "k_dec_count": 72, "k_dec_header": 4,
        "k_dec_live": 8, "k_dec_load_words": 4, "k_dec_plane_end": 72, "k_dec_scan": 72, "k_gather_heads": 1,
        "k_leaf_apply": 72, "k_lip_apply<uint32_t>": 72, "k_lip_deposit": 72, "k_lip_scan": 72, "k_lip_words": 72,
        "k_lis_compact": 72, "k_lis_hi<uint32_t>": 72, "k_lis_l0": 72, "k_lis_l1": 72, "k_lis_l2": 72,
        "k_place_scan": 72, "k_place_scatter": 72, "k_ref_assemble": 4, "k_ref_deposit": 72,
    },
    "decompress_box": {
        "(k_lift_axis<false, 0>)": 6, "(k_lift_xyz_inv<2, true, true>)": 2, "k_dec_count": 36, "k_dec_header": 2,
        "k_dec_live": 4, "k_dec_load_words": 2, "k_dec_plane_end": 36, "k_dec_scan": 36, "k_gather_heads": 1,
        "k_leaf_apply": 36, "k_lip_apply<uint32_t>": 36, "k_lip_deposit": 36, "k_lip_scan": 36, "k_lip_words": 36,
        "k_lis_compact": 36, "k_lis_hi<uint32_t>": 36, "k_lis_l0": 36, "k_lis_l1": 36, "k_lis_l2": 36,
        "k_place_scan": 36, "k_place_scatter": 36, "k_ref_assemble": 2, "k_ref_deposit": 36,
    },
    "decompress_multires": {
        "(k_lift_axis<false, 0>)": 12, "(k_lift_xyz_inv<2, false>)": 4, "k_dec_count": 72, "k_dec_header": 4,
        "k_dec_live": 8, "k_dec_load_words": 4, "k_dec_plane_end": 72, "k_dec_scan": 72, "k_gather_heads": 1,
        "k_inv_quantize<uint32_t>": 4, "k_leaf_apply": 72, "k_lip_apply<uint32_t>": 72, "k_lip_deposit": 72,
        "k_lip_scan": 72, "k_lip_words": 72, "k_lis_compact": 72, "k_lis_hi<uint32_t>": 72, "k_lis_l0": 72,
        "k_lis_l1": 72, "k_lis_l2": 72, "k_place_scan": 72, "k_place_scatter": 72, "k_ref_assemble": 4,
        "k_ref_deposit": 72, "k_sub_volume": 8,
    },
}


def test_existing_calls_launch_what_they_launched(eng, oracle):
    import torch
    v = turbulence((64, 64, 64))
    dev = dev_of(oracle.comp_3d(v, (32, 32, 32), 1, 3.0))
    out = torch.empty((64, 64, 64), dtype=torch.float64, device="cuda")
    got = {
        "decompress": profile_names(eng, lambda: eng.decompress(dev, False, out=out, shape_zyx=(64, 64, 64))),
        "decompress_box": profile_names(eng, lambda: eng.decompress_box(dev, (5, 6, 7), (40, 30, 20),
                                                                        output_float=False)),
        "decompress_multires": profile_names(eng, lambda: eng.decompress_multires(dev, output_float=False)),
    }
    for call, rep in got.items():
        print(call, sum(rep.values()), rep)
    assert got == PARENT_LAUNCHES


# Launches of five more kinds of call, measured the same way with the library built from the parent commit
# 7d7e4b1 ("Quantise, build the leaf pyramid level and take the census in one kernel"): a level and a box of a
# level of that container, a batch of two such containers, and slices of 96 x 80 at 2 bits per value -- one,
# and a batch of three with their headers.
PARENT_LAUNCHES_MORE = {
    "decompress_level_0": {
        "(k_level_write<T, false>)": 4, "k_dec_count": 72, "k_dec_header": 4, "k_dec_live": 8,
        "k_dec_load_words": 4, "k_dec_plane_end": 72, "k_dec_scan": 72, "k_dequant_corner": 4,
        "k_gather_heads": 1, "k_leaf_apply": 72, "k_lip_apply<uint32_t>": 72, "k_lip_deposit": 72,
        "k_lip_scan": 72, "k_lip_words": 72, "k_lis_compact": 72, "k_lis_hi<uint32_t>": 72, "k_lis_l0": 72,
        "k_lis_l1": 72, "k_lis_l2": 72, "k_place_scan": 72, "k_place_scatter": 72, "k_ref_assemble": 4,
        "k_ref_deposit": 72,
    },
    "decompress_level_last_box": {
        "(k_level_write<T, true>)": 1, "(k_lift_axis<false, 0>)": 3, "k_dec_count": 18, "k_dec_header": 1,
        "k_dec_live": 2, "k_dec_load_words": 1, "k_dec_plane_end": 18, "k_dec_scan": 18, "k_gather_heads": 1,
        "k_leaf_apply": 18, "k_lip_apply<uint32_t>": 18, "k_lip_deposit": 18, "k_lip_scan": 18, "k_lip_words": 18,
        "k_lis_compact": 18, "k_lis_hi<uint32_t>": 18, "k_lis_l0": 18, "k_lis_l1": 18, "k_lis_l2": 18,
        "k_place_scan": 18, "k_place_scatter": 18, "k_ref_assemble": 1, "k_ref_deposit": 18,
    },
    "decompress_batch": {
        "(k_lift_axis<false, 0>)": 12, "(k_lift_xyz_inv<2, true>)": 4, "k_dec_count": 72, "k_dec_header": 4,
        "k_dec_live": 8, "k_dec_load_words": 4, "k_dec_plane_end": 72, "k_dec_scan": 72, "k_gather_bytes": 1,
        "k_gather_heads": 2, "k_leaf_apply": 72, "k_lip_apply<uint32_t>": 72, "k_lip_deposit": 72,
        "k_lip_scan": 72, "k_lip_words": 72, "k_lis_compact": 72, "k_lis_hi<uint32_t>": 72, "k_lis_l0": 72,
        "k_lis_l1": 72, "k_lis_l2": 72, "k_place_scan": 72, "k_place_scatter": 72, "k_ref_assemble": 4,
        "k_ref_deposit": 72,
    },
    "decompress_2d": {
        "(k_lift_axis<false, 0>)": 6, "(k_lift_xy<false, 2>)": 1, "k_dec_count": 18, "k_dec_header": 1,
        "k_dec_live": 2, "k_dec_load_words": 1, "k_dec_plane_end": 18, "k_dec_scan": 18, "k_gather_heads": 1,
        "k_inv_quantize<uint32_t>": 1, "k_leaf_apply": 18, "k_lip_apply<uint32_t>": 18, "k_lip_deposit": 18,
        "k_lip_scan": 18, "k_lip_words": 18, "k_lis_compact": 18, "k_lis_mx<false>": 18, "k_place_scan": 18,
        "k_place_scatter": 18, "k_ref_assemble": 1, "k_ref_deposit": 18,
    },
    "decompress_2d_batch": {
        "(k_lift_axis<false, 0>)": 6, "(k_lift_xy<false, 2>)": 1, "k_dec_count": 18, "k_dec_header": 1,
        "k_dec_live": 2, "k_dec_load_words": 1, "k_dec_plane_end": 18, "k_dec_scan": 18, "k_gather_heads": 2,
        "k_inv_quantize<uint32_t>": 1, "k_leaf_apply": 18, "k_lip_apply<uint32_t>": 18, "k_lip_deposit": 18,
        "k_lip_scan": 18, "k_lip_words": 18, "k_lis_compact": 18, "k_lis_mx<false>": 18, "k_place_scan": 18,
        "k_place_scatter": 18, "k_ref_assemble": 1, "k_ref_deposit": 18,
    },
}


def test_more_calls_launch_what_they_launched(eng, oracle):
    dev = [dev_of(oracle.comp_3d(turbulence((64, 64, 64), seed=s), (32, 32, 32), 1, 3.0)) for s in (42, 7)]
    nlev = len(eng.multires_levels((64, 64, 64), (32, 32, 32)))
    assert nlev > 0
    imgs = [turbulence((1, 80, 96), seed=s)[0] for s in (1, 2, 3)]
    one = dev_of(oracle.comp_2d(imgs[0], 1, 2.0, False))
    three = [dev_of(oracle.comp_2d(img, 1, 2.0, True)) for img in imgs]
    got = {
        "decompress_level_0": profile_names(eng, lambda: eng.decompress_level(dev[0], 0)),
        "decompress_level_last_box": profile_names(eng, lambda: eng.decompress_level(dev[0], nlev - 1, (1, 1, 1),
                                                                                     (1, 1, 1))),
        "decompress_batch": profile_names(eng, lambda: eng.decompress_batch(dev, output_float=False)),
        "decompress_2d": profile_names(eng, lambda: eng.decompress_2d(one, (80, 96), output_float=False)),
        "decompress_2d_batch": profile_names(eng, lambda: eng.decompress_2d_batch(three, (80, 96), output_float=False,
                                                                                  header=True)),
    }
    for call, rep in got.items():
        print(call, sum(rep.values()), rep)
    assert got == PARENT_LAUNCHES_MORE


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_level_refusals_leave_the_output_and_engine_alone(eng, oracle):
    import torch
    v = turbulence((64, 64, 64))
    c = oracle.comp_3d(v, (32, 32, 32), 1, 3.0)
    dev = dev_of(c)
    nlev = len(eng.multires_levels((64, 64, 64), (32, 32, 32)))
    assert nlev > 0
    ld = tuple(d // 2 for d in (64, 64, 64))   # the finest level
    sentinel = torch.full((64 * 64 * 64,), 7.0, dtype=torch.float64, device="cuda")
    lib = eng.lib

    def call(d, level, lo, dims, cap, of=0):
        rc = lib.sperrhip_decompress_level_dev(d.data_ptr(), d.numel(), of, level, (_sz * 3)(*lo) if lo else None,
                                               (_sz * 3)(*dims) if dims else None, sentinel.data_ptr(), cap, None)
        torch.cuda.synchronize()
        assert bool((sentinel == 7.0).all()), "a refused call wrote to its output"
        return rc

    big = sentinel.numel() * 8
    assert call(dev, nlev, None, None, big) == -1                              # level equal to nlev
    assert call(dev, nlev, (0, 0, 0), (1, 1, 1), big) == -1
    assert call(dev, nlev - 1, (0, 0, 0), (0, 4, 4), big) == -1                # a zero extent
    assert call(dev, nlev - 1, (ld[0] - 1, 0, 0), (2, 1, 1), big) == -1        # a box leaving the level
    assert call(dev, nlev - 1, (0, 0, ld[2]), (1, 1, 1), big) == -1
    l0 = eng.multires_levels((64, 64, 64), (32, 32, 32))[0]
    assert call(dev, 0, (0, 0, 0), (l0[2] + 1, 1, 1), big) == -1               # (the box fits a finer level, not this one)
    assert call(dev, nlev - 1, None, None, ld[0] * ld[1] * ld[2] * 8 - 8) == -1   # a capacity one value short
    assert call(dev, nlev - 1, None, None, ld[0] * ld[1] * ld[2] * 4 - 4, of=1) == -1
    assert call(dev, nlev - 1, (1, 1, 1), (3, 3, 3), 27 * 8 - 8) == -1
    assert call(dev, nlev - 1, (0, 0, 0), None, big) == -1                     # half a box
    # containers without levels: not dyadic, and not tiling the volume
    for shape, chunks in [((9, 64, 64), (64, 64, 9)), ((50, 64, 72), (32, 32, 32))]:
        s = oracle.comp_3d(turbulence(shape), chunks, 1, 2.0)
        assert oracle.decomp_3d_multi_res(s)[1] == []
        assert call(dev_of(s), 0, None, None, big) == -1
        assert call(dev_of(s), 0, (0, 0, 0), (1, 1, 1), big) == -1
        with pytest.raises(api.SperrHipError):
            eng.decomp_3d_level(s, 0)
    # damaged containers: refused as sperrhip_decompress_dev refuses them
    for damaged in (c[:len(c) - 1], b"\x07" + c[1:]):
        d = dev_of(damaged)
        with pytest.raises(api.SperrHipError):
            eng.decompress(d, True)
        assert call(d, 0, None, None, big) == -1
        assert call(d, nlev - 1, (0, 0, 0), (4, 4, 4), big) == -1
        with pytest.raises(api.SperrHipError):
            eng.decomp_3d_level(damaged, 0)
    # the host call given *dst != NULL returns 1
    buf = np.frombuffer(c, dtype=np.uint8)
    taken, od = C.c_void_p(1), (_sz * 3)()
    assert lib.sperrhip_decomp_3d_level(buf.ctypes.data, buf.size, 0, 0, None, None, od, C.byref(taken)) == 1
    # the engine still works: a whole decode and a level match the oracle
    assert same(eng.decompress(dev, True).cpu().numpy(), oracle.decomp_3d(c, True))
    want = oracle.decomp_3d_multi_res(c)[1]
    assert same(eng.decompress_level(dev, nlev - 1).cpu().numpy(), want[nlev - 1])


# ---- host and pinned sources ------------------------------------------------------------------------------------------

def test_level_host_path_pageable_and_pinned(eng, oracle):
    import torch
    v = turbulence((64, 128, 128))
    c = make(eng, v, (32, 32, 32), 1e-3, mode=3)
    dev = dev_of(c)
    pinned = torch.empty(len(c), dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[:] = np.frombuffer(c, dtype=np.uint8)
    want_levels = oracle.decomp_3d_multi_res(c)[1]
    assert len(want_levels) > 0
    for h, lv in enumerate(want_levels):
        for lo, dims in [(None, None)] + boxes_for(xyz(lv), (4, 4, 2)):
            for of in (False, True):
                want = eng.decompress_level(dev, h, lo, dims, output_float=of).cpu().numpy()
                assert same(want, as_out(lv, of) if lo is None else crop(as_out(lv, of), lo, dims))
                assert same(eng.decomp_3d_level(c, h, lo, dims, output_float=of), want)
                assert same(eng.decomp_3d_level(pinned.numpy(), h, lo, dims, output_float=of), want)
