"""GPU: every kernel that turns a decoded integer coefficient into a sample (sperr_amd/csrc/dequant.h) still runs in the
call meant for it and still agrees with the oracle bit for bit.

Seven kernels apply the rule on their way: k_ref_assemble (packs the sign into the word), k_lift_xyz_inv and k_lift_axis (the
dequantising inverse passes), k_dequant_corner (level 0), k_inv_quantize (32- and 64-bit, with the decoder's masks and,
inside the encoder's point-wise error stage, without) and k_dec_finish (the stage call).  Each case below is the smallest
input that reaches one of them: it asserts through the engine's own profiler (the names are the ones the launch sites give it)
that the kernel was launched, and compares the result with the oracle's -- decomp_3d, decomp_2d, the levels of
decomp_3d_multi_res, comp_3d, speck3d_decode --, never with another call of the library.

Which coefficient scheme a fixed-rate chunk takes (coef_scheme) depends on the plane its stream runs out on.  Turbulence of
32^3 has 32 planes up to 19.5 bits per value and takes the 64-bit retry (src/SPECK_FLT.cpp:530-538) from 20.0 on, the
(16, 40, 24) chunk from 21.0 on: at 2.0 bits the stream ends far above plane 2 (scheme 2); at 19.5 / 20.5 bits it ends
less than half a bit per value before 32 planes would be complete, inside the passes of plane 0 or 1, each of which takes
nearly a bit per value there (scheme 0: magnitudes, signs and masks read as ever); at 29.5 bits byte 17 of the chunk
stream says 54 / 53 planes and the chunk goes through the 64-bit k_inv_quantize.  A PSNR target of 80 dB gives the 32^3
chunk 14 planes (scheme 1).  scheme_of() pins each of these from the magnitudes the oracle decodes."""
import numpy as np
import pytest

from fields import ramp_field
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu

CUBE, SLAB = (32, 32, 32), (16, 40, 24)   # the fused x-y-z inverse kernel / the per-axis passes (z, y, x)


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


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def xyz(shape_zyx):
    return (shape_zyx[2], shape_zyx[1], shape_zyx[0])


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


def has(rep, name):
    return any(name in k for k in rep)


_containers = {}


def container(oracle, shape, mode, q):
    """the oracle's one-chunk container of turbulence(shape), made once"""
    key = (shape, mode, q)
    if key not in _containers:
        _containers[key] = oracle.comp_3d(turbulence(shape), xyz(shape), mode, q)
    return _containers[key]


def planes(c):
    return c[18 + 17]   # byte 17 of the (only) chunk's stream: the number of bit planes


def scheme_of(oracle, c, shape):
    """coef_scheme of the one chunk of a fixed-rate or PSNR container, from the magnitudes the ORACLE decodes of its
    stream: 1 with at most 31 planes; with 32, a decoded magnitude is m + 2^(q-1) - 1, q the lowest plane the sample was
    refined on -- odd and at least 5 when q >= 2 --, so one even magnitude means that some sample went below plane 2
    (scheme 0), and scheme 2 has every non-zero magnitude odd and none below 5"""
    if planes(c) <= 31:
        return 1
    assert planes(c) == 32
    coef, _ = oracle.speck3d_decode(c[18 + 17:], shape)
    nz = coef[coef != 0]
    if (nz % 2 == 0).any():
        return 0
    assert nz.min() >= 5
    return 2


# (rate, planes of the 32^3 chunk's stream, its scheme; more than 32 planes: the 64-bit retry)
@pytest.mark.parametrize("bpp,nplanes,scheme", [(2.0, 32, 2), (19.5, 32, 0), (29.5, 54, None)])
def test_fused_finest_level_fixed_rate(eng, oracle, bpp, nplanes, scheme):
    c = container(oracle, CUBE, 1, bpp)
    assert planes(c) == nplanes
    assert scheme is None or scheme_of(oracle, c, CUBE) == scheme
    dev = dev_of(c)
    for of in (True, False):
        got, rep = launched(eng, lambda: eng.decompress(dev, of).cpu().numpy())
        print(bpp, of, rep)
        assert has(rep, "k_lift_xyz_inv"), rep
        if nplanes == 32:
            assert has(rep, "k_ref_assemble") and not has(rep, "k_inv_quantize"), rep
        else:
            assert has(rep, "k_inv_quantize<uint64_t>") and not has(rep, "k_inv_quantize<uint32_t>"), rep
        assert not has(rep, "k_dec_finish"), rep
        assert same(got, oracle.decomp_3d(c, of)), (bpp, of)


def test_fused_finest_level_at_most_31_planes(eng, oracle):
    c = container(oracle, CUBE, 2, 80.0)
    assert planes(c) == 14 and scheme_of(oracle, c, CUBE) == 1
    dev = dev_of(c)
    for of in (True, False):
        got, rep = launched(eng, lambda: eng.decompress(dev, of).cpu().numpy())
        print(of, rep)
        assert has(rep, "k_lift_xyz_inv") and has(rep, "k_ref_assemble") and not has(rep, "k_inv_quantize"), rep
        assert same(got, oracle.decomp_3d(c, of)), of


@pytest.mark.parametrize("bpp,nplanes,scheme", [(2.0, 32, 2), (20.5, 32, 0), (29.5, 53, None)])
def test_per_axis_passes_dequantise(eng, oracle, bpp, nplanes, scheme):
    c = container(oracle, SLAB, 1, bpp)
    assert planes(c) == nplanes
    assert scheme is None or scheme_of(oracle, c, SLAB) == scheme
    dev = dev_of(c)
    for of in (True, False):
        got, rep = launched(eng, lambda: eng.decompress(dev, of).cpu().numpy())
        print(bpp, of, rep)
        assert has(rep, "k_lift_axis<false") and not has(rep, "k_lift_xyz_inv"), rep
        # (the 32-bit coefficients have no inverse quantiser pass: the lifting passes are it)
        assert not has(rep, "k_inv_quantize<uint32_t>") and has(rep, "k_inv_quantize<uint64_t>") == (nplanes > 32), rep
        assert same(got, oracle.decomp_3d(c, of)), (bpp, of)


@pytest.mark.parametrize("bpp,scheme", [(2.0, 2), (19.5, 0), (29.5, None)])
def test_level_0_corner(eng, oracle, bpp, scheme):
    c = container(oracle, CUBE, 1, bpp)
    assert scheme is None or scheme_of(oracle, c, CUBE) == scheme
    level0 = oracle.decomp_3d_multi_res(c)[1][0]
    dev = dev_of(c)
    lz, ly, lx = level0.shape
    for lo, dims in ((None, None), ((1, 0, 2), (lx - 2, ly - 1, lz - 3))):
        for of in (True, False):
            got, rep = launched(eng, lambda: eng.decompress_level(dev, 0, lo, dims, output_float=of).cpu().numpy())
            print(bpp, lo, of, rep)
            assert has(rep, "k_dequant_corner") and not has(rep, "k_lift_xyz_inv") and not has(rep, "k_lift_axis"), rep
            want = level0.astype(np.float32) if of else level0
            if lo:
                want = np.ascontiguousarray(want[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]])
            assert same(got, want), (bpp, lo, of)


@pytest.mark.parametrize("bpp", [2.0, 19.5])
def test_inverse_quantiser_with_masks_hierarchy(eng, oracle, bpp):
    c = container(oracle, CUBE, 1, bpp)
    assert planes(c) == 32
    want_vol, want_levels = oracle.decomp_3d_multi_res(c)
    (vol, levels), rep = launched(eng, lambda: eng.decompress_multires(dev_of(c), output_float=False))
    print(bpp, rep)
    assert has(rep, "k_inv_quantize<uint32_t>") and not has(rep, "k_dec_finish"), rep
    assert same(vol.cpu().numpy(), want_vol)
    assert len(levels) == len(want_levels) > 0
    for lv, want in zip(levels, want_levels):
        assert same(lv.cpu().numpy(), want)


@pytest.mark.parametrize("bpp", [2.0, 19.5])
def test_inverse_quantiser_with_masks_slice(eng, oracle, bpp):
    img = np.ascontiguousarray(turbulence((8, 24, 40))[3])
    s = oracle.comp_2d(img, 1, bpp, False)
    assert s[17] == 32   # (32 planes: the 32-bit coefficients)
    for of in (True, False):
        got, rep = launched(eng, lambda: eng.decompress_2d(dev_of(s), (24, 40), output_float=of).cpu().numpy())
        print(bpp, of, rep)
        assert has(rep, "k_inv_quantize<uint32_t>") and not has(rep, "k_dec_finish"), rep
        assert same(got, oracle.decomp_2d(s, (24, 40), of)), (bpp, of)


def test_inverse_quantiser_64_bit(eng, oracle):
    r = ramp_field((16, 16, 16))
    c = oracle.comp_3d(r, (16, 16, 16), 1, 30.0)
    assert planes(c) == 53
    for of in (True, False):
        got, rep = launched(eng, lambda: eng.decompress(dev_of(c), of).cpu().numpy())
        print(of, rep)
        assert has(rep, "k_inv_quantize<uint64_t>") and not has(rep, "k_inv_quantize<uint32_t>"), rep
        assert same(got, oracle.decomp_3d(c, of)), of


@pytest.mark.parametrize("shape,kernel", [(CUBE, "k_lift_xyz_inv<2, false>"), (SLAB, "k_inv_quantize<uint32_t>")])
def test_encoder_reconstructs_without_masks(eng, oracle, shape, kernel):
    """The point-wise error stage reconstructs what the decoder will see from the encoder's own coefficients: no masks,
    no decoder state.  A chunk the fused kernels take goes through k_lift_xyz_inv (writing doubles, plain magnitudes and
    signs), any other through k_inv_quantize and the per-axis passes."""
    v = turbulence(shape)
    got, rep = launched(eng, lambda: bytes(eng.compress(cuda(v), xyz(shape), 1e-3, mode=3).cpu().numpy()))
    print(shape, rep)
    assert has(rep, kernel), rep
    assert has(rep, "k_inv_quantize") == (shape == SLAB), rep
    assert got == container(oracle, shape, 3, 1e-3)


@pytest.mark.parametrize("shape,scale", [((13, 21, 30), 3000.0), ((32, 32, 32), 4294967295.0), ((16, 20, 24), float(2 ** 53 - 1))])
def test_stage_call_finishes_the_coefficients(eng, oracle, shape, scale):
    v = oracle.dwt3d(turbulence(shape).astype(np.float64))
    coef, sign, _ = oracle.quantize(v, np.abs(v).max() / scale)
    stream = oracle.speck3d_encode(coef, sign, 0)
    wide = scale > 4294967295.0
    assert (stream[0] > 32) == wide
    for cut in (9 + (len(stream) - 9) // 2, 9 + (len(stream) - 9) // 7):   # (the stream ends inside a plane)
        want_c, want_s = oracle.speck3d_decode(stream[:cut], shape)
        (got_c, got_s), rep = launched(eng, lambda: eng.speck3d_decode(stream[:cut], shape))
        print(shape, cut, rep)
        assert has(rep, "k_dec_finish<uint64_t>" if wide else "k_dec_finish<uint32_t>"), rep
        assert np.array_equal(got_c, want_c) and np.array_equal(got_s, want_s), (shape, cut)
