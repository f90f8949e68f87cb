"""GPU parity on the value ranges real data has (-m gpu): one-signed volumes with a mean far from zero, huge and tiny
units, fp32 subnormals, spikes, steps, masks, mostly-zero fields and chunks of very different dynamic range in one
call (tests/fields.py: value_domain_fields), and the extremes of occupancy of the coefficient array at the SPECK stage
(coefficient_pattern).  The yardstick is the oracle, which tests/test_oracle_vs_ref.py pins to the real reference on
the same fields and settings; every compare is on bytes or bit patterns.  The last tests ask for the reference's
refusals: a chunk whose largest quantised magnitude reaches 2^63 (src/SPECK_FLT.cpp:323-327) and an outlier whose
error does (src/Outlier_Coder.cpp:82-91)."""
import numpy as np
import pytest

from fields import (COEF_BUDGETS, COEF_PATTERNS, COEF_SHAPES, VALUE_DOMAIN_CASES, VD_SHAPE, cached_value_domain_fields,
                    coefficient_pattern, smooth_field, value_domain_plane, value_domain_refused,
                    value_domain_settings)
from sperr_amd.farm import split_container

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    return SperrHip()


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: the cached fields are read-only)


def dev_of(container):
    return cuda(np.frombuffer(container, dtype=np.uint8))


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def span_of(v):
    return float(v.astype(np.float64).max() - v.astype(np.float64).min()) or 1.0


def chunk_planes(container):
    """byte 17 of every chunk stream that has one (a constant chunk's stream is its 17-byte conditioner header)"""
    return [p[17] for p in split_container(container)[3] if len(p) > 17]


def check_container(eng, oracle, v, chunks, mode, q):
    """eng.compress against the oracle's bytes, both decodes against its bits, the tolerance in mode 3"""
    tag = (v.shape, str(v.dtype), chunks, mode, q)
    want = oracle.comp_3d(v, chunks, mode, q)
    if mode != 1:   # (beyond 53 planes the oracle is not pinned to the reference)
        assert max(chunk_planes(want), default=0) <= 53, tag
    got = bytes(eng.compress(cuda(v), chunks, q, mode=mode).cpu().numpy())
    assert len(got) == len(want), tag
    assert got == want, tag
    dev = dev_of(want)
    assert same(eng.decompress(dev, True).cpu().numpy(), oracle.decomp_3d(want, True)), tag
    d = eng.decompress(dev, False).cpu().numpy()
    assert same(d, oracle.decomp_3d(want, False)), tag
    if mode == 3:
        assert np.abs(d - v.astype(np.float64)).max() <= q, tag
    return want


def refuses(call, error):
    try:
        call()
    except error:
        return True
    return False


@pytest.mark.parametrize("name,dtype", VALUE_DOMAIN_CASES)
def test_value_domain_containers(eng, oracle, name, dtype):
    """The grid of tests/test_oracle_vs_ref.py::test_value_domain_containers_bit_exact on the device: each field as
    one chunk and in 16^3 chunks (the patchworks: 12 chunks in 8 shape groups), 0.5 / 4 / 24 bpp, 40 / 120 dB and a
    tolerance of 1e-2 / 1e-5 of the span.  One-signed data takes order_key's negative branch and the range of a large
    common offset in PSNR mode; a mean far from zero exercises the `+ mean` of every inverse tail."""
    from sperr_amd.api import SperrHipError
    v = cached_value_domain_fields(VD_SHAPE, dtype)[name]
    for chunks in (v.shape[::-1], (16, 16, 16)):
        for mode, q in value_domain_settings(name, v):
            check_container(eng, oracle, v, chunks, mode, q)
        for mode, q in value_domain_refused(name, v):   # an outlier's error of 2^63 and more: the reference refuses
            assert refuses(lambda: oracle.comp_3d(v, chunks, mode, q), RuntimeError), (chunks, mode, q)
            assert refuses(lambda: eng.compress(cuda(v), chunks, q, mode=mode), SperrHipError), (chunks, mode, q)


LARGE = [(n, d) for n, d in VALUE_DOMAIN_CASES if n in ("offset_pos", "spike", "step", "checker", "white", "subnormal_f32")]


@pytest.mark.parametrize("name,dtype", LARGE)
def test_value_domain_large_chunk(eng, oracle, name, dtype):
    """One 64^3 chunk, one setting per mode: the fused x-y-z brick, the decoder's compact chunk buffer and the dyadic
    list kernels on sparse, discontinuous, one-signed and subnormal data."""
    v = cached_value_domain_fields((64, 64, 64), dtype)[name]
    for mode, q in ((1, 4.0), (2, 90.0), (3, span_of(v) * 1e-4)):
        check_container(eng, oracle, v, (64, 64, 64), mode, q)


@pytest.mark.parametrize("name", ["patchwork", "patchwork_mild"])
def test_patchwork_batch_and_host_api(eng, oracle, name):
    """Chunks whose dynamic ranges differ by 2^200, an all-zero and a constant one among them, coded in one call:
    through compress_batch beside a plain smooth volume (two volumes' chunks share the shape groups) and through the
    host sperr_comp_3d (the chunk farm); compress() itself runs in test_value_domain_containers."""
    import torch
    v = cached_value_domain_fields(VD_SHAPE, "float32")[name]
    plain = smooth_field(v.shape, seed=5)
    modes = {m for m, _ in value_domain_settings(name, v)}
    for mode, q in ((1, 4.0), (2, 90.0), (3, span_of(v) * 1e-5)):
        if mode not in modes:
            continue
        want = [oracle.comp_3d(a, (16, 16, 16), mode, q) for a in (v, plain)]
        if mode != 1:
            assert max(chunk_planes(want[0]) + chunk_planes(want[1])) <= 53
        for order in ((0, 1), (1, 0)):
            vols = torch.stack([cuda((v, plain)[k]) for k in order]).contiguous()
            parts = eng.compress_batch(vols, (16, 16, 16), q, mode=mode)
            for p, k in zip(parts, order):
                assert bytes(p.cpu().numpy()) == want[k], (mode, q, order, k)
            back = eng.decompress_batch(parts, output_float=False).cpu().numpy()
            for b, k in zip(back, order):
                assert same(b, oracle.decomp_3d(want[k], False)), (mode, q, order, k)
        assert eng.comp_3d(v, (16, 16, 16), mode, q) == want[0], (mode, q)
        assert same(eng.decomp_3d(want[0], True), oracle.decomp_3d(want[0], True)), (mode, q)


@pytest.mark.parametrize("shape", [(17, 17, 17), (20, 33, 40), (64, 64, 64)])
def test_value_domain_dwt_idwt_bit_exact(eng, oracle, shape):
    """The transform alone, forward and inverse, on every fp64 field: tells a transform fault from a coder fault."""
    for name, v in cached_value_domain_fields(shape, "float64").items():
        want = oracle.dwt3d(v)
        d = cuda(v)
        eng.dwt3d(d)
        assert same(d.cpu().numpy(), want), name
        eng.dwt3d(d, inverse=True)
        assert same(d.cpu().numpy(), oracle.idwt3d(want)), name


@pytest.mark.parametrize("shape", COEF_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pattern", COEF_PATTERNS)
def test_speck_coefficient_patterns(eng, oracle, pattern, shape):
    """eng.speck3d_encode / _decode on the extremes of occupancy: every coefficient significant on the first plane
    (the lists at their largest on plane one; 32 and 53 bits deep), one nonzero coefficient at either end of the
    array (every other word and plane empty), one bit per coefficient, a geometric fall-off; three budgets, the whole
    stream and the stream cut to 1/2 and 1/7 of its payload."""
    coef, sign, wide = coefficient_pattern(pattern, shape)
    dcoef = cuda(coef.view(np.int64) if wide else coef.astype(np.uint32).view(np.int32))
    dsign = cuda(sign.view(np.int64))
    for budget in COEF_BUDGETS:
        want = oracle.speck3d_encode(coef, sign, budget)
        got = eng.speck3d_encode(dcoef, dsign, budget)
        assert got[:9] == want[:9], budget
        assert got == want, budget
        for cut in (len(want), 9 + (len(want) - 9) // 2, 9 + (len(want) - 9) // 7):
            c0, s0 = oracle.speck3d_decode(want[:cut], shape)
            c1, s1 = eng.speck3d_decode(want[:cut], shape)
            assert np.array_equal(c0, c1), (budget, cut)
            assert np.array_equal(s0, s1), (budget, cut)


@pytest.mark.parametrize("name,dtype", VALUE_DOMAIN_CASES)
def test_value_domain_2d_slices(eng, oracle, name, dtype):
    """One plane of each field through compress_2d / decompress_2d: three modes, with and without the header, float
    and double output (the settings of tests/test_oracle_vs_ref.py::test_value_domain_2d_slices_bit_exact)."""
    from sperr_amd.api import SperrHipError
    img, settings, refused = value_domain_plane(name, dtype)
    for mode, q in refused:
        assert refuses(lambda: oracle.comp_2d(img, mode, q, False), RuntimeError), (mode, q)
        assert refuses(lambda: eng.compress_2d(cuda(img), q, mode=mode), SperrHipError), (mode, q)
    for mode, q in settings:
        for hdr in (False, True):
            want = oracle.comp_2d(img, mode, q, hdr)
            got = bytes(eng.compress_2d(cuda(img), q, mode=mode, header=hdr).cpu().numpy())
            assert got == want, (mode, q, hdr)
        body = dev_of(want[10:])
        for as_float in (True, False):
            assert same(eng.decompress_2d(body, img.shape, as_float).cpu().numpy(),
                        oracle.decomp_2d(want[10:], img.shape, as_float)), (mode, q, as_float)


@pytest.mark.parametrize("name", ["spike", "step", "binary"])
def test_derived_decodes_of_sparse_containers(eng, oracle, name):
    """A portion, a box and every level of a container whose coefficient words and planes are mostly empty (the
    decoder's plane masks and in-place refinement planes): (32, 32, 64) in 32^3 chunks at 4 bpp."""
    v = cached_value_domain_fields((32, 32, 64), "float32")[name]
    c = oracle.comp_3d(v, (32, 32, 32), 1, 4.0)
    dev = dev_of(c)
    for of in (True, False):
        whole = oracle.decomp_3d(c, of)
        assert same(eng.decompress(dev, of).cpu().numpy(), whole), of
        assert same(eng.decompress(dev, of, pct=30).cpu().numpy(), oracle.decomp_3d(oracle.trunc_3d(c, 30), of)), of
        for lo, dims in (((27, 3, 5), (14, 20, 9)), ((0, 0, 0), (64, 32, 32)), ((33, 17, 17), (1, 1, 1))):
            got = eng.decompress_box(dev, lo, dims, output_float=of).cpu().numpy()
            want = whole[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]]
            assert same(got, np.ascontiguousarray(want)), (of, lo, dims)
    levels = oracle.decomp_3d_multi_res(c)[1]
    assert len(levels) > 0 and eng.multires_levels(v.shape, (32, 32, 32)) == [lv.shape for lv in levels]
    for h, lv in enumerate(levels):
        for of in (False, True):
            got = eng.decompress_level(dev, h, output_float=of).cpu().numpy()
            assert same(got, lv.astype(np.float32) if of else lv), (h, of)


# ---- the refusal rule ------------------------------------------------------------------------------------------
# The reference refuses a chunk exactly when llrint(maxabs / q) raises FE_INVALID: from 2^63 on.  It does not survive
# its own refusal through the C API, so the yardstick here is the oracle alone.

def still_works(eng, oracle):
    v = smooth_field((24, 40, 40))
    want = oracle.comp_3d(v, (16, 16, 16), 3, 1e-2)
    assert bytes(eng.compress(cuda(v), (16, 16, 16), 1e-2, mode=3).cpu().numpy()) == want
    assert eng.comp_3d(v, (16, 16, 16), 3, 1e-2) == want
    assert same(eng.decompress(dev_of(want), True).cpu().numpy(), oracle.decomp_3d(want, True))


def test_refusal_of_a_chunk_far_beyond_2p63(eng, oracle):
    """patchwork in mode 3 with a tolerance of 0.1: the chunk scaled by 2^60 has maxabs / q near 1.5e22.  The device
    call and the host call raise, and the engine compresses as before afterwards."""
    from sperr_amd.api import SperrHipError
    v = cached_value_domain_fields(VD_SHAPE, "float32")["patchwork"]
    assert refuses(lambda: oracle.comp_3d(v, (16, 16, 16), 3, 0.1), RuntimeError)
    with pytest.raises(SperrHipError):
        eng.compress(cuda(v), (16, 16, 16), 0.1, mode=3)
    with pytest.raises(SperrHipError):
        eng.comp_3d(v, (16, 16, 16), 3, 0.1)
    still_works(eng, oracle)


def test_refusal_just_above_2p63(eng, oracle):
    """maxabs / q = 9.25e18: above 2^63 = 9.2234e18, so the reference refuses, and below the 9.3e18 the engine used
    to test for (it went on to llrint of an out-of-range value and coded the chunk), above the 9.2e18 of the oracle.
    One chunk of fp64 data; maxabs is the largest coefficient of the conditioned, transformed chunk."""
    from sperr_amd.api import SperrHipError
    v = smooth_field((16, 20, 24), dtype=np.float64)
    maxabs = float(np.abs(oracle.dwt3d(oracle.condition(v)[0])).max())
    tol = maxabs / (1.5 * 9.25e18)
    assert 2.0 ** 63 < maxabs / (1.5 * tol) < 9.3e18
    chunks = v.shape[::-1]
    assert refuses(lambda: oracle.comp_3d(v, chunks, 3, tol), RuntimeError)
    with pytest.raises(SperrHipError):
        eng.compress(cuda(v), chunks, tol, mode=3)
    with pytest.raises(SperrHipError):
        eng.comp_3d(v, chunks, 3, tol)
    still_works(eng, oracle)
