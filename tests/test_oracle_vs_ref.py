"""CPU: the oracle restatement against the REAL reference, stage by stage and end to end, bit for bit:
the reference itself where oracle/_ref is built (oracle/Makefile), else the digests of its results
recorded from it (tests/refbits.py, tests/golden/ref_digests.json)."""
import numpy as np
import pytest

from fields import (COEF_BUDGETS, COEF_PATTERNS, COEF_SHAPES, VALUE_DOMAIN_CASES, VD_SHAPE, cached_value_domain_fields,
                    coefficient_pattern, ramp_field, smooth_field, value_domain_plane, value_domain_refused,
                    value_domain_settings)
from refbits import same
from sperr_amd.farm import split_container
from sperr_amd.synth import turbulence

SHAPES = [(17, 17, 17), (32, 32, 32), (23, 45, 70), (41, 64, 64), (9, 40, 48), (64, 64, 64)]


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("shape", SHAPES)
def test_dwt_idwt_conditioner_bit_exact(oracle, ref, shape):
    v = turbulence(shape).astype(np.float64)
    a = oracle.dwt3d(v)
    assert same(bits(a), ref.get(lambda r: r.dwt3d(v)))
    assert same(bits(oracle.idwt3d(a)), ref.get(lambda r: r.idwt3d(a)))
    ca, ha, _ = oracle.condition(v)
    cb, hb, _ = ref.get(lambda r: r.condition(v))
    assert same(ha, hb) and same(bits(ca), cb)


@pytest.mark.parametrize("shape", SHAPES[:5])
@pytest.mark.parametrize("budget", [0, 4096, 100000])
def test_speck_streams_bit_exact(oracle, ref, shape, budget):
    v = oracle.dwt3d(turbulence(shape).astype(np.float64))
    q = np.abs(v).max() / 60000.0
    coef, sign, width = oracle.quantize(v, q)
    so = oracle.speck3d_encode(coef, sign, budget)
    assert same(so, ref.get(lambda r: r.speck3d_encode(coef, sign, budget, width=8)))
    co, sgo = oracle.speck3d_decode(so, shape)
    idx = np.nonzero(co.reshape(-1) != 0)[0]

    def sign_bits(words):   # the signs of the nonzero coefficients only
        return (words[idx >> 6] >> (idx & 63).astype(np.uint64)) & np.uint64(1)

    def ref_decode(r):   # the reference's coefficients and the signs of the nonzero ones
        c, s = r.speck3d_decode(so, shape)
        return c, sign_bits(s)

    cr, br = ref.get(ref_decode)
    assert same(co, cr)
    assert same(sign_bits(sgo), br)
    # truncated stream (progressive access): same prefix decodes identically
    cut = 9 + (len(so) - 9) // 3
    co, _ = oracle.speck3d_decode(so[:cut], shape)
    assert same(co, ref.get(lambda r: r.speck3d_decode(so[:cut], shape)[0]))


@pytest.mark.parametrize("chunks", [(64, 64, 64), (32, 32, 32), (40, 30, 20)])
@pytest.mark.parametrize("bpp", [0.5, 2.0, 6.5])
def test_container_bit_exact(oracle, ref, chunks, bpp):
    v = turbulence((50, 64, 72))
    so = oracle.comp_3d(v, chunks, 1, bpp)
    assert same(so, ref.get(lambda r: r.comp_3d(v, chunks, 1, bpp)))
    assert same(bits(oracle.decomp_3d(so, True)), ref.get(lambda r: r.decomp_3d(so, True)))
    assert same(bits(oracle.decomp_3d(so, False)), ref.get(lambda r: r.decomp_3d(so, False)))


def test_high_precision_retry_bit_exact(oracle, ref):
    """src/SPECK_FLT.cpp:530-538: too few bits at 32 planes -> re-quantise for 53 planes."""
    r = ramp_field((16, 16, 16))
    for bpp in (30.0, 60.0):
        so = oracle.comp_3d(r, (16, 16, 16), 1, bpp)
        assert so[18 + 17] == 53 and same(so, ref.get(lambda R: R.comp_3d(r, (16, 16, 16), 1, bpp)))
        assert same(bits(oracle.decomp_3d(so)), ref.get(lambda R: R.decomp_3d(so)))


def test_chunk_volume_matches(oracle, ref):
    for vol, ch in [((128, 128, 41), (64, 64, 41)), ((91, 91, 91), (64, 64, 64)),
                    ((100, 70, 33), (30, 40, 8)), ((5, 5, 5), (9, 9, 9))]:
        ch = tuple(min(c, v) for c, v in zip(ch, vol))
        assert same(oracle.chunk_volume(vol, ch), ref.get(lambda r: r.chunk_volume(vol, ch)))


def test_double_input_and_f64_field(oracle, ref):
    v = smooth_field((24, 40, 40), dtype=np.float64)
    so = oracle.comp_3d(v, (40, 40, 24), 1, 3.0)
    assert same(so, ref.get(lambda r: r.comp_3d(v, (40, 40, 24), 1, 3.0))) and not (so[1] & 0x20)


@pytest.mark.parametrize("chunks", [(32, 32, 32), (48, 40, 24)])
@pytest.mark.parametrize("psnr", [40.0, 85.0, 140.0, 230.0])
def test_psnr_mode_bit_exact(oracle, ref, chunks, psnr):
    """Mode 2 (src/SPECK_FLT.cpp:237-279,431-452): q search, integer width, full-depth coding."""
    v = turbulence((48, 40, 64))
    got = oracle.comp_3d(v, chunks, 2, psnr)
    assert same(got, ref.get(lambda r: r.comp_3d(v, chunks, 2, psnr)))
    assert same(bits(oracle.decomp_3d(got, False)), ref.get(lambda r: r.decomp_3d(got, False)))
    d = smooth_field((24, 40, 40), dtype=np.float64)
    assert same(oracle.comp_3d(d, chunks, 2, psnr), ref.get(lambda r: r.comp_3d(d, chunks, 2, psnr)))


@pytest.mark.parametrize("chunks", [(32, 32, 32), (48, 40, 24), (64, 40, 48)])
@pytest.mark.parametrize("tol", [0.3, 1e-2, 1e-4, 1e-9])
def test_pwe_mode_bit_exact(oracle, ref, chunks, tol):
    """Mode 3 (src/SPECK_FLT.cpp:280-281,461-486,573-584): q = 1.5 tol, full-depth coding, and the
    outlier list through Outlier_Coder / SPECK1D_INT; decoded values honour the tolerance."""
    v = turbulence((48, 40, 64))
    got = oracle.comp_3d(v, chunks, 3, tol)
    assert same(got, ref.get(lambda r: r.comp_3d(v, chunks, 3, tol)))
    dec = oracle.decomp_3d(got, False)
    assert same(bits(dec), ref.get(lambda r: r.decomp_3d(got, False)))
    assert np.abs(dec - v.astype(np.float64)).max() <= tol
    d = smooth_field((24, 40, 40), dtype=np.float64) * 1e-3
    got = oracle.comp_3d(d, chunks, 3, tol)
    assert same(got, ref.get(lambda r: r.comp_3d(d, chunks, 3, tol)))
    assert same(bits(oracle.decomp_3d(got, False)), ref.get(lambda r: r.decomp_3d(got, False)))


@pytest.mark.parametrize("shape,chunks", [((64, 64, 64), (32, 32, 32)), ((48, 64, 32), (32, 32, 24)),
                                          ((40, 40, 40), (40, 40, 40)), ((41, 64, 64), (64, 64, 41))])
def test_multi_resolution_decode_bit_exact(oracle, ref, shape, chunks):
    """SPERR3D_OMP_D::decompress(p, true): volume and hierarchy (src/SPERR3D_OMP_D.cpp:50-150,
    src/CDF97.cpp:150-168, src/SPECK_FLT.cpp:592-603) against the reference's own classes."""
    v = turbulence(shape)
    stream = oracle.comp_3d(v, chunks, 1, 3.0)
    assert same(stream, ref.get(lambda r: r.comp_3d(v, chunks, 1, 3.0)))
    vol_o, lv_o = oracle.decomp_3d_multi_res(stream)
    vol_r, lv_r = ref.get(lambda r: r.decomp_3d_multi_res(stream))
    assert same(bits(vol_o), vol_r)
    assert len(lv_o) == len(lv_r)
    for a, b in zip(lv_o, lv_r):   # (shape and bits)
        assert same(bits(a), b)


@pytest.mark.parametrize("shape", [(64, 64), (37, 50), (96, 121), (9, 200), (150, 11)])
@pytest.mark.parametrize("mode,quality", [(1, 0.7), (1, 5.0), (2, 75.0), (2, 160.0), (3, 1e-2), (3, 1e-6)])
def test_2d_slices_bit_exact(oracle, ref, shape, mode, quality):
    """sperr_comp_2d / sperr_decomp_2d (src/SPERR_C_API.cpp:7-134): dwt2d, SPECK2D_INT with its
    type-I set (src/SPECK2D_INT*.cpp), all three modes, with and without the 10-byte header."""
    for dtype in (np.float32, np.float64):
        img = turbulence((1,) + shape, dtype=dtype)[0]
        for hdr in (False, True):
            got = oracle.comp_2d(img, mode, quality, hdr)
            assert same(got, ref.get(lambda r: r.comp_2d(img, mode, quality, hdr)))
        body = got[10:]
        for as_float in (True, False):
            assert same(bits(oracle.decomp_2d(body, shape, as_float)),
                        ref.get(lambda r: r.decomp_2d(body, shape, as_float)))


@pytest.mark.parametrize("shape", [(64, 64), (37, 50), (96, 121), (9, 200), (150, 11), (7, 7), (100, 128)])
@pytest.mark.parametrize("mode,quality", [(1, 3.0), (2, 90.0), (3, 1e-3)])
def test_2d_multi_resolution_bit_exact(oracle, ref, shape, mode, quality):
    """SPECK2D_FLT::decompress(multi_res = true) (src/SPECK2D_FLT.cpp:52-58, src/CDF97.cpp:114-130,
    src/SPECK_FLT.cpp:592-603): the slice and the slice at every coarsened resolution, full and
    truncated streams."""
    img = turbulence((1,) + shape, dtype=np.float64 if mode == 3 else np.float32)[0]
    stream = oracle.comp_2d(img, mode, quality, False)
    assert same(stream, ref.get(lambda r: r.comp_2d(img, mode, quality, False)))
    for cut in (len(stream), max(27, len(stream) * 2 // 5)):
        a, la = oracle.decomp_2d_multi_res(stream[:cut], shape)
        b, lb = ref.get(lambda r: r.decomp_2d_multi_res(stream[:cut], shape))
        assert same(bits(a), b)
        assert same(bits(a), ref.get(lambda r: r.decomp_2d(stream[:cut], shape, False)))
        assert len(la) == len(lb)
        for x, y in zip(la, lb):   # (shape and bits)
            assert same(bits(x), y)


def test_speck1d_bit_exact(oracle, ref):
    """SPECK1D_INT_ENC / _DEC (src/SPECK1D_INT*.cpp) on sparse arrays: same stream, and it
    round-trips exactly through both decoders."""
    rng = np.random.default_rng(5)
    for n, k, top in [(3, 2, 3), (5, 5, 9), (100, 7, 200), (4097, 300, 5), (65536, 1000, 70000)]:
        coef = np.zeros(n, dtype=np.uint64)
        pos = rng.choice(n, size=min(k, n), replace=False)
        coef[pos] = rng.integers(1, top + 1, size=pos.size, dtype=np.uint64)
        sign = rng.integers(0, 2, size=n).astype(bool)
        stream = oracle.speck1d_encode(coef, sign)
        assert same(stream, ref.get(lambda r: r.speck1d_encode(coef, sign)))
        c2, s2 = oracle.speck1d_decode(stream, n)
        assert np.array_equal(c2, coef)
        assert np.array_equal(s2[coef > 0], sign[coef > 0])

        def ref_decode(r):   # the reference's coefficients and the signs of the nonzero ones
            c, s = r.speck1d_decode(stream, n)
            return c, s[coef > 0]

        c2, s2 = ref.get(ref_decode)
        assert same(coef, c2)
        assert same(sign[coef > 0], s2)


@pytest.mark.parametrize("chunks", [(64, 40, 48), (32, 32, 32), (20, 18, 16)])
@pytest.mark.parametrize("pct", [0, 1, 10, 37, 75, 100, 150])
def test_progressive_truncation_bit_exact(oracle, ref, chunks, pct):
    """sperr_trunc_3d (src/SPERR3D_Stream_Tools.cpp:134-226): same bytes, and the truncated
    container decodes to the same values."""
    v = turbulence((48, 40, 64))
    v[:16, :18, :20] = 2.5   # a constant chunk for the (20, 18, 16) chunking: 17-byte stream
    full = oracle.comp_3d(v, chunks, 1, 3.0)
    assert same(full, ref.get(lambda r: r.comp_3d(v, chunks, 1, 3.0)))
    got = oracle.trunc_3d(full, pct)
    assert same(got, ref.get(lambda r: r.trunc_3d(full, pct)))
    assert same(bits(oracle.decomp_3d(got, True)), ref.get(lambda r: r.decomp_3d(got, True)))


def test_integer_len_rule_matches_the_reference(oracle, ref):
    """SPECK_FLT::integer_len() (src/SPECK_FLT.cpp:193-213) of the reference's encoder and decoder
    against the rule include/sperr_hip.hpp derives from the oracle's stream: byte 17 of a chunk
    stream, the number of bit planes, <= 8 / 16 / 32 / more -> 1 / 2 / 4 / 8 bytes."""
    import ctypes as C
    corner = turbulence((32, 32, 32)).astype(np.float64)

    def integer_len(r, psnr):   # (return code, encoder's integer length, decoder's)
        w = (C.c_size_t * 2)()
        r.probe.refp_integer_len_psnr.restype = C.c_int
        r.probe.refp_integer_len_psnr.argtypes = [C.c_void_p] + [C.c_size_t] * 3 + [C.c_double, C.c_void_p]
        return r.probe.refp_integer_len_psnr(corner.ctypes.data, 32, 32, 32, psnr, w), w[0], w[1]

    seen = set()
    for psnr in (20.0, 60.0, 120.0, 250.0):
        rc, w0, w1 = ref.get(lambda r: integer_len(r, psnr))
        nbp = oracle.comp_3d(corner, (32, 32, 32), 2, psnr)[18 + 17]
        rule = 1 if nbp <= 8 else 2 if nbp <= 16 else 4 if nbp <= 32 else 8
        assert same(0, rc) and same(rule, w0) and same(rule, w1)
        seen.add(rule)
    assert seen == {1, 2, 4, 8}


# ---- value domains (tests/fields.py: value_domain_fields, coefficient_pattern) -----------------------------------


def chunk_planes(container):
    """byte 17 of every chunk stream that has one (a constant chunk's stream is its 17-byte conditioner header)"""
    return [p[17] for p in split_container(container)[3] if len(p) > 17]


@pytest.mark.parametrize("name,dtype", VALUE_DOMAIN_CASES)
def test_value_domain_containers_bit_exact(oracle, ref, name, dtype):
    """One-signed, offset, scaled, subnormal, sparse, discontinuous and mixed-range volumes, as one chunk and in 16^3
    chunks, three rates, two PSNR targets and two tolerances: the container, both decodes, and in mode 3 the
    tolerance on the reference's fp64 decode.  No PSNR target or tolerance reaches the regime of more than 53 bit
    planes, where the oracle is not pinned to the reference."""
    v = cached_value_domain_fields(VD_SHAPE, dtype)[name]
    v64 = v.astype(np.float64)
    for chunks in (v.shape[::-1], (16, 16, 16)):
        for mode, q in value_domain_settings(name, v):
            so = oracle.comp_3d(v, chunks, mode, q)
            assert same(so, ref.get(lambda r: r.comp_3d(v, chunks, mode, q))), (chunks, mode, q)
            if mode != 1:   # (a rate that 32 planes cannot fill makes the reference itself re-quantise for 53 or 54)
                assert max(chunk_planes(so), default=0) <= 53, (chunks, mode, q)
            dec = oracle.decomp_3d(so, False)
            assert same(bits(dec), ref.get(lambda r: r.decomp_3d(so, False))), (chunks, mode, q)
            assert same(bits(oracle.decomp_3d(so, True)), ref.get(lambda r: r.decomp_3d(so, True))), (chunks, mode, q)
            if mode == 3:   # (dec has the bits of the reference's fp64 decode: asserted just above)
                assert np.abs(dec - v64).max() <= q, (chunks, q)
        for mode, q in value_domain_refused(name, v):   # (the reference does not survive its own refusal here)
            assert refuses(lambda: oracle.comp_3d(v, chunks, mode, q)), (chunks, mode, q)


def refuses(call):
    try:
        call()
    except RuntimeError:
        return True
    return False


@pytest.mark.parametrize("name,dtype", VALUE_DOMAIN_CASES)
def test_value_domain_2d_slices_bit_exact(oracle, ref, name, dtype):
    img, settings, refused = value_domain_plane(name, dtype)
    for mode, q in refused:   # (sperr_comp_2d hands the refusal back as an error code)
        assert refuses(lambda: oracle.comp_2d(img, mode, q, False))
        assert same(True, ref.get(lambda r: refuses(lambda: r.comp_2d(img, mode, q, False))))
    for mode, q in settings:
        for hdr in (False, True):
            got = oracle.comp_2d(img, mode, q, hdr)
            assert same(got, ref.get(lambda r: r.comp_2d(img, mode, q, hdr))), (mode, q, hdr)
        body = got[10:]
        assert mode == 1 or len(body) == 17 or body[17] <= 53
        for as_float in (True, False):
            assert same(bits(oracle.decomp_2d(body, img.shape, as_float)),
                        ref.get(lambda r: r.decomp_2d(body, img.shape, as_float))), (mode, q, as_float)


@pytest.mark.parametrize("pattern", COEF_PATTERNS)
def test_value_domain_speck_patterns_bit_exact(oracle, ref, pattern):
    """The SPECK stage on the extremes of occupancy: every coefficient significant on the first plane (32 and 53 bits
    deep), one coefficient in the whole array (first, last), one bit per coefficient, a geometric fall-off."""
    for shape in COEF_SHAPES:
        coef, sign, _ = coefficient_pattern(pattern, shape)

        def sign_bits(words):   # the signs of the nonzero coefficients only
            return (words[idx >> 6] >> (idx & 63).astype(np.uint64)) & np.uint64(1)

        for budget in COEF_BUDGETS:
            so = oracle.speck3d_encode(coef, sign, budget)
            assert same(so, ref.get(lambda r: r.speck3d_encode(coef, sign, budget, width=8))), (shape, budget)
            for cut in (len(so), 9 + (len(so) - 9) // 2, 9 + (len(so) - 9) // 7):
                co, sgo = oracle.speck3d_decode(so[:cut], shape)
                idx = np.nonzero(co.reshape(-1) != 0)[0]

                def ref_decode(r):
                    c, s = r.speck3d_decode(so[:cut], shape)
                    return c, sign_bits(s)

                cr, br = ref.get(ref_decode)
                assert same(co, cr), (shape, budget, cut)
                assert same(sign_bits(sgo), br), (shape, budget, cut)
                if budget == 0 and cut == len(so):   # the whole stream gives the coefficients back
                    assert np.array_equal(co, coef) and np.array_equal(sign_bits(sgo), sign_bits(sign)), shape


# ---- coefficient patterns aligned to the set tree (tests/coef_cases.py) ---------------------------------------------


def _coef_cases():
    import coef_cases as cc
    return pytest.mark.parametrize("name,shape", cc.ALL_CASES, ids=cc.CASE_IDS)


@_coef_cases()
def test_tree_aligned_patterns_bit_exact(oracle, ref, name, shape):
    """The SPECK stage at 128^3 (and at 100 x 128 x 128, whose lists mix set shapes) on patterns that keep the lists
    of the 2^3, 4^3 and 8^3 sets thousands of entries long and choose what their tokens are: the oracle's stream, and
    its decode of the whole stream and of the stream cut to 1/2 and to 1/7 of its payload, against the reference's."""
    import coef_cases as cc
    coef, sign, _ = cc.case(name, shape)
    so = oracle.speck3d_encode(coef, sign, 0)
    assert same(so, ref.get(lambda r: r.speck3d_encode(coef, sign, 0, width=8)))
    for cut in cc.stream_cuts(so):
        co, sgo = oracle.speck3d_decode(so[:cut], shape)
        idx = np.nonzero(co.reshape(-1) != 0)[0]

        def ref_decode(r):   # the reference's coefficients and the signs of the nonzero ones
            c, s = r.speck3d_decode(so[:cut], shape)
            return c, cc.sign_bits(s, idx)

        cr, br = ref.get(ref_decode)
        assert same(co, cr), cut
        assert same(cc.sign_bits(sgo, idx), br), cut
        if cut == len(so):   # the whole stream gives the coefficients back
            assert np.array_equal(co, coef) and np.array_equal(cc.sign_bits(sgo, idx), cc.sign_bits(sign, idx))


def _slice_cases():
    import slice_cases as sc
    return pytest.mark.parametrize("name,shape", sc.ALL_CASES, ids=sc.CASE_IDS)


@_slice_cases()
def test_slice_patterns_bit_exact(oracle, ref, name, shape):
    """The 2D coder on the case table of tests/slice_cases.py (patterns aligned to the quadtree forest, and patterns
    that choose what the type-I set does on every plane): the oracle's stream, and its decode of the whole stream and
    of the stream cut to 1/2 and to 1/7 of its payload, against the reference's SPECK2D_INT_ENC / _DEC."""
    import slice_cases as sc
    coef, sign, _ = sc.case(name, shape)
    so = oracle.speck2d_encode(coef, sign, 0)
    assert same(so, ref.get(lambda r: r.speck2d_encode(coef, sign, 0, width=8)))
    for cut in sc.stream_cuts(so):
        co, sgo = oracle.speck2d_decode(so[:cut], shape)
        idx = np.nonzero(co.reshape(-1) != 0)[0]

        def ref_decode(r):   # the reference's coefficients and the signs of the nonzero ones
            c, s = r.speck2d_decode(so[:cut], shape)
            return c, sc.sign_bits(s, idx)

        cr, br = ref.get(ref_decode)
        assert same(co, cr), cut
        assert same(sc.sign_bits(sgo, idx), br), cut
        if cut == len(so):   # the whole stream gives the coefficients back
            assert np.array_equal(co, coef) and np.array_equal(sc.sign_bits(sgo, idx), sc.sign_bits(sign, idx))


# ---- the outlier coder as a primitive (tests/outlier_cases.py) -----------------------------------------------------


def refusal_code(call):
    """the return code an outlier coder refuses with, 0 if it does not"""
    from oracle.pyoracle import OutlierRefused
    try:
        call()
    except OutlierRefused as e:
        return e.code
    return 0


def test_outlier_coder_bit_exact(oracle, ref):
    """Outlier_Coder (src/Outlier_Coder.cpp) itself against the oracle's orc_outlier_encode / _decode_apply: the table's
    coder cases up to 64 bit planes, and the encoder cases in which the reference's integer width, picked from the
    largest raw error, wraps the magnitudes of error / tolerance -- some or all of them to zero --, the ties of llrint,
    the tolerance's boundary and the refusal from a raw error of 2^63 on.  Same stream byte for byte, same bits from
    both decoders."""
    import outlier_cases as oc
    widths, wrapped = set(), set()
    for name, n in oc.coder_cases():
        coef, sign = oc.coder_case(name, n)
        stream = oracle.speck1d_encode(coef, sign)
        assert same(stream, ref.get(lambda r: r.speck1d_encode(coef, sign))), (name, n)
        if name != "top_bit":   # (an error of 2^63 tolerances needs a raw error the coder refuses or cannot hold)
            pos, err = oc.outlier_list(oc.errors_of(coef, sign, 1.0), 1.0)
            assert oracle.outlier_encode(pos, err, n, 1.0) == stream, (name, n)
            assert same(stream, ref.get(lambda r: r.outlier_encode(pos, err, n, 1.0))), (name, n)
        tol, base = oc.GOLDEN_TOL, oc.golden_base(n)
        got = oracle.outlier_decode_apply(stream, n, tol, base)
        assert same(bits(got), ref.get(lambda r: r.outlier_decode_apply(stream, n, tol, base))), (name, n)
        assert np.array_equal(got, base + oc.corrector(coef, sign, tol)), (name, n)
    for name, n, tol, err in oc.encoder_cases():
        pos, e = oc.outlier_list(err, tol)
        stream = oracle.outlier_encode(pos, e, n, tol)
        assert same(stream, ref.get(lambda r: r.outlier_encode(pos, e, n, tol))), name
        base = np.zeros(n)
        got = oracle.outlier_decode_apply(stream, n, tol, base)
        assert same(bits(got), ref.get(lambda r: r.outlier_decode_apply(stream, n, tol, base))), name
        raw = int(np.rint(np.abs(e).max()))
        width = 8 if raw <= 0xff else 16 if raw <= 0xffff else 32 if raw <= 0xffffffff else 64
        widths.add(width)
        if np.abs(e / tol).max() >= 2.0 ** width:
            wrapped.add(width)
            assert stream[0] <= width, name
    assert widths == {8, 16, 32, 64} and wrapped == {8, 16, 32}
    zero = dict((c[0], c) for c in oc.encoder_cases())["all_wrap_to_zero"]
    assert oracle.outlier_encode(*oc.outlier_list(zero[3], zero[2]), zero[1], zero[2]) == bytes(9)
    ex = dict((c[0], c) for c in oc.encoder_cases())["wrap_example"]
    assert oracle.outlier_encode(*oc.outlier_list(ex[3], ex[2]), ex[1], ex[2]).hex() == \
        "086800000000000000af2c0080000cc0000480000000"
    # refusals: a raw error of 2^63 (FE_INVALID, code 7); an error within the tolerance in the list; an empty list
    name, n, tol, p, e = oc.REFUSED_ENCODER_CASE
    assert refusal_code(lambda: oracle.outlier_encode([p], [e], n, tol)) == 7
    assert same(7, ref.get(lambda r: refusal_code(lambda: r.outlier_encode([p], [e], n, tol))))
    assert refusal_code(lambda: oracle.outlier_encode([p], [-e], n, tol)) == 7
    assert same(7, ref.get(lambda r: refusal_code(lambda: r.outlier_encode([p], [-e], n, tol))))
    below = np.nextafter(e, 0.0)
    assert same(oracle.outlier_encode([p], [below], n, tol), ref.get(lambda r: r.outlier_encode([p], [below], n, tol)))
    for plist, elist in (([3], [0.125]), ([3, 4], [1.0, 0.125]), ([], [])):
        assert refusal_code(lambda: oracle.outlier_encode(plist, elist, 65, 0.125)) != 0
        assert same(True, ref.get(lambda r: refusal_code(lambda: r.outlier_encode(plist, elist, 65, 0.125)) != 0))
