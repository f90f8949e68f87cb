"""CPU: the case table of the 2D coder (tests/slice_cases.py) does what it is built for.  The band geometry is checked
against the oracle's helpers, the reach conditions are read off the model `list_reach` (a property of the input
alone), and what every type-I case does to the set is read from the oracle's stream."""
import ctypes as C

import numpy as np
import pytest

import slice_cases as sc

SHAPES = (sc.SHAPE, sc.RAGGED, sc.FLAT, sc.BIG) + sc.MODEL_SHAPES + ((7, 7), (100, 9), (999, 999))
REGION_BITS = 2048   # k_lis_mx's region


def total_bits(stream):
    return int(np.frombuffer(stream, dtype=np.uint64, count=1, offset=1)[0])


def encoder(oracle):
    return lambda c, s: oracle.speck2d_encode(c, s, 0)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_band_geometry_matches_the_oracle_helpers(oracle, shape):
    """The root band and, level by level from the coarsest, BR, TR and BL, from orc_num_of_xforms and
    orc_approx_detail_len as oracle/sperr_oracle.c's speck2_alloc and speck2_code_I use them; the bands tile the slice."""
    dy, dx = shape
    xf, root, bl = sc.bands(shape)
    assert xf == oracle.lib.orc_num_of_xforms(min(dx, dy)) == sc.num_of_xforms(min(dx, dy))

    def ad(n, lev):
        a, d = C.c_size_t(0), C.c_size_t(0)
        oracle.lib.orc_approx_detail_len(n, lev, C.byref(a), C.byref(d))
        assert (a.value, d.value) == sc.approx_detail(n, lev)
        return a.value, d.value

    assert root == (0, 0, ad(dy, xf)[0], ad(dx, xf)[0])
    want = []
    for lev in range(xf, 0, -1):
        (ax, ddx), (ay, ddy) = ad(dx, lev), ad(dy, lev)
        want += [(lev, "BR", ay, ax, ddy, ddx), (lev, "TR", 0, ax, ay, ddx), (lev, "BL", ay, 0, ddy, ax)]
    assert bl == [b for b in want if b[4] and b[5]]
    cover = np.zeros(shape, dtype=np.int32)
    cover[:root[2], :root[3]] += 1
    for _, _, y0, x0, ly, lx in bl:
        cover[y0:y0 + ly, x0:x0 + lx] += 1
    assert (cover == 1).all()


def test_shapes_are_what_the_table_says():
    assert sc.bands(sc.SHAPE)[:2] == (6, (0, 0, 8, 8))
    assert sc.bands(sc.RAGGED)[:2] == (6, (0, 0, 5, 8))
    assert sc.bands(sc.FLAT)[0] == 1
    assert set(sc.LONG_PLANE) == set(sc.CASES) and set(sc.MX_CASES) <= set(sc.CASES)
    for name, shape in sc.ALL_CASES:
        coef, sign, wide = sc.case(name, shape)
        assert coef.shape == shape and not coef.flags.writeable and not sign.flags.writeable
        assert 0 <= sc.long_plane(name, shape) <= int(coef.max()).bit_length() - 1, (name, shape)
        assert wide == (int(coef.max()).bit_length() > 32), name
        if name in sc.PHASE_CASES:   # the plane the tests cut into is one on which the set releases level 1
            assert sc.release_planes(coef)[1] == sc.long_plane(name, shape), (name, shape)
    for shape in sc.MODEL_SHAPES:
        for name in sc.PHASE_CASES:
            assert sc.release_planes(sc.case(name, shape)[0])[1] == sc.long_plane(name, shape), (name, shape)


@pytest.mark.parametrize("name,shape,e,column,planes", sc.CONDITIONS_2D,
                         ids=["%s-%d-%d-%s" % (c[0], c[1][0], c[2], c[3]) for c in sc.CONDITIONS_2D])
def test_reach_conditions(name, shape, e, column, planes):
    """A list with more entries than k_lis_mx's class ring holds (8192) that is all '0', about half '1' or all '1' on
    the planes the table names; the list of 4^2 sets gets there at 1024 x 1024 only."""
    rows = {p: (L, S) for p, L, S in sc.list_reach(sc.case(name, shape)[0], e)}
    lo, hi = sc.RATIO[column]
    for p in planes:
        L, S = rows[p]
        print("%s %s: list of %d^2 sets, plane %d: L = %d, S = %d" % (name, shape, e, p, L, S))
        assert L > sc.RING, (p, L)
        assert lo <= S / L <= hi, (p, L, S)


def test_reach_figures_at_512():
    """The figures the table is documented with: the list of 2^2 sets on entering the longest plane, and the list of
    4^2 sets, which stays just under the ring at 512 x 512 (hence tiers4_one at 1024 x 1024)."""
    for name, want in sc.LONGEST_2.items():
        assert max(L for _, L, _ in sc.list_reach(sc.case(name)[0], 2)) == want, name
    for name, want in sc.PEAK_4.items():
        assert max(L for _, L, _ in sc.list_reach(sc.case(name)[0], 4)) == want < sc.RING, name
    rows = sc.list_reach(sc.case("checker2")[0], 2)
    assert [r[1:] for r in rows[1:]] == [(32766, 0)] * 23
    for name in ("wide_tiers2_all",):
        L, S = {r[0]: r[1:] for r in sc.list_reach(sc.case(name)[0], 2)}[40]
        assert L > sc.RING and 0.3 <= S / L <= 0.7


I_SHAPES = (sc.SHAPE, sc.RAGGED, sc.FLAT)


@pytest.mark.parametrize("shape", I_SHAPES, ids=["%dx%d" % s for s in I_SHAPES])
def test_type_i_cases_do_to_the_set_what_they_say(oracle, shape):
    """Read from the oracle's stream: the planes before the first release (the set says '0' in one bit a plane: the
    decode of the stream cut in front of the release plane has nothing outside the root band), the levels released
    on each release plane (the decode of the stream cut behind that plane's type-I phase has every coefficient of
    the released levels that the plane finds, and the one cut in front of the phase has none of them)."""
    enc = encoder(oracle)
    xf, root, bl = sc.bands(shape)
    want_release = {"i_dense": {lev: sc.DENSE_TOP for lev in range(1, xf + 1)},
                    "i_stairs": {lev: sc.ROOT_TOP - 3 * (xf - lev + 1) for lev in range(1, xf + 1)},
                    "i_br_only": {lev: 4 + 3 * lev for lev in range(1, xf + 1)},
                    "i_br_first": {lev: sc.ROOT_TOP - 3 * (xf - lev + 1) for lev in range(1, xf + 1)},
                    "i_last_only": {lev: 22 for lev in range(1, xf + 1)},
                    "i_root_only": {}}
    for name in sc.I_CASES:
        coef, sign, _ = sc.case(name, shape)
        rel = sc.release_planes(coef)
        assert rel == want_release[name], name
        full = enc(coef, sign)
        top = full[0] - 1
        outside = np.ones(shape, dtype=bool)
        outside[:root[2], :root[3]] = False
        if not rel:   # i_root_only: '0' on every plane, the whole stream never leaves the root band
            got, _ = oracle.speck2d_decode(full, shape)
            assert np.array_equal(got, coef) and not got[outside].any()
            continue
        first = max(rel.values())
        assert top - first == {"i_dense": 7, "i_stairs": 3, "i_br_first": 3, "i_br_only": sc.ROOT_TOP - (4 + 3 * xf),
                               "i_last_only": 0}[name], (name, top, first)
        for p in sorted(set(rel.values()), reverse=True):
            a, b = sc.i_phase(enc, coef, sign, p)
            start = sc.plane_start(enc, coef, sign, p)
            assert start <= a < b <= sc.plane_start(enc, coef, sign, p - 1), (name, p, a, b)
            levels = [lev for lev, q in rel.items() if q == p]
            mask = np.zeros(shape, dtype=bool)
            for lev, _, y0, x0, ly, lx in bl:
                if lev in levels:
                    mask[y0:y0 + ly, x0:x0 + lx] = True
            found = mask & ((coef >> np.uint64(p)) != 0)
            before, _ = oracle.speck2d_decode(full[:9 + a // 8], shape)
            after, _ = oracle.speck2d_decode(full[:9 + (b + 7) // 8], shape)
            assert not before[mask].any(), (name, p)
            assert found.any() and (after[found] != 0).all(), (name, p)
            cut, mid = sc.cut_into_i_phase(enc, coef, sign, p)
            assert a <= mid < b and 9 + a // 8 <= cut <= 9 + b // 8


@pytest.mark.parametrize("shape", I_SHAPES, ids=["%dx%d" % s for s in I_SHAPES])
def test_i_br_first_finds_listed_subbands_a_plane_later(oracle, shape):
    """TR and BL of level 1 join their lists insignificant on the plane that releases the level and are found there
    on the next one (slice_cases.long_plane), each descending completely: the decode of the stream cut where that
    plane starts has nothing of them, the decode with the plane has all of them, and the plane's list pass alone is
    longer than a region of k_lis_mx."""
    enc = encoder(oracle)
    coef, sign, _ = sc.case("i_br_first", shape)
    p = sc.long_plane("i_br_first", shape)
    assert sc.release_planes(coef)[1] == p + 1
    mask = np.zeros(shape, dtype=bool)
    for lev, name, y0, x0, ly, lx in sc.bands(shape)[2]:
        if lev == 1 and name != "BR":
            assert int(coef[y0:y0 + ly, x0:x0 + lx].min()).bit_length() - 1 == p
            mask[y0:y0 + ly, x0:x0 + lx] = True
    full = enc(coef, sign)
    a, b = sc.plane_start(enc, coef, sign, p), sc.plane_start(enc, coef, sign, p - 1)
    before, _ = oracle.speck2d_decode(full[:9 + a // 8], shape)
    after, _ = oracle.speck2d_decode(full[:9 + (b + 7) // 8], shape)
    assert not before[mask].any() and (after[mask] != 0).all()
    assert b - a - int(np.count_nonzero(coef >> np.uint64(p + 1))) > 2 * int(mask.sum()) > REGION_BITS


def test_release_plane_bit_counts(oracle):
    """i_dense and i_stairs put region boundaries of k_lis_mx (2048 bits) inside the type-I phase: the phase of the
    plane the tests cut into is longer than 16 regions at 512 x 512 and at 301 x 500.  The figures of the whole
    streams and of i_dense's release plane are those the table is documented with."""
    enc = encoder(oracle)
    figures = {}
    for shape in (sc.SHAPE, sc.RAGGED):
        for name in ("i_dense", "i_stairs"):
            coef, sign, _ = sc.case(name, shape)
            p = sc.long_plane(name, shape)
            a, b = sc.i_phase(enc, coef, sign, p)
            plane = sc.plane_start(enc, coef, sign, p - 1) - sc.plane_start(enc, coef, sign, p)
            print("%s %s: plane %d has %d bits, its type-I phase %d .. %d" % (name, shape, p, plane, a, b))
            assert b - a > 16 * REGION_BITS, (name, shape, a, b)
            full = enc(coef, sign)
            figures[name, shape] = (full[0], total_bits(full), plane)
    assert figures["i_dense", sc.SHAPE] == (27, 5592860, 611584)
    assert figures["i_stairs", sc.SHAPE][:2] == (27, 2970919)
    assert figures["i_dense", sc.RAGGED][2] == 385788
    coef, sign, _ = sc.case("i_stairs")
    starts = [sc.plane_start(enc, coef, sign, p) for p in range(26, 18, -1)]
    assert [y - x for x, y in zip(starts, starts[1:])] == [150, 65, 65, 513, 257, 257, 2049]


@pytest.mark.parametrize("shape", I_SHAPES, ids=["%dx%d" % s for s in I_SHAPES])
def test_implied_tests_of_i_last_only(oracle, shape):
    """The phase's bit count derived from the band list, with the test of the remaining set implied after every
    level but the last, is the oracle's; were those tests coded, it would be longer by their number."""
    enc = encoder(oracle)
    coef, sign, _ = sc.case("i_last_only", shape)
    bits, implied = sc.implied_tests(shape)
    a, b = sc.i_phase(enc, coef, sign, 22)
    assert implied == sc.bands(shape)[0] - 1
    assert (a, b - a) == (1, bits), (a, b, bits, implied)
    full = enc(coef, sign)
    assert full[0] == 23 and sc.plane_start(enc, coef, sign, 21) == b   # (nothing to refine on the first plane)
    if shape == sc.SHAPE:
        assert total_bits(full) == 999


@pytest.mark.parametrize("name,shape", [("tiers2_all", sc.SHAPE), ("i_stairs", sc.RAGGED), ("i_last_only", sc.FLAT),
                                        ("stagger4_one", sc.RAGGED)])
def test_plane_cut_against_the_oracle(oracle, name, shape):
    """What places the GPU tests' cut one byte into plane p: the stream in front of plane p is, bit for bit, the whole
    stream of the coefficients shifted down by p + 1, and a decode of the cut stream has every bit above plane p and
    not all of plane p."""
    enc = encoder(oracle)
    coef, sign, _ = sc.case(name, shape)
    full = enc(coef, sign)
    p = sc.long_plane(name, shape)
    head = enc(sc.bits_down_to(coef, p), sign)
    nbits, total = total_bits(head), total_bits(full)
    assert head[0] == full[0] - (p + 1) and 0 <= nbits < total and (nbits > 0) == (p + 1 < full[0])
    whole = nbits // 8
    assert head[9:9 + whole] == full[9:9 + whole]
    if nbits % 8:
        mask = (1 << (nbits % 8)) - 1
        assert head[9 + whole] & mask == full[9 + whole] & mask
    cut = sc.cut_into_plane(enc, coef, sign, p)
    assert 9 + whole < cut <= len(full)
    got, _ = oracle.speck2d_decode(full[:cut], shape)
    assert np.array_equal(got >> np.uint64(p + 1), coef >> np.uint64(p + 1))
    assert not np.array_equal(got >> np.uint64(p), coef >> np.uint64(p))


def test_graft_body_decodes_to_the_pattern(oracle):
    """A grafted body decodes through oracle.decomp_2d, and the result changes when one coefficient of the pattern
    does; a constant slice's header is refused."""
    shape = (37, 50)
    header = sc.header_of(oracle, shape)
    assert len(header) == 17
    coef, sign, _ = sc.case("i_stairs", shape)
    a = oracle.decomp_2d(sc.graft_body(header, oracle.speck2d_encode(coef, sign, 0)), shape, False)
    other = np.array(coef)
    other[20, 30] ^= np.uint64(1 << 9)
    b = oracle.decomp_2d(sc.graft_body(header, oracle.speck2d_encode(other, sign, 0)), shape, False)
    assert a.shape == shape and np.isfinite(a).all() and not np.array_equal(a, b)
    const = oracle.comp_2d(np.full(shape, 3.0, dtype=np.float32), 1, 2.0)
    assert len(const) == 17
    with pytest.raises(AssertionError):
        sc.graft_body(const, b"")
