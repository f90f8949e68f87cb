"""CPU: the case table of the SPECK list kernels (tests/coef_cases.py) does to the lists what it is built for.  The
conditions are read off the reach model `list_reach`, a property of the input alone; one test ties that model to the
coder, through the oracle's stream."""
import numpy as np
import pytest

import coef_cases as cc


@pytest.mark.parametrize("name,e,column,planes", cc.CONDITIONS,
                         ids=["%s-%d-%s" % c[:3] for c in cc.CONDITIONS])
def test_reach_conditions(name, e, column, planes):
    """A long list (512 entries of 8^3 sets, what k_lis_l2 starts at; 4096 of 4^3 and 2^3 sets) that is almost all
    '0', about half '1', or all '1', on the planes the table names."""
    coef, _, _ = cc.case(name)
    rows = {p: (L, S) for p, L, S in cc.list_reach(coef, e)}
    lo, hi = cc.RATIO[column]
    for p in planes:
        L, S = rows[p]
        print("%s: list of %d^3 sets, plane %d: L = %d, S = %d" % (name, e, p, L, S))
        assert L >= cc.L_MIN[e], (p, L)
        assert lo <= S / L <= hi, (p, L, S)


def test_reach_of_the_patterns_without_a_column():
    """stagger8_one: the list of 8^3 sets is long on 26 planes and its length differs from plane to plane; front4: the
    list of 4^3 sets is long and the entries a plane finds significant are one run of box numbers; the wide cases have
    long lists above plane 32; the single-coefficient extremes keep seven entries per list, all_one and dense_top32
    none (every set splits on the first plane)."""
    rows = cc.list_reach(cc.case("stagger8_one")[0], 8)
    long_rows = [r for r in rows if r[1] >= cc.L_MIN[8]]
    assert len(long_rows) >= cc.STAGGER8_LONG_PLANES and len({r[1] for r in long_rows}) == len(long_rows)
    coef = cc.case("front4")[0]
    rows = cc.list_reach(coef, 4)
    assert sum(1 for r in rows if r[1] >= cc.L_MIN[4]) >= 20
    own = cc.box_tops(coef, 4).reshape(-1)
    for p in (20, 13, 5):
        b = np.nonzero(own == p)[0]
        span = own[b[0]:b[-1] + 1]   # (the first children among them took plane 27)
        assert b.size > 900 and set(np.unique(span).tolist()) <= {p, 27}, p
    for name, e, p in (("wide_tiers8_all", 8, 40), ("wide_stagger4_one", 4, 36), ("wide_stagger4_one", 2, 33)):
        L, S = {r[0]: r[1:] for r in cc.list_reach(cc.case(name)[0], e)}[p]
        assert cc.case(name)[2] and L >= cc.L_MIN[e], (name, e, p, L)
    for name, most in (("first_only", 7), ("last_only", 7), ("all_one", 0), ("dense_top32", 0)):
        for e in (8, 4, 2):
            assert max(r[1] for r in cc.list_reach(cc.case(name)[0], e)) == most, (name, e)


def test_every_case_names_a_plane_it_has():
    for name in cc.CASES:
        coef = cc.case(name)[0]
        assert 0 <= cc.LONG_PLANE[name] <= int(coef.max()).bit_length() - 1, name
    assert set(cc.MX_CASES) <= set(cc.CASES) and set(cc.LONG_PLANE) == set(cc.CASES)


@pytest.mark.parametrize("name", ["tiers8_all", "stagger8_one", "last_only"])
def test_reach_model_and_plane_cut_against_the_oracle(oracle, name):
    """What places the GPU tests' cut one byte into plane p: the stream in front of plane p is, bit for bit, the whole
    stream of the coefficients shifted down by p + 1 (bits_down_to), and a decode of the cut stream has every bit
    above plane p and not all of plane p."""
    coef, sign, _ = cc.case(name)
    full = oracle.speck3d_encode(coef, sign, 0)
    p = cc.LONG_PLANE[name]
    head = oracle.speck3d_encode(cc.bits_down_to(coef, p), sign, 0)
    nbits = int(np.frombuffer(head, dtype=np.uint64, count=1, offset=1)[0])
    total = int(np.frombuffer(full, dtype=np.uint64, count=1, offset=1)[0])
    assert head[0] == full[0] - (p + 1) and 0 <= nbits < total and (nbits > 0) == (p + 1 < full[0])
    whole = nbits // 8
    assert head[9:9 + whole] == full[9:9 + whole]
    if nbits % 8:
        mask = (1 << (nbits % 8)) - 1
        assert head[9 + whole] & mask == full[9 + whole] & mask
    cut = cc.cut_into_plane(lambda c, s: oracle.speck3d_encode(c, s, 0), coef, sign, p)
    assert 9 + whole < cut <= len(full)
    # the decode of the cut stream has every bit above plane p and not yet all of plane p
    got, _ = oracle.speck3d_decode(full[:cut], coef.shape)
    assert np.array_equal(got >> np.uint64(p + 1), coef >> np.uint64(p + 1))
    assert not np.array_equal(got >> np.uint64(p), coef >> np.uint64(p))


def test_graft_speck_keeps_the_other_chunks(oracle):
    from fields import smooth_field
    from sperr_amd.farm import split_container
    v = smooth_field((16, 16, 48))
    base = oracle.comp_3d(v, (16, 16, 16), 1, 4.0)
    coef, sign, _ = cc.coefficient_pattern("last_only", (16, 16, 16))
    s = oracle.speck3d_encode(coef, sign, 0)
    got = cc.graft_speck(base, {1: s})
    a, b = split_container(base)[3], split_container(got)[3]
    assert a[0] == b[0] and a[2] == b[2] and b[1] == bytes(a[1][:17]) + s
    dec, ref = oracle.decomp_3d(got, False), oracle.decomp_3d(base, False)
    assert np.array_equal(dec[:, :, :16], ref[:, :, :16]) and np.array_equal(dec[:, :, 32:], ref[:, :, 32:])
    assert not np.array_equal(dec[:, :, 16:32], ref[:, :, 16:32])
