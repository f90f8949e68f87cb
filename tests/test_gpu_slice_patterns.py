"""GPU (-m gpu): the 2D coder and k_lis_mx on the case table of tests/slice_cases.py -- coefficient patterns aligned
to the quadtree forest of a slice, which keep the lists of the 2^2 sets beyond the 8192 entries of k_lis_mx's class
ring, and patterns that choose what the type-I set does on every plane (tests/test_slice_cases_host.py asserts that
of the patterns).

The yardstick is the oracle, which tests/test_oracle_vs_ref.py::test_slice_patterns_bit_exact pins to the real
reference on the same cases; every compare is on bytes or bit patterns.

  stage parity    eng.speck2d_encode / _decode (plan key (x, y, 0): the 2D forest) against the oracle: the encoder at
                  budgets 0, 200000 and one that ends inside the release plane's type-I phase; the decoder on the
                  stream whole, cut to 1/2 and 1/7, cut one byte into the long plane and cut inside that phase
  a batch         six different bodies of one shape in one decompress_2d_batch call
  multi-res       decompress_2d_multires of grafted bodies
  hand-over       SPERR_HIP_MX_WGS = 1, 3, 4096 in fresh processes
  witnesses       the per-path counters of k_lis_mx's <true> instantiation, per case"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import slice_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
_cache = {}


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    return SperrHip()


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: the cached cases are read-only)


def dev_of(stream):
    return cuda(np.frombuffer(stream, dtype=np.uint8))


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def encoder(oracle):
    return lambda c, s: oracle.speck2d_encode(c, s, 0)


def case_stream(oracle, name, shape):
    def make():
        coef, sign, _ = sc.case(name, shape)
        return oracle.speck2d_encode(coef, sign, 0)
    return cached(("stream", name, shape), make)


def body(oracle, name, shape):
    """the case's stream behind the conditioner header of a smooth slice of the same shape"""
    header = cached(("header", shape), lambda: sc.header_of(oracle, shape))
    return cached(("body", name, shape), lambda: sc.graft_body(header, case_stream(oracle, name, shape)))


def oracle_slice(oracle, key, stream, shape, as_float):
    want = cached(("decode", key, shape, as_float), lambda: oracle.decomp_2d(stream, shape, as_float))
    want.setflags(write=False)
    return want


def i_cut(oracle, name, shape):
    """(stream length, bit budget) in the middle of the type-I phase of the case's release plane, or None"""
    if name not in sc.PHASE_CASES:
        return None
    coef, sign, _ = sc.case(name, shape)
    p = sc.long_plane(name, shape)
    return cached(("icut", name, shape), lambda: sc.cut_into_i_phase(encoder(oracle), coef, sign, p))


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


# ---- a. stage parity -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", sc.ALL_CASES, ids=sc.CASE_IDS)
def test_stage_parity(eng, oracle, name, shape):
    """Every (case, shape) of the table.  The encoder's bytes at budgets 0 and 200000 and, for the type-I cases, at a
    budget that ends in the middle of the release plane's type-I phase (k_enc_iphase stops inside it).  The decoder's
    coefficients and signs of the stream whole, cut to 1/2 and 1/7 of its payload, cut one byte into the plane the
    table names (slice_cases.long_plane) and, for the type-I cases, cut in the middle of that phase, so that the
    stream ends in k_lis_mx's kModeISub / kModeISubWalk.  The launch profile of the whole decode names k_lis_mx and
    none of k_lis_l0 / _hi / _walk."""
    coef, sign, wide = sc.case(name, shape)
    dcoef = cuda(coef.view(np.int64) if wide else coef.astype(np.uint32).view(np.int32))
    dsign = cuda(sign.view(np.int64))
    full = case_stream(oracle, name, shape)
    mid = i_cut(oracle, name, shape)
    for budget in (0, 200000) + ((mid[1],) if mid else ()):
        want = full if budget == 0 else oracle.speck2d_encode(coef, sign, budget)
        got = eng.speck2d_encode(dcoef, dsign, budget)
        assert got[:9] == want[:9], budget
        assert got == want, budget
    p = sc.long_plane(name, shape)
    into_plane = sc.cut_into_plane(encoder(oracle), coef, sign, p)
    assert 9 < into_plane <= len(full)
    launched = {}
    for cut in sc.stream_cuts(full) + (into_plane,) + ((mid[0],) if mid else ()):
        c0, s0 = oracle.speck2d_decode(full[:cut], shape)
        if cut == len(full):
            launched = profile_names(eng, lambda: eng.speck2d_decode(full[:cut], shape))
        c1, s1 = eng.speck2d_decode(full[:cut], shape)
        assert np.array_equal(c0, c1), (cut, p)
        assert np.array_equal(s0, s1), (cut, p)
    assert any("k_lis_mx" in n for n in launched), sorted(launched)
    assert not any("k_lis_l0" in n or "k_lis_hi" in n or "k_lis_walk" in n for n in launched), sorted(launched)


# ---- b. a batch of different slices ----------------------------------------------------------------------------------

BATCH = ("tiers2_all", "i_last_only", "wide", "i_dense", "constant", "i_dense cut to 30 %")
WIDE_OF = {sc.SHAPE: "wide_i_stairs", sc.RAGGED: "wide_tiers2_all"}   # (the table has wide cases at SHAPE only)


def batch_bodies(oracle, shape):
    def make(entry):
        if entry == "constant":
            s = oracle.comp_2d(np.full(shape, 2.5, dtype=np.float32), 1, 2.0)
            assert len(s) == 17
            return s
        if entry == "wide":
            return body(oracle, WIDE_OF[shape], shape)
        if entry.endswith("cut to 30 %"):
            whole = body(oracle, "i_dense", shape)
            return whole[:len(whole) * 30 // 100]
        return body(oracle, entry, shape)
    return [make(entry) for entry in BATCH]


@pytest.mark.parametrize("shape", [sc.SHAPE, sc.RAGGED], ids=["512x512", "301x500"])
def test_a_batch_of_different_slices(eng, oracle, shape):
    """tiers2_all, i_last_only, a wide case, i_dense, a constant slice's 17 bytes and i_dense cut to 30 % as the six
    slices of one decompress_2d_batch call: a slice whose type-I phase runs to some 300 regions beside one whose
    phases are a few bits, and one slice on the 64-bit pass alone.  As float and as double, every slice against
    oracle.decomp_2d of its own body and against the bits of a decompress_2d call of its own."""
    bodies = batch_bodies(oracle, shape)
    assert bodies[2][17] > 32 and all(b[17] <= 32 for k, b in enumerate(bodies) if k not in (2, 4))
    devs = [dev_of(b) for b in bodies]
    for as_float in (True, False):
        got = eng.decompress_2d_batch(devs, shape, as_float).cpu().numpy()
        assert got.shape == (len(bodies),) + shape
        for k, b in enumerate(bodies):
            want = oracle_slice(oracle, ("batch", k), b, shape, as_float)
            assert same(got[k], want), (BATCH[k], as_float)
            assert same(eng.decompress_2d(devs[k], shape, as_float).cpu().numpy(), want), (BATCH[k], as_float)


# ---- c. multi-resolution ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [sc.SHAPE, sc.RAGGED], ids=["512x512", "301x500"])
@pytest.mark.parametrize("name", ["i_stairs", "tiers2_all"])
def test_multi_resolution(eng, oracle, name, shape):
    """decompress_2d_multires of the grafted body: the slice and every level against oracle.decomp_2d_multi_res."""
    b = body(oracle, name, shape)
    want, want_lv = oracle.decomp_2d_multi_res(b, shape)
    assert len(want_lv) > 0 and eng.multires_levels_2d(shape) == [lv.shape for lv in want_lv]
    for as_float in (True, False):
        got, got_lv = eng.decompress_2d_multires(dev_of(b), shape, as_float)
        assert same(got.cpu().numpy(), want.astype(np.float32) if as_float else want), as_float
        assert len(got_lv) == len(want_lv)
        for h, (a, lv) in enumerate(zip(got_lv, want_lv)):
            assert same(a.cpu().numpy(), lv), (h, as_float)


@pytest.mark.parametrize("shape", [sc.FLAT, (20, 1100), (2, 10, 1100)], ids=["9x2048", "20x1100", "2x10x1100"])
def test_rows_too_long_for_the_fused_xy_pass(eng, oracle, shape):
    """Rows of 1088 samples and more leave the fused x-y transform kernel no tile in LDS.  Its row count went negative
    there and passed for a large one, the launch asked for more LDS than a workgroup has, and every compress and
    decompress of such a slice or chunk returned -1 (found by test_witnesses at 9 x 2048, the first whole-pipeline
    call at that shape).  The separate passes take these shapes: compress and decompress against the oracle's bytes
    and bits."""
    import torch
    if len(shape) == 2:
        img = sc.smooth_slice(shape)
        want = oracle.comp_2d(img, 1, 3.0)
        assert bytes(eng.compress_2d(torch.from_numpy(img).cuda(), 3.0).cpu().numpy()) == want
        for as_float in (True, False):
            assert same(eng.decompress_2d(dev_of(want), shape, as_float).cpu().numpy(),
                        oracle.decomp_2d(want, shape, as_float)), as_float
    else:
        from fields import smooth_field
        vol = smooth_field(shape)
        chunks = shape[::-1]
        want = oracle.comp_3d(vol, chunks, 1, 3.0)
        assert bytes(eng.compress(torch.from_numpy(vol).cuda(), chunks, 3.0).cpu().numpy()) == want
        for as_float in (True, False):
            assert same(eng.decompress(dev_of(want), as_float).cpu().numpy(), oracle.decomp_3d(want, as_float))


# ---- d. workgroup hand-over in fresh processes -----------------------------------------------------------------------

_CHILD = r"""
import ctypes as C, json, os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
td, dy, dx = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
from sperr_amd.api import SperrHip
e = SperrHip()
res = {}
for name in sys.argv[5:]:
    c = torch.from_numpy(np.load(os.path.join(td, name + ".c.npy"))).cuda()
    r = np.load(os.path.join(td, name + ".r.npy"))
    d = e.decompress_2d(c, (dy, dx), False).cpu().numpy()
    res[name] = bool(d.shape == r.shape and np.array_equal(d.view(np.uint64), r.view(np.uint64)))
with open(os.path.join(td, "out.json"), "w") as f:
    json.dump(res, f)
"""
HANDOVER = ("i_dense", "i_last_only", "tiers2_all")


@pytest.mark.parametrize("wgs", ["1", "3", "4096"])
def test_workgroup_hand_over_in_a_fresh_process(oracle, wgs):
    """SPERR_HIP_MX_WGS is read once per process: one child per value -- 1: one workgroup takes every region itself;
    3; 4096: as many as the kernel allows -- decodes the grafted i_dense (a type-I phase of some 190 regions, handed
    from workgroup to workgroup), i_last_only and tiers2_all bodies at 301 x 500, and the parent checks the doubles
    against the oracle's bits."""
    shape = sc.RAGGED
    with tempfile.TemporaryDirectory() as td:
        for name in HANDOVER:
            b = body(oracle, name, shape)
            np.save(os.path.join(td, name + ".c.npy"), np.frombuffer(b, dtype=np.uint8))
            np.save(os.path.join(td, name + ".r.npy"), oracle_slice(oracle, ("body", name), b, shape, False))
        env = dict(os.environ, SPERR_HIP_MX_WGS=wgs)
        run = subprocess.run([sys.executable, "-c", _CHILD, ROOT, td, str(shape[0]), str(shape[1])] + list(HANDOVER),
                             env=env, timeout=120)
        assert run.returncode == 0, wgs
        with open(os.path.join(td, "out.json")) as f:
            res = json.load(f)
    assert res == {name: True for name in HANDOVER}, (wgs, res)


# ---- e. witnesses ----------------------------------------------------------------------------------------------------

# k_lis_mx's <true> instantiation counts its paths per slice (speck_mx.hip, the wk_* counters, written to words 0-25
# of the slice's 64): these are the words whose paths the table has to reach.
#   18  is out of a slice's reach: only classes up to three steps above the leaf parents have one of the sixteen
#       columns (speck_tree_host.hpp, build_mx_columns), in 2D sets of 16 x 16 at most, whose split is 597 bits at
#       most -- and the rows look kMxM = 768 bits past the region.  In 3D such a set has up to 16^3 samples:
#       test_witness_of_a_split_that_leaves_the_rows reads it from coef_cases.checker8 at 100 x 128 x 128.
#   21  ("reloads") is declared, written out and reset in speck_mx.hip but incremented nowhere: the window of entry
#       classes is rolled along inside the tight loop's asm statement since that statement took the whole loop, so no
#       stream can make it nonzero and no case is asked for it.
WORDS = {0: "regions", 6: "ring refills", 10: "tight hops", 11: "general hops", 12: "walk rounds",
         16: "handed over: saturated", 17: "handed over: outside the list's two column groups",
         18: "handed over: leaves the rows", 19: "handed over: no column", 20: "enters", 21: "reloads"}
UNREACHABLE = {21}
WORDS_3D = {18}

# Which case witnesses which word, with the values measured on an MI355X: {(case, shape): {word: measured}}.  The
# test asserts "nonzero" of every word listed for its case (the counts of regions and of what depends on where a
# region ends differ by a few from run to run: workgroups take regions as they come), and
# test_witness_table_names_every_word that the table leaves no word of WORDS out.
WITNESS = {
    ("i_dense", sc.SHAPE): {0: 513, 12: 808},
    ("i_dense", sc.RAGGED): {0: 402, 12: 518},
    ("i_last_only", sc.SHAPE): {0: 184, 6: 177},
    ("tiers2_all", sc.SHAPE): {0: 768, 6: 50, 10: 32550, 11: 87, 12: 446, 16: 87, 20: 452},
    ("wide_tiers2_all", sc.SHAPE): {10: 32551, 20: 420},
    ("front4", sc.SHAPE): {10: 11180, 11: 688, 12: 10512, 16: 688, 20: 758},
    ("stagger4_one", sc.SHAPE): {6: 185, 10: 14005, 11: 1440, 16: 541, 17: 6, 20: 1480},
    ("stagger4_one", sc.RAGGED): {6: 201, 10: 7169, 11: 1489, 12: 2598, 16: 274, 17: 15, 19: 8, 20: 1438},
    ("stagger4_one", sc.FLAT): {6: 236, 10: 283, 11: 790, 12: 3313, 16: 30, 17: 30, 19: 9, 20: 506},
    ("tiers2_all", sc.FLAT): {10: 3553, 11: 272, 12: 2294, 16: 251, 20: 149},
    ("i_br_first", sc.SHAPE): {11: 13, 12: 708, 16: 5},
    ("tiers4_one", sc.BIG): {0: 2439, 6: 99, 10: 32547, 11: 90, 12: 18652, 16: 89, 20: 2152},
}
WITNESS_3D = {("checker8", (100, 128, 128)): {18: 7}}


def decode_with_stamps(eng, stream, shape):
    """(the slice as doubles, the 64 counters of the slice) of one decompress_2d call through k_lis_mx<true>"""
    eng.lib.sperrhip_debug_lis_stamps.argtypes = [C.c_int, C.c_void_p]
    out = (C.c_ulonglong * 64)()
    eng.lib.sperrhip_debug_lis_stamps(1, None)
    try:
        got = eng.decompress_2d(dev_of(stream), shape, False).cpu().numpy()
    finally:
        eng.lib.sperrhip_debug_lis_stamps(0, out)
    return got, [int(w) for w in out]


@pytest.mark.parametrize("name,shape", sc.ALL_CASES, ids=sc.CASE_IDS)
def test_witnesses(eng, oracle, name, shape):
    """One case at a time as a single slice through the counting instantiation of k_lis_mx: the oracle's bits, and
    every counter the table names for this case is nonzero.  i_dense goes through at least as many regions as its
    release plane alone has (its bits / 2048)."""
    b = body(oracle, name, shape)
    got, words = decode_with_stamps(eng, b, shape)
    assert same(got, oracle_slice(oracle, ("body", name), b, shape, False))
    print("WITNESS %s %dx%d %s" % (name, shape[0], shape[1], json.dumps({w: words[w] for w in sorted(WORDS)})))
    for w in WITNESS.get((name, shape), {}):
        assert words[w] != 0, (w, WORDS[w])
    if name == "i_dense":
        coef, sign, _ = sc.case(name, shape)
        enc = encoder(oracle)
        plane = sc.plane_start(enc, coef, sign, sc.DENSE_TOP - 1) - sc.plane_start(enc, coef, sign, sc.DENSE_TOP)
        assert words[0] >= plane // 2048, (words[0], plane)


def test_witness_of_a_split_that_leaves_the_rows(eng, oracle):
    """Word 18 needs a set with a column whose split is longer than the rows look ahead, which a slice does not have
    (see WORDS): coef_cases.checker8 at 100 x 128 x 128, dense 8^3 boxes whose splits run to a thousand bits and
    more, grafted into a one-chunk container and decoded with the counters on, against the oracle's bits."""
    import coef_cases as cc
    from fields import smooth_field
    (name, shape), row = next(iter(WITNESS_3D.items()))
    assert shape == cc.MX_SHAPE
    base = oracle.comp_3d(smooth_field(shape), shape[::-1], 1, 2.0)
    coef, sign, _ = cc.case(name, shape)
    c = cc.graft_speck(base, {0: oracle.speck3d_encode(coef, sign, 0)})
    eng.lib.sperrhip_debug_lis_stamps.argtypes = [C.c_int, C.c_void_p]
    out = (C.c_ulonglong * 64)()
    eng.lib.sperrhip_debug_lis_stamps(1, None)
    try:
        got = eng.decompress(dev_of(c), False).cpu().numpy()
    finally:
        eng.lib.sperrhip_debug_lis_stamps(0, out)
    assert same(got, oracle.decomp_3d(c, False))
    print("WITNESS %s %dx%dx%d %s" % ((name,) + shape + (json.dumps({w: int(out[w]) for w in sorted(WORDS)}),)))
    for w in row:
        assert out[w] != 0, (w, WORDS[w])


def test_witness_table_names_every_word():
    named = {w for row in WITNESS.values() for w in row}
    assert named == set(WORDS) - UNREACHABLE - WORDS_3D, sorted(set(WORDS) - named)
    assert {w for row in WITNESS_3D.values() for w in row} == WORDS_3D
    assert all(key in sc.ALL_CASES for key in WITNESS)
