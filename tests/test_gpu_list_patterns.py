"""GPU (-m gpu): the decoder's list kernels on the case table of tests/coef_cases.py -- 128^3 coefficient patterns
aligned to the set tree, which keep the lists of the 2^3, 4^3 and 8^3 sets (k_lis_l0 / _l1 / _l2) thousands of
entries long and make them all '0', half '1' or all '1' (tests/test_coef_cases_host.py asserts that of the patterns).

The yardstick is the oracle, which tests/test_oracle_vs_ref.py::test_tree_aligned_patterns_bit_exact pins to the
real reference on the same cases; every compare is on bytes or bit patterns.

  stage parity    eng.speck3d_encode / _decode against the oracle, the stream whole, cut to 1/2 and 1/7 of its
                  payload and cut one byte into the plane whose list is long
  four chunks     four different streams grafted into one container: a long-list chunk decodes beside a nearly
                  empty one in each sub-batch, and in one variant beside a chunk that takes the 64-bit pass
  witnesses       that k_lis_l0 / _l1 / _l2 and, at 100 x 128 x 128, k_lis_mx did the work"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import coef_cases as cc
from fields import smooth_field

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


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


def dev_of(container):
    return cuda(np.frombuffer(container, dtype=np.uint8))


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


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

def stage_parity(eng, oracle, name, shape):
    """-> the kernels the decode of the whole stream launched"""
    coef, sign, wide = cc.case(name, shape)
    dcoef = cuda(coef.view(np.int64) if wide else coef.astype(np.uint32).view(np.int32))
    dsign = cuda(sign.view(np.int64))
    for budget in (0, 200000):
        want = oracle.speck3d_encode(coef, sign, budget)
        got = eng.speck3d_encode(dcoef, dsign, budget)
        assert got[:9] == want[:9], budget
        assert got == want, budget
        if budget == 0:
            full = want
    p = cc.LONG_PLANE[name]
    into_plane = cc.cut_into_plane(lambda c, s: oracle.speck3d_encode(c, s, 0), coef, sign, p)
    assert 9 < into_plane <= len(full)
    launched = {}
    for cut in cc.stream_cuts(full) + (into_plane,):
        c0, s0 = oracle.speck3d_decode(full[:cut], shape)
        if cut == len(full):
            launched = profile_names(eng, lambda: eng.speck3d_decode(full[:cut], shape))
        c1, s1 = eng.speck3d_decode(full[:cut], shape)
        assert np.array_equal(c0, c1), (cut, p)
        assert np.array_equal(s0, s1), (cut, p)
    return launched


@pytest.mark.parametrize("name", cc.CASES)
def test_stage_parity(eng, oracle, name):
    """Every table case at 128^3: the encoder's bytes at budgets 0 and 200000, and the decoder's coefficients and
    signs of the stream whole, cut to 1/2 and 1/7 of its payload and cut one byte into the plane the table names as
    the one whose list is long (coef_cases.LONG_PLANE; the cut comes from a second oracle encode, cut_into_plane).
    The shape is one the table kernels take: the three block-parallel list kernels are launched for it."""
    launched = stage_parity(eng, oracle, name, cc.SHAPE)
    for k in ("k_lis_l0", "k_lis_l1", "k_lis_l2"):
        assert any(k in n for n in launched), (k, sorted(launched))
    assert not any("k_lis_mx" in n for n in launched)


MX_PARAMS = ([pytest.param(name, cc.MX_SHAPE, id=name) for name in cc.MX_CASES]
             + [pytest.param(name, cc.MX_CUBE, id="%s-%dx%dx%d" % ((name,) + cc.MX_CUBE)) for name in cc.MX_CUBE_CASES])


@pytest.mark.parametrize("name,shape", MX_PARAMS)
def test_stage_parity_where_the_lists_mix_set_shapes(eng, oracle, name, shape):
    """The same at 100 x 128 x 128: the boxes are no longer the coder's sets along z, the lists mix set shapes, and the
    launch profile says k_lis_mx decoded them.  At 100 x 100 x 100 no axis is dyadic."""
    launched = stage_parity(eng, oracle, name, shape)
    assert any("k_lis_mx" in n for n in launched), sorted(launched)
    assert not any("k_lis_l0" in n or "k_lis_hi" in n for n in launched)


# ---- b. four different chunks in one call ----------------------------------------------------------------------------

CHUNKS = (128, 128, 128)
FOUR = {"narrow": ("stagger8_one", "all_one", "last_only", "tiers2_all"),
        "wide": ("stagger8_one", "wide_tiers8_all", "last_only", "tiers2_all")}
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def base_container(oracle):
    """four 128^3 chunks side by side along x, each with a conditioner header of its own"""
    return cached("base", lambda: oracle.comp_3d(smooth_field((128, 128, 512)), CHUNKS, 1, 2.0))


def case_stream(oracle, name):
    def make():
        coef, sign, _ = cc.case(name)
        return oracle.speck3d_encode(coef, sign, 0)
    return cached(("stream", name), make)


def grafted(oracle, names):
    """the base container with chunk k's SPECK stream replaced by the stream of case names[k] (None: kept)"""
    return cached(("grafted", names), lambda: cc.graft_speck(
        base_container(oracle), {k: case_stream(oracle, n) for k, n in enumerate(names) if n is not None}))


def oracle_decode(oracle, key, container, as_float):
    want = cached(("decode", key, as_float), lambda: oracle.decomp_3d(container, as_float, 4))
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("variant", sorted(FOUR))
@pytest.mark.parametrize("part", ["whole", "cut to 30 %"])
def test_four_different_chunks_in_one_call(eng, oracle, variant, part):
    """stagger8_one, all_one (wide: wide_tiers8_all), last_only, tiers2_all as the four chunks of one container: the
    four decode as two sub-batches, each a long-list chunk beside a nearly empty one, with 31 planes against 1 in the
    first (wide: against 53, and that chunk alone takes the 64-bit pass) and 3 against 27 in the second.  Float and
    double, the container whole and cut by sperr_trunc_3d to 30 %, against the oracle's bits."""
    c = grafted(oracle, FOUR[variant])
    if part != "whole":
        c = cached(("trunc", variant), lambda: oracle.trunc_3d(c, 30))
        assert len(c) < len(grafted(oracle, FOUR[variant]))
    dev = dev_of(c)
    for as_float in (True, False):
        want = oracle_decode(oracle, (variant, part), c, as_float)
        assert same(eng.decompress(dev, as_float).cpu().numpy(), want), as_float


@pytest.mark.parametrize("variant", sorted(FOUR))
def test_four_different_chunks_box_and_levels(eng, oracle, variant):
    """One box across all four chunks, and every level of the hierarchy, of the same containers."""
    c = grafted(oracle, FOUR[variant])
    dev = dev_of(c)
    lo, dims = (100, 30, 40), (300, 50, 40)   # x 100..399: chunks 0 to 3
    for as_float in (True, False):
        want = oracle_decode(oracle, (variant, "whole"), c, as_float)
        crop = np.ascontiguousarray(want[lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]])
        assert same(eng.decompress_box(dev, lo, dims, as_float).cpu().numpy(), crop), as_float
    levels = oracle.decomp_3d_multi_res(c, 4)[1]
    assert len(levels) > 0 and eng.multires_levels((128, 128, 512), CHUNKS) == [lv.shape for lv in levels]
    for h, lv in enumerate(levels):
        assert same(eng.decompress_level(dev, h, output_float=False).cpu().numpy(), lv), h
        assert same(eng.decompress_level(dev, h, output_float=True).cpu().numpy(), lv.astype(np.float32)), h


# ---- c. witnesses ------------------------------------------------------------------------------------------------

def test_k_lis_l1_handled_blocks_of_the_long_list(eng, oracle):
    """A list kernel that gives up hands its list to k_lis_hi, which decodes the same bits.  With the decoder's tick
    counters on (sperrhip_debug_lis_stamps), word 56 counts the blocks k_lis_l1 finished for the first chunk
    (speck_dec.hip, k_lis_l1: l1stamps).  The first chunk is stagger8_one, whose list of 4^3 sets grows to 27 804
    entries that are all '0'."""
    c = grafted(oracle, FOUR["narrow"])
    eng.lib.sperrhip_debug_lis_stamps.argtypes = [C.c_int, C.c_void_p]
    out = (C.c_ulonglong * 64)()
    eng.lib.sperrhip_debug_lis_stamps(1, None)
    try:
        got = eng.decompress(dev_of(c), True).cpu().numpy()
    finally:
        eng.lib.sperrhip_debug_lis_stamps(0, out)
    assert same(got, oracle_decode(oracle, ("narrow", "whole"), c, True))
    print("k_lis_l1 handled %d blocks of the first chunk (stagger8_one)" % out[56])
    assert out[56] != 0


_CHILD = r"""
import ctypes as C, json, os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
td = sys.argv[2]
from sperr_amd.api import SperrHip
e = SperrHip()
e.lib.sperrhip_debug_lis_stamps.argtypes = [C.c_int, C.c_void_p]
res = {}
for name in sys.argv[3:]:
    c = torch.from_numpy(np.load(os.path.join(td, name + ".c.npy"))).cuda()
    r = np.load(os.path.join(td, name + ".r.npy"))
    out = (C.c_ulonglong * 64)()
    e.lib.sperrhip_debug_lis_stamps(1, None)
    try:
        d = e.decompress(c, True).cpu().numpy()
    finally:
        e.lib.sperrhip_debug_lis_stamps(0, out)
    res[name] = {"same": bool(d.shape == r.shape and np.array_equal(d.view(np.uint32), r.view(np.uint32))),
                 "words": [int(w) for w in out]}
with open(os.path.join(td, "out." + sys.argv[3] + "." + str(os.getpid()) + ".json"), "w") as f:
    json.dump(res, f)
"""


def child_decode(td, names, knobs):
    """a fresh process (the knobs are read once per process) decodes td/<name>.c.npy with the tick counters on:
    {name: {"same": its floats are td/<name>.r.npy bit for bit, "words": the 64 counters of the first chunk}}"""
    before = set(os.listdir(td))
    env = dict(os.environ, **knobs)
    assert subprocess.run([sys.executable, "-c", _CHILD, ROOT, td] + list(names), env=env, timeout=300).returncode == 0
    new = [f for f in set(os.listdir(td)) - before if f.startswith("out.")]
    assert len(new) == 1
    with open(os.path.join(td, new[0])) as f:
        return json.load(f)


# k_lis_hi's tick counters of the first chunk (speck_dec.hip, k_lis_hi: `stamps`): word 0 counts the regions its
# workgroups went through.  (Word 5, beside act == kActTables, counts class tables rebuilt ON the chain: an all-'0'
# list is a zero region that needs none, and a mixed one gets its tables speculatively, off the chain -- measured on
# MI355X it is 2 for checker8 and 3 for tiers8_all whoever decodes the list, so it witnesses nothing here.)
HI_REGIONS = 0


def test_k_lis_l0_and_l2_took_their_lists_from_k_lis_hi(oracle):
    """k_lis_l2 has no counter, and k_lis_l0's (word 48) is compiled out of the product (SPERR_HIP_L0_STAMPS, it costs
    registers the kernel does not have), so both get a differential witness: the work k_lis_hi is left with.  Three
    fresh processes decode containers whose first chunk is checker8 (the list of 8^3 sets: 2048 entries on 23 planes,
    the lists of the smaller sets empty) and checker2 (the list of 2^3 sets: 131 072 entries on 23 planes, the lists
    of the larger sets empty): one with the default settings, one with SPERR_HIP_LIS_L2=0 (the 8^3 sets' list back with
    k_lis_hi), one with SPERR_HIP_LIS_GPUWIDE=0 (every list with k_lis_hi).  All match the oracle's bits, and k_lis_hi
    goes through more regions of the first chunk when it is handed the long list: measured on MI355X, 391 against 414
    for checker8 (one more on each of the 23 planes) and 415 against 944 for checker2.  This is also the first case in
    which SPERR_HIP_LIS_L2 changes the path taken: 64 x 64 x 32 chunks never reach k_lis_l2's 512 entries."""
    names = {"checker8": ("checker8", None, None, None), "checker2": ("checker2", None, None, None)}
    for name in names:   # what the witness rests on: these lists are long, the other two empty, below the top plane
        coef = cc.case(name)[0]
        for e in (8, 4, 2):
            rows = cc.list_reach(coef, e)[1:]
            assert all(L == (0 if str(e) != name[-1] else {8: 2048, 2: 131072}[e]) for _, L, _ in rows), (name, e)
    with tempfile.TemporaryDirectory() as td:
        for name, four in names.items():
            c = grafted(oracle, four)
            np.save(os.path.join(td, name + ".c.npy"), np.frombuffer(c, dtype=np.uint8))
            np.save(os.path.join(td, name + ".r.npy"), oracle_decode(oracle, name, c, True))
        default = child_decode(td, ["checker8", "checker2"], {})
        no_l2 = child_decode(td, ["checker8"], {"SPERR_HIP_LIS_L2": "0"})
        hi_only = child_decode(td, ["checker2"], {"SPERR_HIP_LIS_GPUWIDE": "0"})
    assert default["checker8"]["same"] and default["checker2"]["same"]
    assert no_l2["checker8"]["same"] and hi_only["checker2"]["same"]
    w = HI_REGIONS
    print("k_lis_hi's regions of the first chunk: checker8 %d by default, %d with SPERR_HIP_LIS_L2=0; "
          "checker2 %d by default, %d with SPERR_HIP_LIS_GPUWIDE=0"
          % (default["checker8"]["words"][w], no_l2["checker8"]["words"][w],
             default["checker2"]["words"][w], hi_only["checker2"]["words"][w]))
    assert no_l2["checker8"]["words"][w] > default["checker8"]["words"][w]
    assert hi_only["checker2"]["words"][w] > default["checker2"]["words"][w]
