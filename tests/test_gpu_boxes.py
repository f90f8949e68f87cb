"""GPU: a box per entry out of a batch of containers in one call (sperrhip_decompress_boxes_dev, sperrhip_boxes_plan,
SperrHip.decompress_boxes / boxes_plan).

The expected values are always the oracle's decode -- oracle.decomp_3d, oracle.decomp_3d_multi_res, both also of
oracle.trunc_3d's container -- cut to the boxes with numpy; the library's own single-box call is asserted equal beside
that where a case says so, never instead.  All compares are on the bit patterns, float and double output.  Beside
parity the tests pin which form ran (k_boxes_copy's launches in the profile), that nothing beside the result is
written, every refusal, and that the entries of a call share their launches.

Two refusals of the call cannot be reached with containers that exist on a test's scale -- a staging array taller than
INT32_MAX and more than 2^32 - 1 (entry, chunk) pairs both need millions of distinct chunks -- and are checked where the
rule is stated, in tests/cpp/boxes_check.cpp (tests/test_boxes_host.py)."""
import ctypes as C

import numpy as np
import pytest

from sperr_amd import api
from sperr_amd.synth import turbulence

pytestmark = pytest.mark.gpu
_sz = C.c_size_t
SENTINEL = 0x7FC0BEEF   # a NaN pattern no decode produces


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


def make(eng, v, ch, q, mode=1):
    return bytes(eng.compress(cuda(v), ch, q, mode=mode).cpu().numpy())


def xyz(v):
    return (v.shape[2], v.shape[1], v.shape[0])


def copies(eng):
    """launches of k_boxes_copy since eng.profile(True)"""
    return sum(n for name, (_, n) in eng.profile_report().items() if "k_boxes_copy" in name)


def launches(eng):
    return sum(n for _, n in eng.profile_report().values())


class Decoded:
    """the oracle's decode of every container of a case, once: full[of][c] and, where asked for, levels[c][h]"""

    def __init__(self, oracle, containers, levels=False):
        self.containers = containers
        self.devs = [dev_of(c) for c in containers]
        self.full = {of: [oracle.decomp_3d(c, of) for c in containers] for of in (True, False)}
        self.levels = [oracle.decomp_3d_multi_res(c)[1] for c in containers] if levels else None

    def want(self, of, which, los, dims, level=None):
        out = []
        for e, c in enumerate(which):
            src = self.full[of][c] if level is None else self.levels[c][level]
            if level is not None and of:
                src = src.astype(np.float32)
            out.append(crop(src, los[e], dims))
        return np.stack(out)


def check(eng, dec, los, dims, which=None, level=None, pct=0, of=True, staged=None, single=True, vec=None):
    """one call against the oracle's boxes; staged: the form the call has to take (None: not looked at); vec: whether
    its copy has to be the 16-byte form"""
    n = len(dec.devs)
    wh = list(range(n)) if which is None else list(which)
    if np.ndim(los) == 1:
        los = [tuple(los)] * len(wh)
    if staged is not None:
        eng.profile(True)
    got = eng.decompress_boxes(dec.devs, los if which is not None or len(set(los)) > 1 else los[0], dims, which=which,
                               level=level, pct=pct, output_float=of)
    if staged is not None:
        ran = copies(eng)
        forms = [name for name in eng.profile_report() if "k_boxes_copy" in name]
        eng.profile(False)
        assert ran == (1 if staged else 0), f"k_boxes_copy ran {ran} times"
        if vec is not None:   # the 16-byte form is the launch whose template argument is `true`
            assert len(forms) == 1 and ("true" in forms[0]) == vec, (forms, vec, los, dims)
    got = got.cpu().numpy()
    want = dec.want(of, wh, los, dims, level)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(bits(got), bits(want)), (los, dims, which, level, pct, of)
    if single:   # beside the oracle: entry 0 is the library's own single-box call
        if level is None:
            one = eng.decompress_box(dec.devs[wh[0]], los[0], dims, output_float=of, pct=pct)
        else:
            one = eng.decompress_level(dec.devs[wh[0]], level, los[0], dims, output_float=of, pct=pct)
        assert np.array_equal(bits(one.cpu().numpy()), bits(got[0]))
    return got


# ---- a region of interest over a time series: the direct form ---------------------------------------------------
SERIES_SHAPE, SERIES_CH = (40, 48, 56), (32, 32, 32)   # (z, y, x): chunks of (32, 48, 40) and (24, 48, 40) in x, y, z --
SERIES_BOXES = [((0, 0, 0), (56, 48, 40)),             #   two shape groups, y and z remainders merged; the whole volume
                ((55, 47, 39), (1, 1, 1)),             # one voxel at a corner
                ((29, 30, 31), (11, 9, 9)),            # an odd x origin across every chunk border there is (x = 32) and
                                                       #   across where y and z would have one (32)
                ((33, 33, 1), (20, 13, 37))]           # inside the last, merged chunk


@pytest.fixture(scope="module")
def series(eng, oracle):
    vols = [turbulence(SERIES_SHAPE, seed=s) for s in (42, 43, 44, 45)] + [np.full(SERIES_SHAPE, 2.75, dtype=np.float32)]
    made = {}

    def get(mode, q):
        if mode not in made:
            made[mode] = Decoded(oracle, [make(eng, v, SERIES_CH, q, mode=mode) for v in vols])
        return made[mode]
    return get


@pytest.mark.parametrize("of", [True, False], ids=["fp32", "fp64"])
@pytest.mark.parametrize("mode,q", [(1, 2.0), (2, 80.0), (3, 1e-3)])
def test_boxes_time_series_direct(eng, series, mode, q, of):
    dec = series(mode, q)
    assert len(dec.devs) == 5
    for lo, dims in SERIES_BOXES:
        check(eng, dec, lo, dims, of=of, staged=False, single=(lo != (0, 0, 0)))
    plan = eng.boxes_plan(SERIES_SHAPE, [SERIES_CH] * 5, (29, 30, 31), (11, 9, 9))
    assert plan["slots"] == plan["pairs"] == 5 * 2 and not plan["staged"] and plan["staging_values"] == 0


# ---- random crops that share chunks: the staged form -------------------------------------------------------------
@pytest.fixture(scope="module")
def cubes(eng, oracle):
    """three containers of 64^3 in 32^3 chunks, the third in point-wise-error mode; with their levels"""
    vols = [turbulence((64, 64, 64), seed=s) for s in (7, 8, 9)]
    return Decoded(oracle, [make(eng, vols[0], (32, 32, 32), 2.0), make(eng, vols[1], (32, 32, 32), 3.0),
                            make(eng, vols[2], (32, 32, 32), 1e-3, mode=3)], levels=True)


def crop_entries():
    rng = np.random.default_rng(20261020)
    dims = (24, 20, 17)
    which = [0, 1, 2, 0, 1, 2, 0, 0, 1, 2, 1, 0]
    los = [tuple(int(rng.integers(0, 64 - dims[a] + 1)) for a in range(3)) for _ in which]
    los[7] = los[3]   # entries 3 and 7 are the same box of the same container
    return which, los, dims


@pytest.mark.parametrize("of", [True, False], ids=["fp32", "fp64"])
def test_boxes_crops_share_chunks_staged(eng, cubes, of):
    which, los, dims = crop_entries()
    assert len(which) == 12 and which[3] == which[7] and los[3] == los[7]
    plan = eng.boxes_plan((64, 64, 64), [(32, 32, 32)] * 3, los, dims, which=which)
    assert plan["staged"] and plan["slots"] < plan["pairs"] and plan["slots"] <= 24
    assert plan["output_values"] == 12 * 24 * 20 * 17 and plan["staging_values"] == 32 * 32 * 32 * plan["slots"]
    got = check(eng, cubes, los, dims, which=which, of=of, staged=True)
    assert np.array_equal(bits(got[3]), bits(got[7]))


# ---- the copy kernel's edges, through the staged form ------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(eng, oracle):
    return Decoded(oracle, [make(eng, turbulence((16, 16, 64), seed=3), (32, 16, 16), 4.0)])


@pytest.mark.parametrize("of", [True, False], ids=["fp32", "fp64"])
def test_boxes_copy_kernel_row_edges(eng, wide, of):
    """widths and x origins around the 16-byte pack (4 floats, 2 doubles) and across the border at x = 32; the two
    entries overlap, so every call stages and both forms of the kernel run (aligned cases: the pack form)"""
    for w in (1, 3, 4, 5, 31, 32, 33):
        for x0 in (0, 1, 2, 3):
            if x0 + w > 64:
                continue
            los = [(x0, 0, 0), (x0, 1, 2)]
            # every window starts at x0 or at the border (32) and is as wide as the box or cut there: whole packs on
            # both sides exactly when x0 and the width are
            pack = 4 if of else 2
            check(eng, wide, los, (w, 8, 8), which=[0, 0], of=of, staged=True, single=False,
                  vec=(w % pack == 0 and x0 % pack == 0))
    # a second x origin in the same call: windows that start at different alignments side by side
    check(eng, wide, [(0, 0, 0), (28, 0, 0), (5, 3, 3)], (32, 8, 8), which=[0, 0, 0], of=of, staged=True, single=False,
          vec=False)
    check(eng, wide, [(0, 0, 0), (28, 0, 0), (4, 3, 3)], (32, 8, 8), which=[0, 0, 0], of=of, staged=True, single=False,
          vec=True)


# ---- every writer of the decoder's last pass, direct and staged --------------------------------------------------
def tiny_volume(seed):
    shape = (4, 6, 9)
    return (np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) * (0.37 + 0.01 * seed) + 0.1) ** 2


WRITERS = {
    "long_rows": (lambda s: turbulence((10, 37, 300), seed=s), (300, 37, 10), 4.0, 1),
    "merged_remainder": (lambda s: turbulence((70, 40, 300), seed=s), (256, 32, 32), 2.0, 1),
    "untransformed_chunks": (tiny_volume, (3, 2, 2), 1e-3, 3),
    "pwe_correctors": (lambda s: turbulence((48, 32, 48), seed=s), (16, 16, 24), 1e-3, 3),
}


@pytest.mark.parametrize("name", list(WRITERS))
def test_boxes_every_last_pass_writer(eng, oracle, name):
    gen, ch, q, mode = WRITERS[name]
    vols = [gen(1), gen(2)]
    dec = Decoded(oracle, [make(eng, v, ch, q, mode=mode) for v in vols])
    vol = xyz(vols[0])
    # an odd-x box across the first chunk border of every axis that has one, else most of the axis
    lo, dims = [], []
    for a in range(3):
        if ch[a] < vol[a]:
            l = ch[a] - 3 if ch[a] > 3 else ch[a] - 1
            if a == 0 and l % 2 == 0:
                l = max(l - 1, 0)
            d = min(vol[a] - l - 1, 9)
        else:
            l, d = min(1, vol[a] - 1), max(1, vol[a] - 2)
        lo.append(l)
        dims.append(d)
    lo, dims = tuple(lo), tuple(dims)
    moved = tuple(lo[a] + (1 if lo[a] + dims[a] < vol[a] else 0) for a in range(3))
    for of in (True, False):
        check(eng, dec, (0, 0, 0), vol, of=of, staged=False, single=False)              # direct, whole volumes
        check(eng, dec, lo, dims, of=of, staged=False)                                   # direct, a box
        check(eng, dec, [lo, moved, lo], dims, which=[0, 0, 1], of=of, staged=True)      # staged: 0 and 1 overlap
        check(eng, dec, [(0, 0, 0)] * 3, vol, which=[1, 0, 1], of=of, staged=True, single=False)


# ---- levels of the hierarchy ----------------------------------------------------------------------------------
def test_boxes_levels_whole_and_boxes(eng, cubes):
    nlev = len(cubes.levels[0])
    assert nlev >= 2 and all(len(lv) == nlev for lv in cubes.levels)
    for h in range(nlev):
        side = cubes.levels[0][h].shape[0]   # the level is a cube of `side`: 2 x 2 x 2 corners of side / 2
        cr = side // 2
        for of in (True, False):
            check(eng, cubes, (0, 0, 0), (side,) * 3, level=h, of=of, staged=False)      # every container's whole level
            check(eng, cubes, [(0, 0, 0)] * 2, (side,) * 3, which=[2, 2], level=h, of=of, staged=True, single=False)
            if cr < 2:
                check(eng, cubes, [(1, 0, 1), (0, 1, 0), (1, 1, 1)], (1, 1, 1), level=h, of=of, staged=False)
                continue
            d = (cr, cr - 1, cr + 1)
            check(eng, cubes, (1, cr // 2, cr - 1), d, level=h, of=of, staged=False)     # across the corner borders
            check(eng, cubes, [(1, cr // 2, cr - 1), (0, 0, 0), (1, 1, 0), (cr, 1, cr - 1)], d, which=[0, 2, 2, 0],
                  level=h, of=of, staged=True)
            check(eng, cubes, [(0, 0, 0), (cr, cr, cr)], (cr, cr, cr), which=[1, 1], level=h, of=of, staged=False)


# ---- portions ---------------------------------------------------------------------------------------------------
def test_boxes_portion_at_full_resolution_and_at_a_level(eng, oracle, cubes):
    cut = Decoded(oracle, [oracle.trunc_3d(c, 30) for c in cubes.containers], levels=True)
    cut.devs = cubes.devs   # the call reads the whole containers' first 30 percent
    nlev = len(cut.levels[0])
    for of in (True, False):
        check(eng, cut, (3, 30, 9), (40, 5, 30), pct=30, of=of, staged=False)
        check(eng, cut, [(3, 30, 9), (5, 31, 10), (0, 0, 0)], (40, 5, 30), which=[1, 1, 2], pct=30, of=of, staged=True)
        h = nlev - 1
        side = cut.levels[0][h].shape[0]
        check(eng, cut, (1, 2, 3), (side - 2, side - 3, side - 4), level=h, pct=30, of=of, staged=False)
        check(eng, cut, [(1, 2, 3), (0, 0, 0)], (side - 2, side - 3, side - 4), which=[0, 0], level=h, pct=30, of=of,
              staged=True)
    # the portion differs from the whole decode, so the compare above was of the portion
    whole = eng.decompress_boxes(cubes.devs, (3, 30, 9), (40, 5, 30)).cpu().numpy()
    part = eng.decompress_boxes(cubes.devs, (3, 30, 9), (40, 5, 30), pct=30).cpu().numpy()
    assert not np.array_equal(bits(whole), bits(part))


# ---- containers that differ ----------------------------------------------------------------------------------------
def test_boxes_containers_that_differ_in_chunks_mode_and_precision(eng, oracle):
    v32 = turbulence(SERIES_SHAPE, seed=11)
    v64 = turbulence(SERIES_SHAPE, seed=12, dtype=np.float64)
    dec = Decoded(oracle, [make(eng, v32, (32, 32, 32), 2.0), make(eng, v64, (16, 16, 16), 90.0, mode=2),
                           make(eng, v32, (56, 48, 40), 1e-3, mode=3), make(eng, v64, (20, 48, 13), 3.0)])
    for of in (True, False):
        check(eng, dec, (29, 30, 11), (20, 17, 25), of=of, staged=False)
        check(eng, dec, (0, 0, 0), (56, 48, 40), of=of, staged=False, single=False)
        check(eng, dec, [(29, 30, 11), (1, 2, 3), (30, 30, 12), (2, 2, 2), (9, 9, 9), (10, 10, 10)], (20, 17, 25),
              which=[0, 1, 0, 2, 3, 3], of=of, staged=True)


# ---- nothing beside the result is written ----------------------------------------------------------------------------
@pytest.mark.parametrize("of", [True, False], ids=["fp32", "fp64"])
def test_boxes_write_the_result_and_nothing_else(eng, cubes, of):
    import torch
    which, los, dims = crop_entries()
    n = 12 * dims[0] * dims[1] * dims[2]
    for wh, lo in ((which, los), (None, [los[0]] * 3)):   # staged, then direct
        nbox = len(lo)
        room = torch.full((nbox * dims[0] * dims[1] * dims[2] + 4099,), float("nan"),
                          dtype=torch.float32 if of else torch.float64, device="cuda")
        pat = SENTINEL if of else (SENTINEL << 32 | 0xBEEF)
        room.view(torch.int32 if of else torch.int64).fill_(pat)
        used = nbox * dims[0] * dims[1] * dims[2]
        assert used <= n
        out = room[:used].view(nbox, dims[2], dims[1], dims[0])
        back = eng.decompress_boxes(cubes.devs, lo if wh is not None else lo[0], dims, which=wh, output_float=of, out=out)
        assert back.data_ptr() == room.data_ptr()
        host = bits(room.cpu().numpy())
        assert not (host[:used] == pat).any(), "a value of the result was left unwritten"
        assert (host[used:] == pat).all(), "something behind the result was written"
        want = cubes.want(of, wh if wh is not None else [0, 1, 2], lo, dims)
        assert np.array_equal(host[:used], bits(want).ravel())


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_boxes_refusals_leave_the_output_alone(eng, oracle, cubes):
    import torch
    lib = eng.lib
    devs = list(cubes.devs)
    other = dev_of(make(eng, turbulence(SERIES_SHAPE), (32, 32, 32), 2.0))          # another volume
    chunks16 = dev_of(make(eng, turbulence((64, 64, 64), seed=5), (16, 16, 16), 2.0))  # the same volume, other chunks
    nolevel = dev_of(make(eng, turbulence((64, 64, 64), seed=5), (64, 64, 24), 2.0))   # chunks that do not tile it
    damaged = dev_of(cubes.containers[0][:-1])
    with pytest.raises(api.SperrHipError):
        eng.decompress(damaged, True)
    sentinel = torch.full((3 * 8 * 8 * 8 + 64,), 7.0, dtype=torch.float32, device="cuda")
    cap = 3 * 8 * 8 * 8 * 4

    def call(conts, which, los, dims, level=None, pct=0, cap=cap, nbox=None, ncont=None, ptrs=None, lo_null=False,
             dims_null=False, lens_null=False):
        n = len(conts) if ncont is None else ncont
        nb = (len(which) if which is not None else n) if nbox is None else nbox
        p = ptrs if ptrs is not None else (C.c_void_p * max(len(conts), 1))(*[c.data_ptr() for c in conts])
        ln = None if lens_null else (_sz * max(len(conts), 1))(*[c.numel() for c in conts])
        lo = None if lo_null else (_sz * (3 * max(len(los), 1)))(*[v for o in los for v in o])
        wh = None if which is None else (C.c_uint32 * max(len(which), 1))(*which)
        rc = lib.sperrhip_decompress_boxes_dev(p, ln, n, wh, lo, nb, None if dims_null else (_sz * 3)(*dims),
                                               None if level is None else C.byref(_sz(level)), pct, 1,
                                               sentinel.data_ptr(), cap, None)
        torch.cuda.synchronize()
        if rc == 0:   # (a call that is fine, to show that its refused neighbour fails for the one thing it changes)
            sentinel.fill_(7.0)
        assert bool((sentinel == 7.0).all()), "a refused call wrote to its output"
        return rc

    b, o3 = (8, 8, 8), [(0, 0, 0)] * 3
    assert call(devs, None, o3, b) == 0
    assert call(devs, [0, 1], o3[:2], b, nbox=0) == -1                            # nbox of 0
    assert call(devs, None, o3, b, ncont=0, nbox=3) == -1                         # ncont of 0
    assert call([], None, [], b) == -1
    assert call(devs, None, o3, b, ptrs=C.cast(None, C.POINTER(C.c_void_p))) == -1   # NULL pointers
    assert call(devs, None, o3, b, ptrs=(C.c_void_p * 3)(devs[0].data_ptr(), None, devs[2].data_ptr())) == -1
    assert call(devs, None, o3, b, lens_null=True) == -1
    assert call(devs, None, o3, b, lo_null=True) == -1
    assert call(devs, None, o3, b, dims_null=True) == -1
    assert lib.sperrhip_decompress_boxes_dev((C.c_void_p * 1)(devs[0].data_ptr()), (_sz * 1)(devs[0].numel()), 1, None,
                                             (_sz * 3)(0, 0, 0), 1, (_sz * 3)(*b), None, 0, 1, None, cap, None) == -1
    assert call(devs, [0, 3, 1], o3, b) == -1                                     # a `which` index out of range
    assert call(devs, None, o3[:2], b, nbox=2) == -1                              # which NULL and nbox != ncont
    assert call(devs, None, o3, (8, 0, 8)) == -1                                  # an extent of 0
    assert call(devs, None, [(0, 0, 0), (57, 0, 0), (0, 0, 0)], b) == -1          # entry 1 leaves its volume
    assert call(devs, [0, 0, 0], [(0, 0, 0), (0, 0, 0), (0, 64, 0)], b) == -1
    assert call(devs, None, o3, (8, 8, 65)) == -1
    nlev = len(cubes.levels[0])
    side = cubes.levels[0][0].shape[0]
    assert call(devs, None, [(side - 1, 0, side - 1)] * 3, (1, 1, 1), level=0) == 0
    assert call(devs, None, o3, (side + 1, 1, 1), level=0) == -1                  # ... its level
    assert call(devs, None, [(0, 0, 0), (0, side, 0), (0, 0, 0)], (1, 1, 1), level=0) == -1
    assert call([devs[0], other, devs[1]], None, o3, b) == -1                     # volume dims differ
    assert call([devs[0], chunks16, devs[1]], None, o3, b) == 0                   # (chunk dims may, at full resolution)
    assert call([devs[0], chunks16, devs[1]], None, o3, (1, 1, 1), level=0) == -1    # with a level they may not
    assert call(devs, None, o3, (1, 1, 1), level=nlev) == -1                      # no such level
    assert call([nolevel], None, o3[:1], (1, 1, 1), level=0) == -1
    assert call([nolevel], None, o3[:1], b) == 0
    # nbox * bz beyond INT32_MAX: 2^25 + 1 entries of 64 slices (arrays of zeros nobody gets to read)
    many = (1 << 25) + 1
    wh = np.zeros(many, dtype=np.uint32)
    lo = np.zeros(3 * many, dtype=np.uint64)
    rc = lib.sperrhip_decompress_boxes_dev((C.c_void_p * 1)(devs[0].data_ptr()), (_sz * 1)(devs[0].numel()), 1,
                                           wh.ctypes.data_as(C.POINTER(C.c_uint32)), lo.ctypes.data_as(C.POINTER(_sz)),
                                           many, (_sz * 3)(1, 1, 64), None, 0, 1, sentinel.data_ptr(), cap, None)
    assert rc == -1
    assert call(devs, None, o3, b, cap=cap - 4) == -1                             # an output that is too small
    assert call(devs, None, o3, b, cap=0) == -1
    assert call([devs[0], damaged, devs[1]], None, o3, b) == -1                   # a container decompress refuses
    assert call([devs[0], dev_of(b"\x07" + cubes.containers[1][1:]), devs[1]], None, o3, b) == -1
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())
    # the Python layer raises, and the engine still works
    with pytest.raises(api.SperrHipError):
        eng.decompress_boxes(devs, (60, 0, 0), b)
    with pytest.raises(api.SperrHipError):
        eng.boxes_plan((64, 64, 64), [(32, 32, 32)] * 3, (60, 0, 0), b)
    check(eng, cubes, (5, 6, 7), (40, 30, 20), staged=False)


# ---- the entries of a call share their launches ------------------------------------------------------------------
def test_boxes_sixteen_containers_share_their_launches(eng, oracle):
    """Sixteen containers of one 32^3 chunk each, one entry each.  pick_sub_batches cuts fewer than 56 chunks of a
    shape into at most four sub-batches, each with one chain of per-plane launches, where sixteen single calls run
    sixteen chains: a quarter of the launches is expected, under half is asserted.  A condition on counts, no timing."""
    dec = Decoded(oracle, [make(eng, turbulence((32, 32, 32), seed=100 + s), (32, 32, 32), 2.0) for s in range(16)])
    lo, dims = (1, 2, 3), (30, 29, 28)
    eng.profile(True)
    got = eng.decompress_boxes(dec.devs, lo, dims)
    one_call = launches(eng)
    singles = 0
    outs = []
    for d in dec.devs:
        eng.profile(True)
        outs.append(eng.decompress_box(d, lo, dims))
        singles += launches(eng)
    eng.profile(False)
    assert 0 < one_call and one_call * 2 < singles, (one_call, singles)
    want = dec.want(True, list(range(16)), [lo] * 16, dims)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    for e in range(16):
        assert np.array_equal(bits(outs[e].cpu().numpy()), bits(want[e]))
