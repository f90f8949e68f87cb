"""The case table of the 2D coder (plain numpy, no GPU): coefficient patterns aligned to the quadtree forest of a
slice, the 2D twin of tests/coef_cases.py.  The pattern, not a field's statistics, decides what the lists of the 2^2
and 4^2 sets hold, what the type-I set does on every plane, and how long the type-I phase of a plane is.

Band geometry (src/SPECK2D_INT.cpp:149-218): a slice has xf = num_of_xforms(min(dx, dy)) levels; the root band is the
approximation of level xf, and the type-I set releases, from level xf down to 1, the three subbands of a level in the
order BR, TR, BL.  `bands` states that without the coder.

  box cases      checker(e), tiers(e, planes, fill), stagger(e, fill), front(e) of coef_cases in 2D: boxes of edge e in
                 raster order, local index in e^2, the pick of fill "one" taken mod e^2.  On a dyadic slice every box
                 outside the top-left (2e)^2 corner is a coder set whose parent is the 2e box
  type-I cases   the root band is 2^26 | hashed bits unless stated otherwise
    i_dense      every coefficient outside the root is 2^19 | hashed bits: the set is '0' for seven planes, then
                 releases every level on one plane, each subband descending completely inside the type-I phase
    i_stairs     the subbands of level k have top plane 26 - 3 (xf - k + 1): one level released every third plane
    i_br_first   i_stairs, but TR and BL of a level have their top plane one below BR's: they join their lists
                 insignificant and are found there on the next plane, where each descends completely -- a listed set
                 whose split is many regions long
    i_br_only    only the BR subband of each level is nonzero, top plane 4 + 3 k; TR and BL join insignificant
    i_last_only  one coefficient in the slice, in the last corner of BL of level 1, the root band all zero: the set is
                 significant on the first plane and on every level no subband is until the last one, so the remaining
                 set's test is implied each time
    i_root_only  nothing outside the root: the set's test is '0' on every plane
  wide cases     wide_tiers2_all, wide_i_stairs (planes up to 52: the 64-bit pass)
  the extremes   all_one, first_only, last_only, dense_top32 of fields.coefficient_pattern on the slice

`list_reach` is the reach model of coef_cases in 2D; CONDITIONS_2D names the rows the tests rest on and
tests/test_slice_cases_host.py asserts them."""
import functools

import numpy as np

from coef_cases import RATIO, TIERS, WIDE_TIERS, _bit_top, bits_down_to, sign_bits, stream_cuts   # noqa: F401
from fields import _hash_words, coefficient_pattern

SHAPE = (512, 512)        # dyadic, six transform levels, root 8 x 8
RAGGED = (301, 500)       # (rows, columns): the lists mix set shapes, root 5 x 8
FLAT = (9, 2048)          # one transform level, sets that split along one axis only
BIG = (1024, 1024)        # tiers4_one only: the list of 4^2 sets beyond the class ring
MODEL_SHAPES = ((64, 64), (37, 50))
_U = np.uint64
_H_SEED, _HB_SEED, _SIGN_SEED, _ROOT_SEED = 131, 137, 37, 139
ROOT_TOP, DENSE_TOP, WIDE_ROOT_TOP = 26, 19, 52


# ---- band geometry -------------------------------------------------------------------------------------------------

def num_of_xforms(n):
    k = 0
    while n >= 9:
        k += 1
        n -= n // 2
    return min(k, 6)


def approx_detail(n, lev):
    lo, hi = n, 0
    for _ in range(lev):
        hi = lo // 2
        lo -= hi
    return lo, hi


def bands(shape_yx):
    """(xf, root (y0, x0, ly, lx), [(level, name, y0, x0, ly, lx)]): the subbands in the order the type-I set releases
    them, level xf first, BR, TR, BL within a level; empty ones left out"""
    dy, dx = shape_yx
    xf = num_of_xforms(min(dx, dy))
    out = []
    for lev in range(xf, 0, -1):
        ax, ddx = approx_detail(dx, lev)
        ay, ddy = approx_detail(dy, lev)
        for name, y0, x0, ly, lx in (("BR", ay, ax, ddy, ddx), ("TR", 0, ax, ay, ddx), ("BL", ay, 0, ddy, ax)):
            if ly and lx:
                out.append((lev, name, y0, x0, ly, lx))
    return xf, (0, 0, approx_detail(dy, xf)[0], approx_detail(dx, xf)[0]), out


# ---- box cases -----------------------------------------------------------------------------------------------------

def _box_index(shape_yx, e):
    """(box number of every coefficient in raster order of the boxes, local index in its box, boxes per axis)"""
    nb = tuple((s + e - 1) // e for s in shape_yx)
    y, x = np.meshgrid(*[np.arange(s, dtype=np.int64) for s in shape_yx], indexing="ij", sparse=True)
    return (y // e) * nb[1] + (x // e), (y % e) * e + (x % e), nb


def _box_coords(nb):
    return np.meshgrid(*[np.arange(n, dtype=np.int64) for n in nb], indexing="ij")


def _filled(shape_yx, e, top_of_box, fill, hb):
    box, local, _ = _box_index(shape_yx, e)
    h = _hash_words(shape_yx, _H_SEED)
    t = top_of_box.astype(np.uint64)[box]
    coef = (_U(1) << t) | (h & ((_U(1) << t) - _U(1)))
    if fill == "one":
        pick = ((hb >> _U(8)) % _U(e * e)).astype(np.int64)[box]
        coef = np.where(local == pick, coef, _U(0))
    elif fill != "all":
        raise KeyError(fill)
    return coef


def stagger(shape_yx, e, fill, modulus=31):
    _, _, nb = _box_index(shape_yx, e)
    hb = _hash_words((nb[0] * nb[1],), _HB_SEED)
    return _filled(shape_yx, e, hb % _U(modulus), fill, hb)


def tiers(shape_yx, e, planes, fill):
    _, _, nb = _box_index(shape_yx, e)
    hb = _hash_words((nb[0] * nb[1],), _HB_SEED)
    by, bx = _box_coords(nb)
    top = np.asarray(planes, dtype=np.uint64)[(hb % _U(len(planes))).astype(np.int64)]
    top[(((by | bx) & 1) == 0).reshape(-1)] = planes[0]
    return _filled(shape_yx, e, top, fill, hb)


def checker(shape_yx, e):
    box, _, nb = _box_index(shape_yx, e)
    by, bx = _box_coords(nb)
    dense = (((by + bx) & 1) == 1).reshape(-1)
    h = _hash_words(shape_yx, _H_SEED)
    return np.where(dense[box], (h >> _U(40)) | _U(1 << 23), _U(0))


def front(shape_yx, e):
    _, _, nb = _box_index(shape_yx, e)
    n = nb[0] * nb[1]
    top = 27 - (np.arange(n, dtype=np.int64) * 28) // n
    by, bx = _box_coords(nb)
    top[(((by | bx) & 1) == 0).reshape(-1)] = 27
    return _filled(shape_yx, e, top, "all", None)


# ---- type-I cases ----------------------------------------------------------------------------------------------------

def _with_top(h, t):
    return (_U(1) << _U(t)) | (h & ((_U(1) << _U(t)) - _U(1)))


def _root_band(shape_yx, top):
    _, (_, _, ly, lx), _ = bands(shape_yx)
    coef = np.zeros(shape_yx, dtype=np.uint64)
    coef[:ly, :lx] = _with_top(_hash_words((ly, lx), _ROOT_SEED), top)
    return coef


def _band_tops(shape_yx, top_of, root_top=ROOT_TOP):
    """the root band at root_top, subband (level, name) at top_of(level, name) (None: zero), hashed bits below"""
    coef = _root_band(shape_yx, root_top)
    h = _hash_words(shape_yx, _H_SEED)
    for lev, name, y0, x0, ly, lx in bands(shape_yx)[2]:
        t = top_of(lev, name)
        if t is not None:
            coef[y0:y0 + ly, x0:x0 + lx] = _with_top(h[y0:y0 + ly, x0:x0 + lx], t)
    return coef


def i_dense(shape_yx):
    return _band_tops(shape_yx, lambda lev, name: DENSE_TOP)


def i_stairs(shape_yx, root_top=ROOT_TOP):
    xf = bands(shape_yx)[0]
    return _band_tops(shape_yx, lambda lev, name: root_top - 3 * (xf - lev + 1), root_top)


def i_br_first(shape_yx):
    xf = bands(shape_yx)[0]
    return _band_tops(shape_yx, lambda lev, name: ROOT_TOP - 3 * (xf - lev + 1) - (name != "BR"))


def i_br_only(shape_yx):
    return _band_tops(shape_yx, lambda lev, name: 4 + 3 * lev if name == "BR" else None)


def i_last_only(shape_yx):
    lev, name, y0, x0, ly, lx = bands(shape_yx)[2][-1]
    assert (lev, name) == (1, "BL")
    coef = np.zeros(shape_yx, dtype=np.uint64)
    coef[y0 + ly - 1, x0 + lx - 1] = 0x5A5A5A   # top plane 22
    return coef


_BUILDERS = {
    "checker2": lambda s: checker(s, 2),
    "checker4": lambda s: checker(s, 4),
    "tiers2_all": lambda s: tiers(s, 2, TIERS, "all"),
    "tiers4_one": lambda s: tiers(s, 4, TIERS, "one"),
    "stagger4_one": lambda s: stagger(s, 4, "one"),
    "front4": lambda s: front(s, 4),
    "i_dense": i_dense,
    "i_stairs": i_stairs,
    "i_br_only": i_br_only,
    "i_br_first": i_br_first,
    "i_last_only": i_last_only,
    "i_root_only": lambda s: _root_band(s, ROOT_TOP),
    "wide_tiers2_all": lambda s: tiers(s, 2, WIDE_TIERS, "all"),
    "wide_i_stairs": lambda s: i_stairs(s, WIDE_ROOT_TOP),
}
_EXTREMES = ("all_one", "first_only", "last_only", "dense_top32")
I_CASES = ("i_last_only", "i_root_only", "i_br_only", "i_br_first", "i_stairs", "i_dense")
PHASE_CASES = ("i_last_only", "i_br_only", "i_stairs", "i_dense", "wide_i_stairs")   # long_plane releases a level
CASES = ("last_only", "first_only", "all_one", "i_last_only", "i_root_only", "i_br_only", "i_br_first", "i_stairs",
         "checker4",
         "checker2", "tiers4_one", "stagger4_one", "tiers2_all", "front4", "i_dense", "dense_top32",
         "wide_tiers2_all", "wide_i_stairs")   # the whole table, at SHAPE
MX_CASES = I_CASES + ("checker2", "tiers2_all", "stagger4_one")   # at RAGGED and FLAT
ALL_CASES = ([(name, SHAPE) for name in CASES] + [(name, RAGGED) for name in MX_CASES]
             + [(name, FLAT) for name in MX_CASES] + [("tiers4_one", BIG)])
CASE_IDS = ["%s-%dx%d" % ((name,) + shape) for name, shape in ALL_CASES]
MODEL_CASES = [(name, shape) for shape in MODEL_SHAPES for name in I_CASES + ("checker2", "tiers2_all")]
MODEL_IDS = ["%s-%dx%d" % ((name,) + shape) for name, shape in MODEL_CASES]


@functools.lru_cache(maxsize=4)
def case(name, shape_yx=SHAPE):
    """(coef uint64 (y, x), sign uint64 words, wide?) of the named case, read-only"""
    shape_yx = tuple(shape_yx)
    if name in _EXTREMES:
        coef, sign, wide = coefficient_pattern(name, (1,) + shape_yx)
        coef = np.ascontiguousarray(coef.reshape(shape_yx))
    else:
        coef = np.ascontiguousarray(_BUILDERS[name](shape_yx), dtype=np.uint64)
        sign = np.ascontiguousarray(_hash_words(((coef.size + 63) // 64,), _SIGN_SEED))
        wide = name.startswith("wide_")
    coef.setflags(write=False)
    sign.setflags(write=False)
    return coef, sign, wide


# ---- the reach model -------------------------------------------------------------------------------------------------

def box_tops(coef, e):
    """int64 (boxes y, x): the top plane of every box of edge e, -1 for an all-zero box"""
    nb = tuple((s + e - 1) // e for s in coef.shape)
    pad = np.zeros((nb[0] * e, nb[1] * e), dtype=np.uint64)
    pad[:coef.shape[0], :coef.shape[1]] = coef
    return _bit_top(pad.reshape(nb[0], e, nb[1], e).max(axis=(1, 3)))


def list_reach(coef, e):
    """[(p, L, S)] per plane p from the top one down to 0, as coef_cases.list_reach: L the boxes of edge e whose 2e
    parent has its top plane above p while their own is <= p, S those of them whose top plane is p.  The boxes of the
    top-left (2e)^2 corner are left out: there the 2e box is no parent (the root band and the coarsest subbands)."""
    own = box_tops(coef, e)
    nb = own.shape
    even = tuple(n + (n & 1) for n in nb)
    pad = np.full(even, -1, dtype=np.int64)
    pad[:nb[0], :nb[1]] = own
    par = pad.reshape(even[0] // 2, 2, even[1] // 2, 2).max(axis=(1, 3))
    par = np.repeat(np.repeat(par, 2, axis=0), 2, axis=1)[:nb[0], :nb[1]]
    keep = np.ones(nb, dtype=bool)
    keep[:2, :2] = False
    top = int(own.max())
    rows = []
    o, q, k = own.reshape(-1), par.reshape(-1), keep.reshape(-1)
    for p in range(top, -1, -1):
        inl = (o <= p) & (q > p) & k
        rows.append((p, int(inl.sum()), int((inl & (o == p)).sum())))
    return rows


# The conditions the table is built for: (case, shape, box edge of the list, column, planes), the columns as in
# coef_cases.RATIO.  A long list has MORE than the 8192 entries of k_lis_mx's class ring.
RING = 8192
CONDITIONS_2D = (
    ("checker2", SHAPE, 2, "zeros", tuple(range(22, -1, -1))),
    ("tiers2_all", SHAPE, 2, "zeros", tuple(range(25, 14, -1))),
    ("tiers2_all", SHAPE, 2, "half", (14,)),
    ("tiers2_all", SHAPE, 2, "ones", (3,)),
    ("tiers4_one", SHAPE, 2, "zeros", (2, 1, 0)),
    ("stagger4_one", SHAPE, 2, "zeros", (2, 1, 0)),
    ("tiers4_one", BIG, 4, "half", (14,)),
    ("tiers4_one", BIG, 4, "ones", (3,)),
)
# the list of 2^2 sets on entering the case's longest plane at SHAPE, and the peak of the list of 4^2 sets there
LONGEST_2 = {"checker2": 32766, "tiers2_all": 32634, "tiers4_one": 49149, "stagger4_one": 47667}
PEAK_4 = {"checker4": 8190, "tiers4_one": 8144}

# The plane a stream is cut one byte into: the one the conditions name, else the plane the lists are largest on; for
# the type-I cases the release plane whose type-I phase is the longest
LONG_PLANE = {"last_only": 2, "first_only": 31, "all_one": 0, "checker4": 11, "checker2": 11, "tiers4_one": 14,
              "stagger4_one": 9, "tiers2_all": 14, "front4": 13, "dense_top32": 31, "i_dense": DENSE_TOP,
              "i_stairs": 8, "i_br_only": 7, "i_br_first": 7, "i_last_only": 22, "i_root_only": 20, "wide_tiers2_all": 40,
              "wide_i_stairs": 34}


def long_plane(name, shape_yx):
    """LONG_PLANE at SHAPE; the stairs end higher where a slice has fewer levels than SHAPE's six"""
    xf = bands(shape_yx)[0]
    if name == "i_stairs":
        return ROOT_TOP - 3 * xf
    if name == "i_br_first":   # the plane that finds TR and BL of level 1 on their lists
        return ROOT_TOP - 3 * xf - 1
    if name == "wide_i_stairs":
        return WIDE_ROOT_TOP - 3 * xf
    return LONG_PLANE[name]


# ---- what a pattern does to the type-I set ---------------------------------------------------------------------------

def band_tops(coef):
    """[top plane of every subband of bands(coef.shape), -1 for an all-zero one]"""
    return [int(_bit_top(coef[y0:y0 + ly, x0:x0 + lx].max().reshape(1))[0])
            for _, _, y0, x0, ly, lx in bands(coef.shape)[2]]


def release_planes(coef):
    """{level: the plane on which the type-I set releases it}, read off the band tops: the set that holds the levels
    1 .. k is significant from the highest top plane among them on.  A level that is never released is left out."""
    xf, _, bl = bands(coef.shape)
    tops = band_tops(coef)
    of_level = {lev: max(t for (l, *_), t in zip(bl, tops) if l == lev) for lev in range(1, xf + 1)}
    out, m = {}, -1
    for lev in range(1, xf + 1):
        m = max(m, of_level[lev])
        if m >= 0:
            out[lev] = m
    return out


def plane_start(encode, coef, sign, plane):
    """the bit at which plane `plane` starts in the stream of (coef, sign), as cut_into_plane finds it; the whole
    stream's bit count for plane -1"""
    head = encode(bits_down_to(coef, plane) if plane >= 0 else coef, sign)
    return int(np.frombuffer(head, dtype=np.uint64, count=1, offset=1)[0])


def cut_into_plane(encode, coef, sign, plane):
    """the length of the stream of (coef, sign) cut one byte into plane `plane`; encode(coef, sign) -> stream"""
    return 9 + plane_start(encode, coef, sign, plane) // 8 + 1


def i_phase(encode, coef, sign, plane):
    """(first bit, end bit) of the type-I phase of plane `plane`, a plane on which the set releases a level, from
    oracle streams of shifted coefficients and never from the code under test.

    end: the plane's refinement pass follows the phase, one bit per coefficient found on the planes above, and the
    next plane follows that.  start: with everything the set holds on entering the plane zeroed, the planes above and
    this plane's passes over the pixels and the listed sets stay bit for bit what they were, the set then says '0'
    in one bit, and the same refinement pass ends the stream.  With nothing above the plane and nothing outside the
    set (i_last_only) that stream is empty and the phase starts behind the one '0' of the root band's test."""
    xf, root, bl = bands(coef.shape)
    rel = release_planes(coef)
    held = [lev for lev, p in rel.items() if p <= plane] + [lev for lev in range(1, xf + 1) if lev not in rel]
    assert held and any(rel.get(lev) == plane for lev in held), "the set releases nothing on this plane"
    refine = int(np.count_nonzero(coef >> _U(plane + 1)))
    end = plane_start(encode, coef, sign, plane - 1) - refine
    cleared = np.array(coef)
    for lev, _, y0, x0, ly, lx in bl:
        if lev in held:
            cleared[y0:y0 + ly, x0:x0 + lx] = 0
    if not (cleared >> _U(plane)).any():
        assert root[2] * root[3] > 1
        return 1, end
    tail = encode(np.ascontiguousarray(cleared >> _U(plane)), sign)
    return int(np.frombuffer(tail, dtype=np.uint64, count=1, offset=1)[0]) - 1 - refine, end


def cut_into_i_phase(encode, coef, sign, plane):
    """(the stream length that ends in the middle of the type-I phase of `plane`, that middle as a bit budget)"""
    a, b = i_phase(encode, coef, sign, plane)
    mid = (a + b) // 2
    return 9 + mid // 8, mid


def implied_tests(shape_yx):
    """(the type-I phase's bit count, the tests of the remaining set that are implied) of i_last_only, from the band
    list: the set's '1', a coded '0' or '1' per subband, nothing for the remaining set after each level but the last
    (no subband of the level was significant), then the descent into the last corner of BL of level 1 -- at every
    split the first non-empty child holds the corner, says '1', and the others say '0' -- and the sign."""
    xf, _, bl = bands(shape_yx)
    bits = 1 + len(bl)
    _, _, _, _, ly, lx = bl[-1]
    while ly * lx > 1:
        dly, dlx = ly // 2, lx // 2
        kids = [k for k in ((dly, dlx), (dly, lx - dlx), (ly - dly, dlx), (ly - dly, lx - dlx)) if k[0] and k[1]]
        bits += len(kids)
        ly, lx = kids[0]
    return bits + 1, xf - 1


# ---- grafting a stream behind a conditioner header -------------------------------------------------------------------

def graft_body(header17, speck_stream):
    """a 2D stream body: the 17-byte conditioner header (src/SPECK_FLT.cpp:88-103) followed by the SPECK stream"""
    assert len(header17) == 17 and not header17[0] & 0x01, "a constant slice has no SPECK stream"
    return bytes(header17) + bytes(speck_stream)


def smooth_slice(shape_yx, dtype=np.float32):
    from fields import smooth_field
    return np.ascontiguousarray(smooth_field((1,) + tuple(shape_yx), dtype=dtype)[0])


def header_of(oracle, shape_yx):
    """the conditioner header of a smooth slice of this shape in rate mode: q and the mean are real"""
    return oracle.comp_2d(smooth_slice(shape_yx), 1, 2.0)[:17]
