"""The shared case table of the SPECK list kernels (plain numpy, no GPU): coefficient patterns aligned to the set tree
of a 128^3 chunk, where the lists of the 2^3, 4^3 and 8^3 sets (k_lis_l0 / _l1 / _l2) run to thousands of entries
and the pattern, not a field's statistics, decides what their tokens are.

A box has edge e in array index space and a number in raster order (z slowest); on a dyadic chunk the boxes are the
coder's sets (src/SPECK3D_INT.cpp:99-212 halves every axis).  `h` is a hash word per coefficient, `hb` one per box
(tests/fields.py: _hash_words), so the patterns are the same on every machine (tests/golden/ref_digests.json depends
on that).  Every pattern returns what fields.coefficient_pattern does: (coef uint64 (z, y, x), sign words, wide?).

  stagger(e, fill)        box b has top plane t_b = hb % 31 (% 53: wide).  fill "one": one coefficient of the box, at
                          local index (hb >> 8) % e^3, is 2^t_b | hashed lower bits, the rest zero; fill "all": every
                          coefficient of the box is 2^t_b | (h & (2^t_b - 1))
  tiers(e, planes, fill)  the first child of every 2e box (three even box coordinates) takes planes[0], every other
                          box planes[hb % len(planes)]: all boxes enter the list on planes[0] and leave it tier by tier
  checker(e)              boxes of odd coordinate parity are dense, (h >> 40) | 1 << 23, the others zero
  front(e)                a box's top plane falls linearly with its raster index, from 27 to 0; every coefficient of
                          the box has that bit and hashed lower bits.  The first child of every 2e box takes plane 27,
                          as in tiers: without it neighbouring boxes share a top plane, their parents split on the
                          plane the boxes do, and the list never holds a thousand entries (914 at most for e = 4).
                          With it every box is listed from plane 27 on and the boxes a plane finds significant are
                          one run of raster indices, which moves through the list as the planes go down
  the extremes            all_one, dense_top32, last_only, first_only of fields.coefficient_pattern

`list_reach` is the model of what a pattern does to a list: a property of the input, computed without the coder.
CONDITIONS names the (case, list, plane) rows the tests rest on; tests/test_coef_cases_host.py asserts them."""
import functools

import numpy as np

from fields import _hash_words, coefficient_pattern
from sperr_amd.farm import build_container, split_container

SHAPE = (128, 128, 128)
MX_SHAPE = (100, 128, 128)   # not dyadic along z: the lists mix set shapes, k_lis_mx decodes them
MX_CUBE = (100, 100, 100)    # no axis dyadic: the sets change shape along all three
TIERS = (26, 14, 3)
WIDE_TIERS = (52, 40, 33)
_U = np.uint64
_H_SEED, _HB_SEED, _SIGN_SEED = 131, 137, 37


def _box_index(shape_zyx, e):
    """(box number of every coefficient in raster order of the boxes, local index in its box, boxes per axis)"""
    nb = tuple((s + e - 1) // e for s in shape_zyx)
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.int64) for s in shape_zyx], indexing="ij", sparse=True)
    box = ((z // e) * nb[1] + (y // e)) * nb[2] + (x // e)
    local = ((z % e) * e + (y % e)) * e + (x % e)
    return box, local, nb


def _box_coords(nb):
    return np.meshgrid(*[np.arange(n, dtype=np.int64) for n in nb], indexing="ij")


def _filled(shape_zyx, e, top_of_box, fill, hb):
    """coef: box b has top plane top_of_box[b], filled as `fill` says"""
    box, local, _ = _box_index(shape_zyx, e)
    h = _hash_words(shape_zyx, _H_SEED)
    t = top_of_box.astype(np.uint64)[box]
    coef = (_U(1) << t) | (h & ((_U(1) << t) - _U(1)))
    if fill == "one":
        pick = ((hb >> _U(8)) % _U(e ** 3)).astype(np.int64)[box]
        coef = np.where(local == pick, coef, _U(0))
    elif fill != "all":
        raise KeyError(fill)
    return coef


def stagger(shape_zyx, e, fill, modulus=31):
    _, _, nb = _box_index(shape_zyx, e)
    hb = _hash_words((int(np.prod(nb)),), _HB_SEED)
    return _filled(shape_zyx, e, hb % _U(modulus), fill, hb)


def tiers(shape_zyx, e, planes, fill):
    _, _, nb = _box_index(shape_zyx, e)
    hb = _hash_words((int(np.prod(nb)),), _HB_SEED)
    bz, by, bx = _box_coords(nb)
    first = (((bz | by | bx) & 1) == 0).reshape(-1)
    top = np.asarray(planes, dtype=np.uint64)[(hb % _U(len(planes))).astype(np.int64)]
    top[first] = planes[0]
    return _filled(shape_zyx, e, top, fill, hb)


def checker(shape_zyx, e):
    box, _, nb = _box_index(shape_zyx, e)
    bz, by, bx = _box_coords(nb)
    dense = (((bz + by + bx) & 1) == 1).reshape(-1)
    h = _hash_words(shape_zyx, _H_SEED)
    return np.where(dense[box], (h >> _U(40)) | _U(1 << 23), _U(0))


def front(shape_zyx, e):
    _, _, nb = _box_index(shape_zyx, e)
    n = int(np.prod(nb))
    top = 27 - (np.arange(n, dtype=np.int64) * 28) // n
    bz, by, bx = _box_coords(nb)
    top[(((bz | by | bx) & 1) == 0).reshape(-1)] = 27
    return _filled(shape_zyx, e, top, "all", None)


_BUILDERS = {
    "checker8": lambda s: checker(s, 8),
    "stagger8_one": lambda s: stagger(s, 8, "one"),
    "tiers8_all": lambda s: tiers(s, 8, TIERS, "all"),
    "tiers4_one": lambda s: tiers(s, 4, TIERS, "one"),
    "checker2": lambda s: checker(s, 2),
    "tiers2_all": lambda s: tiers(s, 2, TIERS, "all"),
    "front4": lambda s: front(s, 4),
    "wide_tiers8_all": lambda s: tiers(s, 8, WIDE_TIERS, "all"),
    "wide_stagger4_one": lambda s: stagger(s, 4, "one", modulus=53),
}
_EXTREMES = ("all_one", "dense_top32", "last_only", "first_only")
CASES = ("last_only", "first_only", "all_one", "checker8", "stagger8_one", "tiers8_all", "tiers4_one", "checker2",
         "tiers2_all", "front4", "dense_top32", "wide_tiers8_all", "wide_stagger4_one")   # the cheapest first
MX_CASES = ("checker8", "tiers4_one", "stagger8_one")   # at MX_SHAPE
MX_CUBE_CASES = ("checker8", "tiers4_one")   # at MX_CUBE
ALL_CASES = ([(name, SHAPE) for name in CASES] + [(name, MX_SHAPE) for name in MX_CASES]
             + [(name, MX_CUBE) for name in MX_CUBE_CASES])
CASE_IDS = ["%s-%dx%dx%d" % ((name,) + shape) for name, shape in ALL_CASES]


@functools.lru_cache(maxsize=3)
def case(name, shape_zyx=SHAPE):
    """(coef uint64 (z, y, x), sign uint64 words, wide?) of the named case, read-only"""
    if name in _EXTREMES:
        coef, sign, wide = coefficient_pattern(name, shape_zyx)
    else:
        coef = np.ascontiguousarray(_BUILDERS[name](shape_zyx), dtype=np.uint64)
        sign = np.ascontiguousarray(_hash_words(((coef.size + 63) // 64,), _SIGN_SEED))
        wide = name.startswith("wide_")
    coef.setflags(write=False)
    sign.setflags(write=False)
    return coef, sign, wide


# ---- the reach model ---------------------------------------------------------------------------------------------

def _bit_top(m):
    """the highest set bit of every element, -1 for zero"""
    top = np.full(m.shape, -1, dtype=np.int64)
    for k in range(64):
        top[(m >> _U(k)) != 0] = k
    return top


def box_tops(coef, e):
    """int64 (boxes z, y, x): the top plane of every box of edge e, -1 for an all-zero box"""
    nb = tuple((s + e - 1) // e for s in coef.shape)
    pad = np.zeros(tuple(n * e for n in nb), dtype=np.uint64)
    pad[:coef.shape[0], :coef.shape[1], :coef.shape[2]] = coef
    m = pad.reshape(nb[0], e, nb[1], e, nb[2], e).max(axis=(1, 3, 5))
    return _bit_top(m)


def list_reach(coef, e):
    """[(p, L, S)] per plane p from the top one down to 0.  L: the boxes of edge e whose 2e parent has its top plane
    above p while their own is <= p -- the parent has split, the box has not: the entries of that list on entering
    plane p.  S: those of them whose top plane is p -- the entries that plane finds significant."""
    own = box_tops(coef, e)
    nb = own.shape
    even = tuple(n + (n & 1) for n in nb)
    pad = np.full(even, -1, dtype=np.int64)
    pad[:nb[0], :nb[1], :nb[2]] = own
    par = pad.reshape(even[0] // 2, 2, even[1] // 2, 2, even[2] // 2, 2).max(axis=(1, 3, 5))
    par = np.repeat(np.repeat(np.repeat(par, 2, axis=0), 2, axis=1), 2, axis=2)[:nb[0], :nb[1], :nb[2]]
    top = int(own.max())
    rows = []
    o, q = own.reshape(-1), par.reshape(-1)
    for p in range(top, -1, -1):
        inl = (o <= p) & (q > p)
        rows.append((p, int(inl.sum()), int((inl & (o == p)).sum())))
    return rows


# The conditions the table is built for, at SHAPE: (case, box edge of the list, column, planes).
#   "zeros": a long list that is almost all '0' (S / L <= 0.02)      "half": about half '1' (0.3 <= S / L <= 0.7)
#   "ones":  a long list that is all '1' (S / L >= 0.95)
# A long list has L >= 512 for the 8^3 sets (k_lis_l2's threshold) and L >= 4096 for the 4^3 and 2^3 sets.
L_MIN = {8: 512, 4: 4096, 2: 4096}
RATIO = {"zeros": (0.0, 0.02), "half": (0.3, 0.7), "ones": (0.95, 1.0)}
CONDITIONS = (
    ("checker8", 8, "zeros", tuple(range(22, -1, -1))),
    ("tiers8_all", 8, "half", (14,)),
    ("tiers8_all", 8, "ones", (3,)),
    ("stagger8_one", 4, "zeros", tuple(range(24, -1, -1))),
    ("tiers4_one", 4, "half", (14,)),
    ("tiers4_one", 4, "ones", (3,)),
    ("checker2", 2, "zeros", tuple(range(22, -1, -1))),
    ("tiers2_all", 2, "half", (14,)),
    ("tiers2_all", 2, "ones", (3,)),
)
# stagger8_one keeps the list of the 8^3 sets long while its length changes on every plane (checker8's never does):
# L >= 512 on at least this many planes.  With one box in 31 leaving on each plane, S / L is about 1 / (p + 1) there.
STAGGER8_LONG_PLANES = 26

# The plane a stream is cut one byte into: the one the conditions name, else the plane the lists are largest on
LONG_PLANE = {"last_only": 2, "first_only": 31, "all_one": 0, "checker8": 11, "stagger8_one": 9, "tiers8_all": 14,
              "tiers4_one": 14, "checker2": 11, "tiers2_all": 14, "front4": 13, "dense_top32": 31,
              "wide_tiers8_all": 40, "wide_stagger4_one": 20}


def bits_down_to(coef, plane):
    """The coefficients with every plane below `plane` + 1 shifted out: the coder's decisions on the planes above
    `plane` read those bits only, so the whole stream of this array is, bit for bit, what the stream of `coef` holds
    in front of plane `plane` -- its bit count is where that plane starts."""
    return np.ascontiguousarray(coef >> _U(plane + 1))


def cut_into_plane(encode, coef, sign, plane):
    """the length of the stream of (coef, sign) cut one byte into plane `plane`; encode(coef, sign) -> stream"""
    head = encode(bits_down_to(coef, plane), sign)
    start = int(np.frombuffer(head, dtype=np.uint64, count=1, offset=1)[0])
    return 9 + start // 8 + 1


def stream_cuts(stream):
    """the lengths a case's stream is decoded at besides the plane cut: whole, 1/2 and 1/7 of the payload"""
    return (len(stream), 9 + (len(stream) - 9) // 2, 9 + (len(stream) - 9) // 7)


def sign_bits(words, idx):
    """the sign bits of the coefficients idx (flat indices)"""
    return (words[idx >> 6] >> (idx & 63).astype(np.uint64)) & _U(1)


# ---- grafting a stream into a container --------------------------------------------------------------------------

def graft_speck(container, streams):
    """container: a container of non-constant chunks; streams: {chunk index: SPECK stream}.  Each chosen chunk keeps
    its 17-byte conditioner header (src/SPECK_FLT.cpp:88-103) and the given stream replaces everything behind it;
    the other chunks stay.  The SPECK twin of outlier_cases.graft."""
    flags, vol, cd, parts = split_container(container)
    parts = list(parts)
    for i, s in streams.items():
        assert len(parts[i]) > 17 and not parts[i][0] & 0x01, "a constant chunk has no SPECK stream"
        parts[i] = bytes(parts[i][:17]) + bytes(s)
    return build_container(parts, vol, cd, bool(flags & 0x20), bool(flags & 0x80))
