"""Deterministic test fields. `smooth_field` uses only integer arithmetic and exact float
conversions, so its bytes are identical on every machine (golden vectors depend on that)."""
import numpy as np

_M64 = (1 << 64) - 1


def _splitmix_array(n, seed):
    idx = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) + np.uint64(seed)
    z = idx
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def smooth_field(shape_zyx, seed=7, dtype=np.float32, passes=3):
    """Integer noise, box-smoothed `passes` times along each axis by exact integer sums, scaled
    by a power of two: every value is exactly representable in float32."""
    n = int(np.prod(shape_zyx))
    with np.errstate(over="ignore"):
        r = _splitmix_array(n, seed)
    v = ((r >> np.uint64(48)).astype(np.int64) - 32768).reshape(shape_zyx)
    for _ in range(passes):
        for ax in range(3):
            v = v + np.roll(v, 1, axis=ax) + np.roll(v, -1, axis=ax)
    # |v| < 2^15 * 27^passes < 2^15 * 2^15 ; keep 20 significant bits so float32 is exact
    v = v >> 10
    return (v.astype(np.float64) / 64.0).astype(dtype)


def ramp_field(shape_zyx, dtype=np.float32):
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.int64) for s in shape_zyx], indexing="ij")
    return ((x * 3 + y * 5 - z * 7) % 97).astype(dtype)


# ---- value domains --------------------------------------------------------------------------------------------
# Fields with the value ranges real data has: one-signed, far from zero, sparse, discontinuous, tiny and huge units.
# They are built from smooth_field (multiples of 2^-6 below 2^14 in magnitude, at most 20 significant bits), the hash
# words of _splitmix_array and exact or correctly rounded IEEE operations only (+, -, x by a power of two, comparisons,
# round, astype): no libm call, so their bytes are the same on every machine (tests/golden/ref_digests.json depends
# on that).

def _hash_words(shape_zyx, seed):
    with np.errstate(over="ignore"):
        return _splitmix_array(int(np.prod(shape_zyx)), seed).reshape(shape_zyx)


def _pow2(k):
    """2.0 ** k as float64 for integer arrays or scalars -1022 <= k <= 1023, from the exponent field's bits"""
    return ((np.asarray(k, dtype=np.int64) + 1023) << 52).view(np.float64)


def _white(shape_zyx, seed=11):
    """24 hash bits mapped to [-1, 1): exact in float32"""
    return (_hash_words(shape_zyx, seed) >> np.uint64(40)).astype(np.float64) * _pow2(-23) - 1.0


def _checker(shape_zyx):
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.int64) for s in shape_zyx], indexing="ij")
    return (1 - 2 * ((x + y + z) & 1)).astype(np.float64)


def _step(shape_zyx):
    """0 up to an odd (so non-dyadic) cut along x, 1000 beyond"""
    cut = (shape_zyx[2] // 3) | 1
    v = np.zeros(shape_zyx, dtype=np.float64)
    v[:, :, cut:] = 1000.0
    return v


def _spike(shape_zyx):
    v = np.zeros(shape_zyx, dtype=np.float64)
    v[tuple(min(s - 1, s // 2 + 1) for s in shape_zyx)] = 1.0
    return v


def _neg_zero(s):
    v = s.copy()
    v[np.abs(s) < 128.0] = -0.0
    return v


def _offset(s, dtype):
    """one-signed with a large mean; the sum is rounded to `dtype` (correctly, hence the same everywhere)"""
    return s.astype(dtype) + dtype(2.0 ** 20 if dtype == np.float32 else 2.0 ** 27)


PATCHWORK_SHAPE = (40, 40, 56)   # 12 cells of the 16^3 chunking (x: 16 16 24, y and z: 16 24): 8 chunk shapes
PATCHWORK_CELLS = ("smooth", "offset_pos", "scale_2p60", "scale_2m60", "zero", "const", "white", "checker",
                   "all_negative", "integers", "scale_2m140", "step")
PATCHWORK_MILD_CELLS = ("smooth", "offset_pos", "binary", "neg_zero", "zero", "const", "white", "checker",
                        "all_negative", "integers", "spike", "step")   # the scaled cells replaced by mild ones


def _cell(name, shape_zyx, seed):
    s = smooth_field(shape_zyx, seed=seed, dtype=np.float64)
    if name == "smooth":
        return s
    if name == "offset_pos":
        return _offset(s, np.float32)
    if name.startswith("scale_2"):
        return s * _pow2((-1 if name[7] == "m" else 1) * int(name[8:]))
    if name == "zero":
        return np.zeros(shape_zyx)
    if name == "const":
        return np.full(shape_zyx, 3.25)
    if name == "white":
        return _white(shape_zyx, seed)
    if name == "checker":
        return _checker(shape_zyx)
    if name == "all_negative":
        return -(np.abs(s) + 7.0)
    if name == "integers":
        return np.round(s)
    if name == "binary":
        return (_hash_words(shape_zyx, seed) >> np.uint64(63)).astype(np.float64)
    if name == "neg_zero":
        return _neg_zero(s)
    if name == "spike":
        return _spike(shape_zyx)
    if name == "step":
        return _step(shape_zyx)
    raise KeyError(name)


def patchwork_field(cells=PATCHWORK_CELLS):
    """float32 (40, 40, 56): every cell of the 16^3 chunking holds a different kind of data, so one call codes chunks
    whose dynamic ranges differ by 2^200, a constant and an all-zero chunk among them"""
    from sperr_amd.farm import chunk_grid
    grid = chunk_grid(PATCHWORK_SHAPE, (16, 16, 16))
    assert len(grid) == len(cells)
    v = np.zeros(PATCHWORK_SHAPE, dtype=np.float32)
    for k, (name, (x0, lx, y0, ly, z0, lz)) in enumerate(zip(cells, grid)):
        v[z0:z0 + lz, y0:y0 + ly, x0:x0 + lx] = _cell(name, (lz, ly, lx), 100 + k).astype(np.float32)
    return v


def value_domain_fields(shape_zyx, dtype):
    """Ordered dict name -> array of `dtype` shaped shape_zyx (the two patchworks: float32 only, PATCHWORK_SHAPE).
    FIXED_RATE_ONLY names the fields only mode 1 may see; PATCHWORK_MODES the modes of the patchworks."""
    dtype = np.dtype(dtype).type
    f32 = dtype == np.float32
    s = smooth_field(shape_zyx, dtype=np.float64)
    h = _hash_words(shape_zyx, 23)
    out = {}
    out["offset_pos"] = _offset(s, dtype)
    out["all_negative"] = -(np.abs(s) + 7.0)
    out["scale_up"] = s * _pow2(66)
    out["scale_down"] = s * _pow2(-66)
    out["scale_extreme_up"] = s * _pow2(100 if f32 else 990)
    out["scale_extreme_down"] = s * _pow2(-100 if f32 else -1000)
    if f32:
        out["subnormal_f32"] = s * _pow2(-140)   # k 2^-146, k < 2^20: subnormal and exact in float32
    out["spike"] = _spike(shape_zyx)
    out["step"] = _step(shape_zyx)
    out["checker"] = _checker(shape_zyx)
    out["white"] = _white(shape_zyx)
    out["binary"] = (h >> np.uint64(63)).astype(np.float64)
    out["integers"] = np.round(s)
    out["neg_zero"] = _neg_zero(s)
    out["wide_dynamic"] = s * _pow2((h % np.uint64(81)).astype(np.int64) - 40)
    out = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in out.items()}
    if f32:
        out["patchwork"] = patchwork_field(PATCHWORK_CELLS)
        out["patchwork_mild"] = patchwork_field(PATCHWORK_MILD_CELLS)
    return out


VALUE_DOMAIN_NAMES = ("offset_pos", "all_negative", "scale_up", "scale_down", "scale_extreme_up", "scale_extreme_down",
                      "subnormal_f32", "spike", "step", "checker", "white", "binary", "integers", "neg_zero",
                      "wide_dynamic", "patchwork", "patchwork_mild")
F32_ONLY = ("subnormal_f32", "patchwork", "patchwork_mild")
VALUE_DOMAIN_CASES = [(n, d) for d in ("float32", "float64") for n in VALUE_DOMAIN_NAMES
                      if d == "float32" or n not in F32_ONLY]
FIXED_RATE_ONLY = ("scale_extreme_up", "scale_extreme_down")
PATCHWORK_MODES = {"patchwork": (1, 2), "patchwork_mild": (1, 2, 3)}


# The reference sizes the outlier coder's integers by llrint of the largest raw error (src/Outlier_Coder.cpp:82-91) and
# refuses the chunk when that raises FE_INVALID, i.e. from an error of 2^63 on: scale_up (values near 2^77) with a
# tolerance of 1e-2 of its span has such outliers, and through its C API the reference does not survive the refusal
# in 3D.  That setting is therefore no container case; the tests ask the oracle and the engine to refuse it.
REFUSED_BY_OUTLIER_RULE = {"scale_up": 1e-2}


def _span(v):
    return float(v.astype(np.float64).max() - v.astype(np.float64).min()) or 1.0


def value_domain_settings(name, v):
    """[(mode, quality)] of the container grid for field `name`: 0.5, 4 and 24 bpp; 40 and 120 dB; a tolerance of
    1e-2 and of 1e-5 of the span (of 1.0 where the span is 0)"""
    modes = (1,) if name in FIXED_RATE_ONLY else PATCHWORK_MODES.get(name, (1, 2, 3))
    grid = [(1, 0.5), (1, 4.0), (1, 24.0), (2, 40.0), (2, 120.0)]
    grid += [(3, _span(v) * f) for f in (1e-2, 1e-5) if REFUSED_BY_OUTLIER_RULE.get(name) != f]
    return [(m, q) for m, q in grid if m in modes]


def value_domain_refused(name, v):
    """[(mode, quality)]: what the reference's outlier rule refuses of the grid"""
    return [(3, _span(v) * REFUSED_BY_OUTLIER_RULE[name])] if name in REFUSED_BY_OUTLIER_RULE else []


_FIELD_CACHE = {}


def cached_value_domain_fields(shape_zyx, dtype):
    """value_domain_fields, built once per (shape, dtype) and handed out read-only"""
    key = (tuple(shape_zyx), np.dtype(dtype).name)
    if key not in _FIELD_CACHE:
        d = value_domain_fields(shape_zyx, dtype)
        for a in d.values():
            a.setflags(write=False)
        _FIELD_CACHE[key] = d
    return _FIELD_CACHE[key]


# ---- coefficient patterns of the SPECK stage --------------------------------------------------------------------
COEF_PATTERNS = ("dense_top32", "all_max32", "all_one", "first_only", "last_only", "dense_top53", "one_bit_each",
                 "geometric")
COEF_SHAPES = [(16, 16, 16), (13, 21, 30), (32, 32, 32), (3, 5, 7), (1, 16, 16), (41, 64, 64)]
COEF_BUDGETS = (0, 777, 20000)


def coefficient_pattern(name, shape_zyx):
    """(coef uint64 (z, y, x), sign uint64 words from the hash, wide?): the extremes of occupancy a quantised chunk can
    have -- every coefficient significant on the first plane, one coefficient in all, one bit per coefficient, ..."""
    n = int(np.prod(shape_zyx))
    h = _hash_words((n,), 31)
    coef = np.zeros(n, dtype=np.uint64)
    if name == "dense_top32":      # bit 31 set everywhere, hash below
        coef = (h >> np.uint64(33)) | np.uint64(1 << 31)
    elif name == "all_max32":
        coef[:] = 0xFFFFFFFF
    elif name == "all_one":
        coef[:] = 1
    elif name == "first_only":
        coef[0] = 0x80000001
    elif name == "last_only":
        coef[-1] = 5
    elif name == "dense_top53":    # bit 52 set everywhere: the 64-bit path
        coef = (h >> np.uint64(12)) | np.uint64(1 << 52)
    elif name == "one_bit_each":
        coef = np.uint64(1) << (h % np.uint64(32))
    elif name == "geometric":      # as many coefficients with k bits as with k + 1
        coef = h >> (np.uint64(32) + h % np.uint64(32))
    else:
        raise KeyError(name)
    sign = _hash_words(((n + 63) // 64,), 37)
    return np.ascontiguousarray(coef.reshape(shape_zyx)), np.ascontiguousarray(sign), name == "dense_top53"


VD_SHAPE = (20, 33, 40)   # the container grid's volume: no extent a multiple of 16, two of them odd or non-dyadic


def value_domain_plane(name, dtype):
    """(plane z = 11 of the field at VD_SHAPE -- the spike lies in it --, [(mode, quality)] one per mode the field
    takes: 2 bpp, 90 dB, 1e-3 of the plane's span, [(mode, quality)] that the reference refuses: scale_up in mode 3,
    see REFUSED_BY_OUTLIER_RULE)"""
    v = cached_value_domain_fields(VD_SHAPE, dtype)[name]
    img = np.ascontiguousarray(v[11])
    quality = {1: 2.0, 2: 90.0, 3: _span(img) * 1e-3}
    modes = sorted({m for m, _ in value_domain_settings(name, v)})
    refused = [3] if name in REFUSED_BY_OUTLIER_RULE else []
    return img, [(m, quality[m]) for m in modes if m not in refused], [(m, quality[m]) for m in refused]
