"""A numpy statement of the smooth in-fill of missing values (include/sperr_hip.h, SPERRHIP_FILL_SMOOTH), written out
independently of sperr_amd/csrc/mask_fill.h: the levels as arrays, the pull with its fixed order of the children, the push
axis by axis.  Every operation is one numpy double operation on whole arrays, so nothing is fused.  The predicate, the
masks and the stream are tests/mask_model.py's.  The tests compare the library and tests/cpp/mask_fill_check.cpp with it."""
import numpy as np

import mask_model as M  # noqa: F401  (the predicate, the masks and the stream, for the tests that import this module)

FILL_MIDRANGE, FILL_VALUE, FILL_SMOOTH = 0, 1, 2
HEAD_BYTES = 256


def level_shapes(shape_zyx):
    """[(z, y, x)] of the levels 0 .. L"""
    s = tuple(int(d) for d in shape_zyx)
    assert len(s) == 3 and min(s) >= 1
    out = [s]
    while max(out[-1]) > 1:
        out.append(tuple((d + 1) // 2 for d in out[-1]))
    return out


def global_levels(shape_zyx, top_cells):
    """G: how many levels l >= 1 the device keeps in global memory (0 for a volume of one sample)"""
    shapes = level_shapes(shape_zyx)
    if len(shapes) == 1:
        return 0
    return max(1, sum(1 for s in shapes[1:] if s[0] * s[1] * s[2] > top_cells))


def pyramid_bytes(shape_zyx, top_cells):
    """the device's pyramid buffer: the head and the levels 1 .. G as doubles"""
    shapes = level_shapes(shape_zyx)
    g = global_levels(shape_zyx, top_cells)
    if g == 0:
        return 0
    return HEAD_BYTES + 8 * sum(s[0] * s[1] * s[2] for s in shapes[1:g + 1])


def launches(shape_zyx, top_cells):
    """{kernel: launches} of one smooth fill"""
    g = global_levels(shape_zyx, top_cells)
    assert g >= 1
    return {"k_mask_pull0": 1, "k_mask_pull": g - 1, "k_mask_top": 1, "k_mask_push": g - 1, "k_mask_fill_smooth": 1}


def pq(i, dim):
    """(P, Q) of coordinate i against a coarser level of extent dim"""
    p = i >> 1
    if i & 1:
        return p, min(p + 1, dim - 1)
    return p, (0 if p == 0 else p - 1)


def _pull(val, known):
    """(values, known, all sums finite) of the next level"""
    shape = tuple((d + 1) // 2 for d in val.shape)
    s = np.zeros(shape, dtype=np.float64)
    k = np.zeros(shape, dtype=np.int64)
    for c in (0, 1):
        for b in (0, 1):
            for a in (0, 1):
                v = val[c::2, b::2, a::2]
                kn = known[c::2, b::2, a::2]
                part = (slice(0, v.shape[0]), slice(0, v.shape[1]), slice(0, v.shape[2]))
                with np.errstate(over="ignore", invalid="ignore"):
                    s[part] = np.where(kn, s[part] + v, s[part])
                k[part] += kn
    finite = bool(np.isfinite(s).all())
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(k > 0, s / np.maximum(k, 1).astype(np.float64), np.float64(0.0))
    return out, k > 0, finite


def _push(coarse, shape):
    """the interpolated value of every cell of a level of `shape` from the complete level above it"""
    idx = [np.array([pq(i, coarse.shape[ax]) for i in range(shape[ax])], dtype=np.int64).reshape(-1, 2) for ax in range(3)]
    h, q = np.float64(0.75), np.float64(0.25)
    with np.errstate(over="ignore", invalid="ignore"):
        t = h * coarse[:, :, idx[2][:, 0]]
        t = t + q * coarse[:, :, idx[2][:, 1]]
        u = h * t[:, idx[1][:, 0], :]
        u = u + q * t[:, idx[1][:, 1], :]
        w = h * u[idx[0][:, 0]]
        w = w + q * u[idx[0][:, 1]]
    return w


def smooth_filled(a, miss):
    """the in-filled array (a's shape and dtype; fewer than three dimensions lead with 1s), or None when a sum of the
    pull is not finite (the call fails)"""
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.float64) and a.ndim <= 3
    shape = (1,) * (3 - a.ndim) + a.shape
    src = a.reshape(shape)
    known = ~np.asarray(miss, dtype=bool).reshape(shape)
    if src.size == 1:
        out = src.copy()
        out[~known] = 0
        return out.reshape(a.shape)
    with np.errstate(invalid="ignore"):     # (a signalling NaN among the missing samples, widened and then dropped)
        vals = [np.where(known, src.astype(np.float64), np.float64(0.0))]
    knowns = [known]
    while max(vals[-1].shape) > 1:
        v, kn, finite = _pull(vals[-1], knowns[-1])
        if not finite:
            return None
        vals.append(v)
        knowns.append(kn)
    if not knowns[-1][0, 0, 0]:
        vals[-1][0, 0, 0] = 0.0
    for lev in range(len(vals) - 2, -1, -1):
        w = _push(vals[lev + 1], vals[lev].shape)
        vals[lev] = np.where(knowns[lev], vals[lev], w)
    out = src.copy()
    out[~known] = vals[0][~known].astype(a.dtype)
    return out.reshape(a.shape)


def value_filled(a, miss, value):
    out = np.array(a, copy=True)
    out[np.asarray(miss, dtype=bool).reshape(a.shape)] = a.dtype.type(value)
    return out
