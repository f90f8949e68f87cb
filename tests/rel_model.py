"""A numpy statement of the rule of point-wise relative error (include/sperr_hip.h, "relative error"), written out
independently of sperr_amd/csrc/rel.h: the forward map to y with the zero class and the signs, the tolerance, the
inverse, the side stream "SPRL" and the figures of the check.  The SPMK payloads are tests/mask_model.py's.  The tests
compare the library and tests/cpp/rel_check.cpp with it."""
import os
import struct

import numpy as np

import mask_model as M

HEADER_BYTES = 48
NAN_BITS = 0x7FF8000000000000
EPS_MAX = 0.5
Y_MIN, Y_MAX = -1080.0, float(np.nextafter(np.float64(1024.0), np.float64(0.0)))
FLT_MAX = float(np.finfo(np.float32).max)
SUB_FLOAT = np.float64(-126.0)   # y of the smallest normal float


def slack(is_float):
    return 2.0 ** -22 if is_float else 2.0 ** -40


def tolerance(eps, is_float):
    """t of eps, or None where eps is refused"""
    eps = np.float64(eps)
    if not np.isfinite(eps) or not eps <= EPS_MAX:
        return None
    s = np.float64(slack(is_float))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = eps / (np.float64(1.0) + eps) - s
    return float(t) if t >= s else None


def tolerance_floor(is_float):
    """the smallest eps that is accepted, found by bisection on the doubles' bit patterns"""
    lo, hi = np.float64(0.0).view(np.uint64), np.float64(EPS_MAX).view(np.uint64)
    lo, hi = int(lo), int(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if tolerance(np.uint64(mid).view(np.float64), is_float) is None:
            lo = mid
        else:
            hi = mid
    return float(np.uint64(hi).view(np.float64))


def classes(x):
    """(zero, neg, finite) bool arrays of the samples, flat"""
    d = np.ascontiguousarray(x).reshape(-1).astype(np.float64)
    u = d.view(np.uint64)
    E = (u >> np.uint64(52)) & np.uint64(0x7FF)
    return E == 0, (u >> np.uint64(63)) != 0, E != 0x7FF


def forward(x):
    """(y, zero, neg) of a float32 / float64 array, flat; None where a sample is not finite (the call is refused)"""
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.float64)
    zero, neg, finite = classes(x)
    if not finite.all():
        return None
    u = x.reshape(-1).astype(np.float64).view(np.uint64)
    E = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    Mant = (u & np.uint64((1 << 52) - 1)).astype(np.float64)
    y = (E - 1023).astype(np.float64) + Mant * np.float64(2.0 ** -52)
    if x.dtype == np.float32:   # the subnormal floats: twice the resolution
        y = np.where(y < SUB_FLOAT, SUB_FLOAT + np.float64(2.0) * (y - SUB_FLOAT), y)
    y[zero] = np.uint64(NAN_BITS).view(np.float64)
    return y, zero, neg


def inverse(yp, zero, neg, output_float, is_float):
    """x' of y' (any shape) and the bits at the same positions, in y's shape; is_float: the SOURCE was fp32 data"""
    yp = np.asarray(yp, dtype=np.float64)
    if is_float:
        with np.errstate(invalid="ignore"):
            yp = np.where(yp < SUB_FLOAT, SUB_FLOAT + np.float64(0.5) * (yp - SUB_FLOAT), yp)
    zero, neg = np.asarray(zero).reshape(yp.shape), np.asarray(neg).reshape(yp.shape)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        c = np.where(yp >= Y_MIN, yp, Y_MIN)
        c = np.where(c > Y_MAX, Y_MAX, c)
        e = np.floor(c)
        m = c - e
        a = np.ldexp(np.float64(1.0) + m, e.astype(np.int32))
        if output_float:
            a = np.where(a > FLT_MAX, np.float32(FLT_MAX), a.astype(np.float32)).astype(np.float32)
    a = np.where(zero, a.dtype.type(0), a)
    return np.where(neg, -a, a).astype(a.dtype)


def side_stream(zero, neg, eps, is_float):
    """the bytes of the side stream"""
    z, s = M.stream(zero), M.stream(neg)
    pad = b"\0" * (-len(z) % 8)
    head = b"SPRL" + bytes([1, int(bool(is_float)), 0, 0]) + struct.pack("<dQQQQ", float(eps), np.asarray(zero).size,
                                                                       len(z), len(s), 0)
    assert len(head) == HEADER_BYTES
    return head + z + pad + s


def max_size(n):
    return HEADER_BYTES + 2 * M.max_size(n)


def parse(s):
    """(is_float, eps, n, zero, neg) of a side stream"""
    assert s[:4] == b"SPRL" and s[4] == 1 and s[5] in (0, 1) and s[6:8] == b"\0\0"
    eps, n, zl, sl, rsv = struct.unpack("<dQQQQ", s[8:48])
    at = 48 + (zl + 7) // 8 * 8
    assert rsv == 0 and len(s) == at + sl
    zero, neg = M.bits_of_stream(s[48:48 + zl]), M.bits_of_stream(s[at:])
    assert zero.size == n and neg.size == n
    return s[5], eps, n, zero, neg


def check(x, xr, eps):
    """the four figures of sperrhip_rel_check_dev: the largest |x' - x| / |x| over the samples outside the zero class,
    how many of them have |x' - x| > eps |x|, how many samples differ in zero class or sign, and the first count"""
    a = np.ascontiguousarray(x).reshape(-1).astype(np.float64)
    b = np.ascontiguousarray(xr).reshape(-1).astype(np.float64)
    za, na, _ = classes(a)
    zb, nb, _ = classes(b)
    err, mag = np.abs(b - a)[~za], np.abs(a)[~za]
    worst = float((err / mag).max()) if mag.size else 0.0
    return worst, int((~(err <= np.float64(eps) * mag)).sum()), int(((za != zb) | (na != nb)).sum()), int(mag.size)


# ---- the adversarial samples of the rule's statement -----------------------------------------------------------------
def adversarial(dtype):
    """powers of two from 2^-149 to 2^127 with both neighbours, float subnormals, +-0.0, the largest value, negative
    copies; for float64 also double subnormals and DBL_MAX"""
    f32 = []
    for e in range(-149, 128):
        p = np.float32(2.0 ** e)
        f32 += [p, np.nextafter(p, np.float32(np.inf)), np.nextafter(p, np.float32(0))]
    f32 += [np.uint32(k).view(np.float32) for k in (1, 2, 3, 5, 64, 65, 0x7FFFFF, 0x400001, 0x123456)]
    f32 += [np.float32(0.0), np.float32(-0.0), np.finfo(np.float32).max, np.float32(1.5), np.float32(3.1415927)]
    v = np.array(f32, dtype=np.float32)
    if dtype == np.float64:
        d = [np.float64(2.0 ** e) for e in (-900, -500, 500, 1023)]
        d = [q for p in d for q in (p, np.nextafter(p, np.inf), np.nextafter(p, 0.0))]
        d += [np.uint64(k).view(np.float64) for k in (1, 2, 0xFFFFFFFFFFFFF, 0x8000000000000)]   # double subnormals
        d += [np.finfo(np.float64).max, np.float64(1.0) + 2.0 ** -52, np.float64(np.pi)]
        v = np.concatenate([v.astype(np.float64), np.array(d, dtype=np.float64)])
    return np.concatenate([v, -v])


def planted_volume(shape_zyx, dtype, seed=11):
    """a volume spanning 2^-140 to 2^120, both signs, a ball of zeros, the adversarial samples planted from index 7"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape_zyx))
    mag = np.exp2(rng.uniform(-140.0, 120.0, n))
    v = (mag * rng.choice([-1.0, 1.0], n)).astype(dtype)
    v[M.ball_mask(shape_zyx, min(shape_zyx) / 4).reshape(-1)] = 0
    adv = adversarial(dtype)
    v[7:7 + adv.size] = adv
    return v.reshape(shape_zyx)


def vort_with_zeros():
    """tests/golden/vort_crop.f32 (33, 36, 40) with a ball of samples set to zero and a few -0.0"""
    here = os.path.dirname(os.path.abspath(__file__))
    vol = np.fromfile(os.path.join(here, "golden", "vort_crop.f32"), dtype=np.float32).reshape(33, 36, 40).copy()
    vol[M.ball_mask(vol.shape, 9)] = 0.0
    flat = vol.reshape(-1)
    flat[[5, 1234, 20000, flat.size - 1]] = -0.0
    return vol
