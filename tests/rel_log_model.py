"""A numpy statement of the LOG kind of point-wise relative error (include/sperr_hip.h, "relative error", map kind 1),
written out independently of sperr_amd/csrc/rel.h: y is log2|x| itself, not its piecewise linear interpolant, and the
inverse is 2^y'.  Both maps are built from IEEE + - * /, floor, ldexp and bit casts alone, each operation rounded once
and in the order written here, so that the library, the host check and this model give the same bits.  What the two
kinds share -- the zero class, the signs, the stretch of the subnormal floats, the clamp, the narrowing, the SPMK
streams, the adversarial samples -- is tests/rel_model.py's."""
import numpy as np

import rel_model as R

f64 = np.float64
SQRT2 = f64(float.fromhex("0x1.6a09e667f3bcdp+0"))
LN2 = f64(float.fromhex("0x1.62e42fefa39efp-1"))
# 2 / (ln 2 * (2 k + 1)), k = 0 .. 10: log2(m) = s * sum c_k s^2k with s = (m - 1) / (m + 1)
LOG_C = [f64(float.fromhex(h)) for h in (
    "0x1.71547652b82fep+1", "0x1.ec709dc3a03fdp-1", "0x1.2776c50ef9bfep-1", "0x1.a61762a7aded9p-2",
    "0x1.484b13d7c02a9p-2", "0x1.0c9a84994022dp-2", "0x1.c68f568d31760p-3", "0x1.89f3b1694cffep-3",
    "0x1.5b9ac9b743f0dp-3", "0x1.3703c1f4d0ffep-3", "0x1.1964ec6fc9491p-3")]
# 1 / k!, k = 0 .. 13
EXP_C = [f64(float.fromhex(h)) for h in (
    "0x1p+0", "0x1p+0", "0x1p-1", "0x1.5555555555555p-3", "0x1.5555555555555p-5", "0x1.1111111111111p-7",
    "0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-13", "0x1.a01a01a01a01ap-16", "0x1.71de3a556c734p-19",
    "0x1.27e4fb7789f5cp-22", "0x1.ae64567f544e4p-26", "0x1.1eed8eff8d898p-29", "0x1.6124613a86d09p-33")]
DBL_MAX = float(np.finfo(np.float64).max)
MAGIC = b"SPLG"


def log2(mag):
    """log2 of normal positive doubles: the mantissa folded into [sqrt(1/2), sqrt(2)), an odd series in
    s = (m - 1) / (m + 1) by Horner in s^2, then the exponent added in one step"""
    u = np.ascontiguousarray(mag, dtype=np.float64).view(np.uint64)
    e = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((u & np.uint64((1 << 52) - 1)) | np.uint64(0x3FF << 52)).view(np.float64)
    up = m >= SQRT2
    m = np.where(up, m * f64(0.5), m)
    e = np.where(up, e + 1, e)
    s = (m - f64(1.0)) / (m + f64(1.0))
    z = s * s
    p = np.full(z.shape, LOG_C[10])
    for c in LOG_C[9::-1]:
        p = p * z + c
    return e.astype(np.float64) + s * p


def exp2(y):
    """2^y for y in [-1080, 1024): y = e + f with f in (-1/2, 1/2], the series of exp(f ln 2) by Horner, ldexp.  Finite:
    where the last rounding would reach 2^1024 the result is DBL_MAX; below 2^-1075 it is +0.0"""
    y = np.asarray(y, dtype=np.float64)
    e = np.floor(y)
    f = y - e
    up = f > f64(0.5)
    f = np.where(up, f - f64(1.0), f)
    e = np.where(up, e + f64(1.0), e)
    w = f * LN2
    p = np.full(w.shape, EXP_C[13])
    for c in EXP_C[12::-1]:
        p = p * w + c
    with np.errstate(over="ignore", under="ignore"):
        a = np.ldexp(p, e.astype(np.int32))
    return np.where((e == 1024.0) & ~(p < 1.0), f64(DBL_MAX), a)


def tolerance(eps, is_float):
    """t of eps for this kind, or None where eps is refused"""
    eps = f64(eps)
    if not np.isfinite(eps) or not eps > 0.0 or not eps <= R.EPS_MAX:
        return None
    s = f64(R.slack(is_float))
    t = log2(np.array([f64(1.0) + eps]))[0] - s
    return float(t) if t >= s else None


def tolerance_floor(is_float):
    """the smallest eps this kind accepts, by bisection on the doubles' bit patterns"""
    lo, hi = 0, int(f64(R.EPS_MAX).view(np.uint64))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if tolerance(np.uint64(mid).view(np.float64), is_float) is None:
            lo = mid
        else:
            hi = mid
    return float(np.uint64(hi).view(np.float64))


def forward(x):
    """(y, zero, neg) of a float32 / float64 array, flat; None where a sample is not finite"""
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.float64)
    zero, neg, finite = R.classes(x)
    if not finite.all():
        return None
    mag = np.abs(x.reshape(-1).astype(np.float64))
    y = log2(np.where(zero, f64(1.0), mag))
    if x.dtype == np.float32:
        y = np.where(y < R.SUB_FLOAT, R.SUB_FLOAT + f64(2.0) * (y - R.SUB_FLOAT), y)
    y[zero] = np.uint64(R.NAN_BITS).view(np.float64)
    return y, zero, neg


def inverse(yp, zero, neg, output_float, is_float):
    """x' of y' (any shape) and the bits at the same positions; is_float: the SOURCE was fp32 data"""
    yp = np.asarray(yp, dtype=np.float64)
    if is_float:
        with np.errstate(invalid="ignore"):
            yp = np.where(yp < R.SUB_FLOAT, R.SUB_FLOAT + f64(0.5) * (yp - R.SUB_FLOAT), yp)
    zero, neg = np.asarray(zero).reshape(yp.shape), np.asarray(neg).reshape(yp.shape)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        c = np.where(yp >= R.Y_MIN, yp, R.Y_MIN)
        c = np.where(c > R.Y_MAX, R.Y_MAX, c)
        a = exp2(c)
        if output_float:
            a = np.where(a > R.FLT_MAX, np.float32(R.FLT_MAX), a.astype(np.float32)).astype(np.float32)
    a = np.where(zero, a.dtype.type(0), a)
    return np.where(neg, -a, a).astype(a.dtype)


def side_stream(zero, neg, eps, is_float):
    """the bytes of this kind's side stream: SPRL's layout under the magic "SPLG" """
    return MAGIC + R.side_stream(zero, neg, eps, is_float)[4:]


def parse(s):
    """(is_float, eps, n, zero, neg) of a side stream of this kind"""
    assert s[:4] == MAGIC
    return R.parse(b"SPRL" + s[4:])


def synthetic(n, dtype=np.float32):
    """tools/rel_bench.py::synthetic restated in numpy at n^3: six decades, both signs, smooth in the exponent, with a
    ball of zeros"""
    ax = np.arange(n, dtype=np.float64) * (2.0 * np.pi / n)
    z, y, x = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    expo = 3.0 * (np.sin(1.3 * x + 0.2) * np.cos(0.9 * y) + 0.6 * np.sin(0.7 * z + 1.0) * np.cos(2.1 * x + y))
    expo = np.clip(expo, -3.0, 3.0)
    wave = np.sin(3.1 * x + 2.3 * y + 1.7 * z) + 0.05 * np.sin(17.0 * x) * np.sin(13.0 * y + z)
    v = np.power(10.0, expo) * (1.0 + 0.3 * wave)
    v = np.where(np.cos(1.1 * x + 0.4 * z) * np.sin(0.8 * y + 0.3) > -0.2, v, -v)
    c = np.arange(n, dtype=np.float64) - n / 2
    v[(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) <= (n / 8) ** 2] = 0.0
    return np.ascontiguousarray(v.astype(dtype))
