"""PSNR of the whole volume, stated again in Python (sperr_amd/csrc/psnr_vol.h is the statement the library uses): the
common target, the ladder of five quantisation steps, the error estimate of a step on a chunk's coefficients, the pick
and the width rule.  Every number is a double handled as the header handles it; the fused multiply-adds are libm's."""
import ctypes as C
import ctypes.util
import math

import numpy as np

RUNGS = 5
STRIDE = 4096

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = C.c_double
_libm.fma.argtypes = [C.c_double] * 3
_libm.exp2.restype = C.c_double
_libm.exp2.argtypes = [C.c_double]
_fma = getattr(math, "fma", _libm.fma)


def value_range(vol):
    """double(max) - double(min) of the raw samples: one subtraction"""
    return float(np.float64(vol.max()) - np.float64(vol.min()))


def ladder(rng, psnr):
    """(t, [q_0 .. q_4]) in the reference's order of operations"""
    t = (rng * rng) * math.pow(10.0, -psnr / 10.0)
    q = 2.0 * math.sqrt(t * 3.0)
    step = _libm.exp2(0.25)
    qs = []
    for _ in range(RUNGS):
        qs.append(q)
        q = q / step
    return t, qs


def stride_sums(vals, q):
    """the sums of the strides of 4096, the last one short or empty, each added up in order"""
    v = np.ascontiguousarray(vals, dtype=np.float64).ravel()
    rcp = 1.0 / q
    r = np.rint(v * rcp)   # (one rounding of the product, then round-half-even: elementwise, as the chain takes them)
    sums = []
    for beg in range(0, (v.size // STRIDE) * STRIDE + 1, STRIDE):
        acc = 0.0
        for i in range(beg, min(beg + STRIDE, v.size)):
            diff = _fma(-q, float(r[i]), float(v[i]))
            acc = _fma(diff, diff, acc)
        sums.append(acc)
    return sums


def estimate(vals, q):
    total = 0.0
    for s in stride_sums(vals, q):
        total += s
    return total / float(np.asarray(vals).size)


def pick(vals, t, qs):
    """(rung, mse of that rung): the first rung whose estimate is at most t; (None, mse of the last) when none is"""
    mse = 0.0
    for k, q in enumerate(qs):
        mse = estimate(vals, q)
        if mse <= t:
            return k, mse
    return None, mse


def width(maxabs, q):
    """4 or 8 bytes a coefficient; None: refused (2^63 steps or more, or a NaN)"""
    m = maxabs / q
    if not m < 2.0 ** 63:
        return None
    return 8 if int(np.rint(m)) > 0xffffffff else 4


def chunk_q(vals, rng, psnr):
    """(q, rung) of a chunk's coefficients at the common range"""
    t, qs = ladder(rng, psnr)
    k, _ = pick(vals, t, qs)
    return (None, None) if k is None else (qs[k], k)


def ladder_chunk(oracle, signs_shape_zyx, seed=11):
    """A chunk whose coefficients are all about +-1: the inverse transform of random signs, plus 3.0 -- the input the
    ladder tests are built on (its error estimate at q is nearly that of the constant 1)"""
    rng = np.random.default_rng(seed)
    w = np.where(rng.random(signs_shape_zyx) < 0.5, -1.0, 1.0)
    return oracle.idwt3d(w) + 3.0


def range_for(inv_q0, psnr):
    """the range whose ladder starts at q_0 = 1 / inv_q0 (to rounding): q_0 = 2 sqrt(3) range 10^(-psnr/20)"""
    return (1.0 / inv_q0) / (2.0 * math.sqrt(3.0)) * math.pow(10.0, psnr / 20.0)


LADDER_SHAPES = {"16": (16, 16, 16), "17": (17, 17, 17), "20x18x16": (16, 18, 20)}   # (z, y, x)
LADDER_INV_Q0 = (0.26, 0.60, 0.50, 0.35, 0.30)   # the oracle stops at rungs 0, 1, 2, 3, 4
LADDER_PSNR = 60.0
