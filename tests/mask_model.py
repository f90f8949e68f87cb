"""A numpy statement of the rules of missing values (include/sperr_hip.h, "masked volumes"), written out independently
of sperr_amd/csrc/mask.h: which samples are missing, the order of the valid ones, the fill value, the toggles, the kind
and the bytes of a mask stream.  The tests compare the library and tests/cpp/mask_check.cpp with it."""
import struct

import numpy as np

RULE_NAN, RULE_ABS_GE = 1, 2
KIND_NONE, KIND_TOGGLES, KIND_BITS = 0, 1, 2
HEADER_BYTES = 32


def missing(a, rule, threshold=0.0):
    """bool array: the missing samples of `a` (flat or not)"""
    a = np.asarray(a)
    if rule == RULE_NAN:
        return a != a
    assert rule == RULE_ABS_GE and np.isfinite(threshold) and threshold > 0
    with np.errstate(invalid="ignore"):
        return ~(np.abs(a.astype(np.float64)) < np.float64(threshold))


def ordered_key(a):
    """unsigned keys that compare as the sign-magnitude bit patterns of `a` do: -0.0 before +0.0"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        u, top, ones = a.view(np.uint32), np.uint32(1 << 31), np.uint32(0xFFFFFFFF)
    else:
        assert a.dtype == np.float64
        u, top, ones = a.view(np.uint64), np.uint64(1 << 63), np.uint64(0xFFFFFFFFFFFFFFFF)
    return np.where((u & top) != 0, u ^ ones, u | top)


def fill_value(a, miss):
    """F of the valid samples of `a`, in a's dtype; None when lo or hi is not finite (the call fails)"""
    a = np.ascontiguousarray(a).reshape(-1)
    valid = a[~np.asarray(miss).reshape(-1)]
    if valid.size == 0:
        return a.dtype.type(0)
    key = ordered_key(valid)
    lo, hi = valid[np.argmin(key)], valid[np.argmax(key)]
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return None
    f = np.float64(0.5) * np.float64(lo) + np.float64(0.5) * np.float64(hi)
    return a.dtype.type(f)


def filled(a, miss):
    """the in-filled array (a's shape), or None when the call fails"""
    f = fill_value(a, miss)
    if f is None:
        return None
    out = np.array(a, copy=True)
    out[np.asarray(miss).reshape(a.shape)] = f
    return out


def toggles(miss):
    """ascending positions p with bit(p) != bit(p - 1), bit(-1) = 0"""
    b = np.asarray(miss).reshape(-1).astype(np.uint8)
    prev = np.concatenate([np.zeros(1, dtype=np.uint8), b[:-1]])
    return np.flatnonzero(b != prev).astype(np.uint64)


def words(miss):
    """ceil(n / 64) little-endian 64-bit words, sample i at bit i % 64 of word i / 64, tail bits 0"""
    b = np.asarray(miss).reshape(-1).astype(np.uint8)
    nw = (b.size + 63) // 64
    pad = np.zeros(nw * 64, dtype=np.uint8)
    pad[:b.size] = b
    return np.packbits(pad, bitorder="little").view("<u8")


def choose_kind(n, nmissing, ntoggles):
    if nmissing == 0:
        return KIND_NONE
    nw = (n + 63) // 64
    if n <= 2 ** 32 and 4 * ntoggles < 8 * nw:
        return KIND_TOGGLES
    return KIND_BITS


def max_size(n):
    return HEADER_BYTES + 8 * ((n + 63) // 64)


def stream(miss):
    """the bytes of the mask stream of a bool array"""
    b = np.asarray(miss).reshape(-1)
    n, nmissing = b.size, int(b.sum())
    t = toggles(b)
    kind = choose_kind(n, nmissing, t.size)
    if kind == KIND_NONE:
        count, payload = 0, b""
    elif kind == KIND_TOGGLES:
        count, payload = t.size, t.astype("<u4").tobytes()
    else:
        w = words(b)
        count, payload = w.size, w.tobytes()
    return b"SPMK" + bytes([1, kind, 0, 0]) + struct.pack("<QQQ", n, nmissing, count) + payload


def parse(s):
    """(kind, n, nmissing, count) of a stream's header"""
    assert s[:4] == b"SPMK" and s[4] == 1 and s[6:8] == b"\0\0"
    return (s[5],) + struct.unpack("<QQQ", s[8:32])


def bits_of_stream(s):
    """the bool array a stream describes"""
    kind, n, _, count = parse(s)
    if kind == KIND_NONE:
        return np.zeros(n, dtype=bool)
    if kind == KIND_BITS:
        w = np.frombuffer(s[32:], dtype="<u8")
        assert w.size == count
        return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)
    t = np.frombuffer(s[32:], dtype="<u4").astype(np.int64)
    assert t.size == count
    flips = np.zeros(n + 1, dtype=np.int64)
    np.add.at(flips, t, 1)
    return (np.cumsum(flips[:n]) % 2).astype(bool)


# ---- the masks of the issue's table, on a (z, y, x) grid -------------------------------------------------------------
def ball_mask(shape_zyx, radius):
    dz, dy, dx = shape_zyx
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    return (z - dz / 2) ** 2 + (y - dy / 2) ** 2 + (x - dx / 2) ** 2 <= radius * radius


def slab_mask(shape_zyx, x_from):
    m = np.zeros(shape_zyx, dtype=bool)
    m[:, :, x_from:] = True
    return m


def density_mask(shape_zyx, density, seed):
    return np.random.default_rng(seed).random(shape_zyx) < density
