"""The time-series rule of sperr_amd/csrc/series.h, stated again in numpy: the plan, the band order, the needs, the two
butterflies, the tolerances and the info record.  Every figure is compared bit for bit with the header (test_series_host)
and with the device (test_gpu_series)."""
import struct

import numpy as np

S = float.fromhex("0x1.6a09e667f3bcdp-1")
MAX_LEVELS = 4
ROUND_K = (0.0, 13.0, 28.0, 46.0, 67.0)
INFO_BYTES = 64


def plan(n, levels):
    """[(start, l)]: consecutive groups of 2^levels, the remainder cut by its binary digits, largest first"""
    assert n >= 1 and 0 <= levels <= MAX_LEVELS
    g = 1 << levels
    out = [(i * g, levels) for i in range(n // g)]
    at = n // g * g
    for b in range(levels - 1, -1, -1):
        if (n >> b) & 1:
            out.append((at, b))
            at += 1 << b
    return out


def slot_cover(l, slot):
    """steps of its group, relative to the group's start, that a slot covers"""
    if slot == 0:
        return 0, 1 << l
    k = l - (slot.bit_length() - 1)
    j = slot - (1 << (l - k))
    return j << k, (j + 1) << k


def needs(n, levels, t0, nt):
    """the sorted band indices a decode of [t0, t0 + nt) needs"""
    assert 0 <= t0 < n and 1 <= nt <= n - t0
    out = []
    for start, l in plan(n, levels):
        for slot in range(1 << l):
            lo, hi = slot_cover(l, slot)
            if start + lo < t0 + nt and t0 < start + hi:
                out.append(start + slot)
    return out


def forward_group(steps):
    """steps: (g, ...) of one group, any float dtype -> bands (g, ...) float64 in slot order"""
    v = np.asarray(steps).astype(np.float64)
    g = v.shape[0]
    length = g
    while length > 1:
        e, o = v[0:length:2].copy(), v[1:length:2].copy()
        v[: length // 2] = (e + o) * S
        v[length // 2: length] = (e - o) * S
        length //= 2
    return v


def inverse_group(bands):
    """bands: (g, ...) float64 in slot order -> steps (g, ...) float64"""
    v = np.array(bands, dtype=np.float64)
    g = v.shape[0]
    length = 2
    while length <= g:
        a, d = v[: length // 2].copy(), v[length // 2: length].copy()
        v[0:length:2] = (a + d) * S
        v[1:length:2] = (a - d) * S
        length *= 2
    return v


def forward(steps, levels):
    """steps: (N, ...) -> bands (N, ...) float64"""
    steps = np.asarray(steps)
    out = np.empty(steps.shape, np.float64)
    for start, l in plan(steps.shape[0], levels):
        out[start:start + (1 << l)] = forward_group(steps[start:start + (1 << l)])
    return out


def inverse(bands, levels, t0=0, nt=None, present=None, out_dtype=np.float64):
    """bands: (N, ...) float64; bands outside `present` (default: the needs of the range) count as zero"""
    bands = np.asarray(bands, np.float64)
    n = bands.shape[0]
    nt = n - t0 if nt is None else nt
    need = set(needs(n, levels, t0, nt) if present is None else present)
    b = bands.copy()
    for i in range(n):
        if i not in need:
            b[i] = 0.0
    steps = np.empty_like(b)
    for start, l in plan(n, levels):
        steps[start:start + (1 << l)] = inverse_group(b[start:start + (1 << l)])
    return steps[t0:t0 + nt].astype(out_dtype)


def gain(l):
    a = 1.0
    for _ in range(l):
        a = S * (a + 1.0)
    return a


def tolerance(tol, M, levels):
    """(rho, [tau_0 .. tau_levels]) or None where the call refuses"""
    if not (0 <= levels <= MAX_LEVELS) or not (tol > 0.0) or not np.isfinite(tol) or not (M >= 0.0) or not np.isfinite(M):
        return None
    rho = ROUND_K[levels] * 2.0 ** -53 * (M if M > tol else tol)
    if not (rho < tol / 2.0):
        return None
    return rho, [(tol - rho) / gain(l) for l in range(levels + 1)]


def band_tolerances(n, levels, tol, M):
    """tau of every band of the series"""
    rho, tau = tolerance(tol, M, levels)
    out = np.empty(n)
    for start, l in plan(n, levels):
        out[start:start + (1 << l)] = tau[l]
    return out


def write_info(n, levels, dims_xyz, is_float, kind, quality, rng, M, rho):
    return (b"SPTS" + bytes([1, levels, 1 if is_float else 0, kind]) + struct.pack("<4I", n, *dims_xyz) +
            struct.pack("<4d", quality, rng, M, rho) + bytes(8))


def parse_info(rec):
    rec = bytes(rec)
    assert len(rec) == INFO_BYTES and rec[:4] == b"SPTS" and rec[4] == 1
    n, dx, dy, dz = struct.unpack("<4I", rec[8:24])
    quality, rng, M, rho = struct.unpack("<4d", rec[24:56])
    return dict(n=n, levels=rec[5], is_float=rec[6], kind=rec[7], dims=(dx, dy, dz), quality=quality, range=rng, M=M,
                rho=rho)
