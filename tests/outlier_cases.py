"""The shared case table of the outlier coder (plain numpy, no GPU): the 1D SPECK coder of mode 3's outlier list,
beyond the one to three bit planes that containers of natural fields ever give it.

Three kinds of case, all built from the hash words of tests/fields.py and exact IEEE operations, so they are the same
on every machine (tests/golden/outlier_streams.npz depends on that):

  coder cases     (name, n, coef uint64[n], sign bool[n])   what the coder codes; True = non-negative
  encoder cases   (name, n, tol, err float64[n])            an error array; the outliers are where |err| > tol
  graft           an oracle mode-3 container with the outlier stream of chosen chunks replaced by one of the table's

A corrector is 1.1 tol for a magnitude of 1 and (m - 0.25) tol otherwise (src/Outlier_Coder.cpp:206-234)."""
import numpy as np

from fields import _hash_words, _pow2
from sperr_amd.farm import build_container, split_container

# Every n has a chunk shape (z, y, x) for the container tests.  The table starts at n = 3: a one-sample chunk is always
# constant and never has an outlier stream, and below three samples the reference's 1D coder is undefined --
# SPECK1D_INT::m_initialize_lists / m_code_S index m_LIS beyond its num_of_partitions + 1 lists
# (src/SPECK1D_INT.cpp:19-34, src/SPECK1D_INT_ENC.cpp:137-160), a write past a vector's end.  There is nothing to
# compare with there, so the oracle and the kernels are not compared below three samples either.
SHAPE_OF_N = {3: (1, 1, 3), 5: (1, 1, 5), 64: (4, 4, 4), 65: (1, 5, 13), 100: (4, 5, 5),
              4096: (16, 16, 16), 8190: (13, 21, 30), 32768: (32, 32, 32), 262144: (64, 64, 64)}
DENSE_MAX_N = 32768   # the coder is one wavefront per chunk: dense cases stay at or below this
GOLDEN_MAX_N = 8190   # the cases whose reference streams tests/golden/outlier_streams.npz records

_NS = {"first_last": (3, 5, 64, 65, 4096, 8190, 32768, 262144),
       "one_top": (3, 5, 65, 8190, 262144),
       "top_bit": (3, 64, 8190, 32768),
       "every_plane": (64, 65, 4096, 8190, 262144),
       "width_edges": (8190, 32768, 262144),
       "all_one": (3, 5, 64, 65, 4096, 8190, 32768),
       "dense_wide": (3, 5, 64, 65, 4096, 8190, 32768),
       "run": (4096, 8190, 32768, 262144),
       "single_one": (3, 64, 65, 4096, 8190, 262144)}
SPARSE = ("first_last", "one_top", "top_bit", "every_plane", "width_edges", "run", "single_one")
_U = np.uint64


GOLDEN_TOL = 2.0 ** -10


def golden_base(n):
    """float64[n] in [-2, 2): what the golden decodes add their correctors to"""
    return (_hash_words((n,), 83) >> _U(40)).astype(np.float64) * _pow2(-22) - 2.0


def coder_case(name, n):
    """(coef uint64[n], sign bool[n]) of the named case at length n"""
    h = _hash_words((n,), 41)
    coef = np.zeros(n, dtype=np.uint64)
    sign = (_hash_words((n,), 43) >> _U(63)).astype(bool)
    if name == "first_last":
        coef[0] = 1
        coef[n - 1] = (1 << 40) + 5
    elif name == "one_top":        # 63 planes
        coef[n // 2] = 1 << 62
    elif name == "top_bit":        # 64 planes, the most a stream can name
        coef[n // 2] = 1 << 63
    elif name == "every_plane":    # one value 2^p for each p in 0..62 at hashed positions
        coef[np.argsort(h, kind="stable")[:63]] = _U(1) << np.arange(63, dtype=np.uint64)
    elif name == "width_edges":    # the word boundaries of the position masks and of the integer widths
        for p, m in zip((63, 64, 127, 128, 4095, 4096), (3, 255, 256, 65535, 65536, 1 << 32)):
            if p < n:   # (a 37 x 50 slice takes the first four)
                coef[p] = m
    elif name == "all_one":
        coef[:] = 1
    elif name == "dense_wide":     # every position, 20 hashed bits
        coef = np.maximum(h >> _U(44), _U(1))
    elif name == "run":            # 200 consecutive positions from an odd start, 1 to 22 bits, alternating signs
        lo = (n // 3) | 1
        coef[lo:lo + 200] = (h[lo:lo + 200] >> (_U(42) + h[lo:lo + 200] % _U(22))) | _U(1)
        sign = (np.arange(n) & 1).astype(bool)
    elif name == "single_one":
        coef[(2 * n) // 3] = 1
    else:
        raise KeyError(name)
    return np.ascontiguousarray(coef), sign


def coder_cases(max_n=None, names=None):
    """[(name, n)] of the table, optionally up to a length / of some names"""
    return [(name, n) for name, ns in _NS.items() if names is None or name in names
            for n in ns if max_n is None or n <= max_n]


def planes_of(stream):
    """the planes byte of an outlier stream"""
    return stream[0]


def corrector(coef, sign, tol):
    """float64[n]: what the decoder adds (src/Outlier_Coder.cpp:206-234), from the magnitudes in plain numpy"""
    c = np.where(coef == 1, 1.1, coef.astype(np.float64) - 0.25)
    return np.where(coef == 0, 0.0, c * tol * np.where(sign, 1.0, -1.0))


# ---- encoder cases: error arrays --------------------------------------------------------------------------------

def errors_of(coef, sign, tol):
    """float64[n] whose outliers quantise to (coef, sign) where no width wrap intervenes: m tol, and 1.25 tol for
    m = 1 (an error of exactly tol is no outlier); exact for a power-of-two tol"""
    units = np.where(coef == 1, 1.25, coef.astype(np.float64))
    return units * tol * np.where(sign, 1.0, -1.0)


def _hashed(n, count, seed):
    """`count` distinct hashed positions below n, ascending"""
    return np.sort(np.argsort(_hash_words((n,), seed), kind="stable")[:count])


def _signed(n, seed):
    return np.where(_hash_words((n,), seed) >> _U(63), 1.0, -1.0)


def encoder_cases():
    """[(name, n, tol, err float64[n])].  The tolerances are powers of two, so every err is exact.  The integer width
    comes from llrint of the largest |err| itself, the magnitudes from err / tol (src/Outlier_Coder.cpp:82-100,188-203):
    with a small tolerance the magnitudes outgrow the width and wrap."""
    out = []

    def add(name, n, tol, pos, units, seed=47):
        err = np.zeros(n)
        err[pos] = np.asarray(units, dtype=np.float64) * tol * _signed(n, seed)[pos]
        out.append((name, n, float(tol), err))

    h = _hash_words((8190,), 53)
    # |err| <= 1 -> uint8, err / tol up to 2^20: most magnitudes wrap
    pos = _hashed(4096, 300, 59)
    add("wrap8", 4096, _pow2(-20), pos, np.maximum(h[:300] >> _U(44), _U(2)))
    # |err| < 2^15 -> uint16, err / tol up to 2^35
    pos = _hashed(8190, 500, 61)
    m = np.maximum(h[:500] >> _U(29), _U(2))
    m[0] = 300 << 20   # (the largest |err| is above 255 whatever the hash gives)
    add("wrap16", 8190, _pow2(-20), pos, m)
    # |err| < 2^30 -> uint32, err / tol up to 2^50
    pos = _hashed(4096, 200, 67)
    m = np.maximum(h[:200] >> _U(14), _U(2))
    m[0] = 70000 << 20
    add("wrap32", 4096, _pow2(-20), pos, m)
    # uint64: nothing wraps, 63 planes
    add("wide64", 65, 1.0, [3, 64], [1 << 62, (1 << 33) + 1])
    # some magnitudes are multiples of 256 under uint8 and wrap to zero: they are no coefficients
    pos = _hashed(8190, 400, 71)
    m = np.maximum(h[:400] >> _U(47), _U(2))   # 17 bits, |err| < 128
    m[::3] &= ~_U(255)
    m[::3] = np.maximum(m[::3], _U(256))
    add("some_wrap_to_zero", 8190, _pow2(-10), pos, m)
    # all of them do: the stream is {0 planes, 0 bits}
    pos = _hashed(4096, 50, 73)
    add("all_wrap_to_zero", 4096, _pow2(-10), pos, (np.arange(50) + 1) * 256)
    # ties of llrint: err / tol = m + 0.5 for even and odd m, both signs (round half to even)
    err = np.zeros(64)
    err[3:3 + 16] = (np.repeat(np.arange(1, 9), 2) + 0.5) * _pow2(-4) * np.tile([1.0, -1.0], 8)
    out.append(("ties", 64, float(_pow2(-4)), err))
    # |err| = tol exactly is no outlier, the next double is one
    tol = _pow2(-3)
    err = np.zeros(65)
    err[[0, 7, 63]] = [tol, -tol, tol]
    err[[1, 8, 64]] = [np.nextafter(tol, np.inf), -np.nextafter(tol, np.inf), np.nextafter(tol, np.inf)]
    err[30] = 2.0 * tol
    out.append(("tolerance_boundary", 65, float(tol), err))
    # the issue's example (its tolerance is no power of two: the errors are given, not built): 3.0 / 0.001 = 3000
    # under uint8 is 184, and 0.5 / 0.001 = 500 is 244
    err = np.zeros(100)
    err[5], err[17] = 3.0, -0.5
    out.append(("wrap_example", 100, 0.001, err))
    return out


REFUSED_ENCODER_CASE = ("raw_error_2p63", 64, 1.0, 9, 2.0 ** 63)   # (name, n, tol, position, error): refused, code 7


def outlier_list(err, tol):
    """(pos uint64[k], err float64[k]): the samples beyond the tolerance, ascending"""
    pos = np.nonzero(np.abs(err) > tol)[0]
    return pos.astype(np.uint64), np.ascontiguousarray(err[pos])


def recon_and_orig(err, tol, dtype=np.float64):
    """(recon float64[n], orig dtype[n]) with orig.astype(float64) - recon == err exactly: recon is a hashed multiple
    of tol below 512 tol in magnitude where the sum is exact in dtype, and 0 elsewhere"""
    k = (_hash_words(err.shape, 79) >> _U(54)).astype(np.float64) - 512.0
    recon = k * tol
    orig = (recon + err).astype(dtype)
    bad = orig.astype(np.float64) - recon != err
    recon[bad] = 0.0
    orig = (recon + err).astype(dtype)
    assert np.array_equal(orig.astype(np.float64) - recon, err), "the errors are not exact in this type"
    return recon, orig


# ---- grafting a stream into a container --------------------------------------------------------------------------

def outlier_start(chunk):
    """where the outlier stream of a chunk's stream starts (the bytes behind its SPECK stream), or None:
    {17 bytes of conditioner header, u8 planes, u64 total_bits, payload} (src/SPECK_FLT.cpp:88-103)"""
    if len(chunk) < 26 or chunk[0] & 0x01:
        return None
    tb = int(np.frombuffer(chunk, dtype=np.uint64, count=1, offset=18)[0])
    speck = min(9 + (tb + 7) // 8, len(chunk) - 17)
    return 17 + speck if 17 + speck + 9 <= len(chunk) else None


def speck_end(chunk):
    """the end of a whole chunk stream's SPECK stream; the chunk is not constant"""
    assert len(chunk) >= 26 and not chunk[0] & 0x01
    tb = int(np.frombuffer(chunk, dtype=np.uint64, count=1, offset=18)[0])
    end = 17 + 9 + (tb + 7) // 8
    assert end <= len(chunk), "the SPECK stream is cut"
    return end


def graft(container, streams):
    """container: an oracle mode-3 container; streams: {chunk index: outlier stream (b"" for none)}.  Each chosen
    chunk is cut at the end of its SPECK stream and the given stream appended; the other chunks stay."""
    flags, vol, cd, parts = split_container(container)
    parts = list(parts)
    for i, s in streams.items():
        parts[i] = bytes(parts[i][:speck_end(parts[i])]) + bytes(s)
    return build_container(parts, vol, cd, bool(flags & 0x20), bool(flags & 0x80))


def graft_2d(stream, outlier_stream):
    """the same for a headerless 2D stream, which is one chunk stream"""
    return bytes(stream[:speck_end(stream)]) + bytes(outlier_stream)
