"""Inputs and a numpy model of the quality figures (sperr::calc_stats / calc_mean_var), shared by the fixture's
generator (tests/golden/make_quality_ref.py) and the tests that compare against tests/golden/quality_ref.json.

Every case is a pair (a, b) of one dtype: a the original, b the reconstruction.  Inputs are deterministic: seeded
numpy generators, or committed volumes against the oracle's decode of a committed or freshly coded container.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURE = os.path.join(GOLDEN, "quality_ref.json")
FIGURES = ("rmse", "linfty", "psnr", "min", "max", "mean", "var", "mse")
DTYPES = {"f32": np.float32, "f64": np.float64}
SIZES = (1, 8191, 8192, 8193, 16384, 16385, 57349, (1 << 24) + 8197)
N_SPECIAL = 24581          # three blocks of 8192 and a tail of 5: one block of 16384 and a tail of 8197
N_BATCH3 = 24579           # odd: slices 1 and 2 of a batch start off a 16-byte boundary
SMOKE_SHAPE, SMOKE_CHUNKS = (40, 48, 56), (32, 32, 32)


def field(n, dt, seed):
    """a seeded normal field and a copy with errors of mixed magnitude: another order of summation changes the bits"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(n) * 3.0 + 1.5).astype(dt)
    err = rng.standard_normal(n) * 10.0 ** rng.uniform(-6.0, -1.0, n)
    return a, (a.astype(np.float64) + err).astype(dt)


def _special(kind, dt):
    a, _ = field(N_SPECIAL, dt, 77)
    b = a.copy()
    if kind == "identical":
        return a, b
    if kind == "const_a":
        a = np.full(N_SPECIAL, 2.5, dt)
        b = a.copy()
        b[12345] = 2.25
        return a, b
    at = {"diff_first": 0, "diff_last": N_SPECIAL - 1, "diff_tail_first": N_SPECIAL - N_SPECIAL % 8192}[kind]
    b[at] += dt(0.125)
    return a, b


def subnormal():
    """every square of a difference is a subnormal float; the reference's mse is about 1.005e-42"""
    n = 8492
    rng = np.random.default_rng(5)
    a = np.zeros(n, np.float32)
    a[5] = np.float32(1e-10)
    e = (rng.uniform(0.5, 1.5, n) * 1e-21 * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return a, a + e


def batch(nvol, n, dt, seed):
    a, b = field(nvol * n, dt, seed)
    return a.reshape(nvol, n), b.reshape(nvol, n)


def smoke_volume():
    from sperr_amd.synth import turbulence
    return turbulence(SMOKE_SHAPE)


def golden_pair(oracle, tag, inp, shape_zyx):
    """a committed volume against the oracle's decode of a committed container of it"""
    a = np.fromfile(os.path.join(GOLDEN, inp + ".f32"), dtype=np.float32)
    with open(os.path.join(GOLDEN, tag + ".sperr"), "rb") as f:
        b = oracle.decomp_3d(f.read(), True)
    assert b.shape == tuple(shape_zyx) and a.size == b.size
    return a, np.ascontiguousarray(b).reshape(-1)


GOLDEN_PAIRS = {"wmag17_bpp2": ("wmag17_c17x17x17_bpp2.0", "wmag17", (17, 17, 17)),
                "vort_crop_bpp2": ("vort_crop_c20x18x16_bpp2.0", "vort_crop", (33, 36, 40))}


def cases(oracle=None, big=True):
    """name -> (a, b), lazily: a dict of callables"""
    out = {}
    for key, dt in DTYPES.items():
        for n in SIZES:
            if big or n < (1 << 20):
                out[f"size_{n}_{key}"] = (lambda n=n, dt=dt: field(n, dt, 1000 + n % 9973))
        for kind in ("identical", "diff_first", "diff_last", "diff_tail_first", "const_a"):
            out[f"{kind}_{key}"] = (lambda kind=kind, dt=dt: _special(kind, dt))
        for v in range(3):
            out[f"batch3_v{v}_{key}"] = (lambda v=v, dt=dt: tuple(x[v] for x in batch(3, N_BATCH3, dt, 31)))
    for v in (0, 63):
        out[f"batch64_v{v}_f32"] = (lambda v=v: tuple(x[v] for x in batch(64, 32 ** 3, np.float32, 64)))
    out["subnormal_f32"] = subnormal
    if oracle is not None:
        for name, (tag, inp, shape) in GOLDEN_PAIRS.items():
            out[name + "_f32"] = (lambda tag=tag, inp=inp, shape=shape: golden_pair(oracle, tag, inp, shape))

        def smoke():
            vol = smoke_volume()
            back = oracle.decomp_3d(oracle.comp_3d(vol, SMOKE_CHUNKS, 1, 2.0), True)
            return vol.reshape(-1), np.ascontiguousarray(back).reshape(-1)
        out["smoke_bpp2_f32"] = smoke
    return out


# ---- the numpy model: sequential sums per block, then over the block sums, everything in T ---------------------
def _seq(x):
    return np.cumsum(x, dtype=x.dtype)[-1] if x.size else x.dtype.type(0)


def blocked_sum(x, block):
    nb = x.size // block
    sums = np.cumsum(x[:nb * block].reshape(nb, block), axis=1, dtype=x.dtype)[:, -1] if nb else np.empty(0, x.dtype)
    return _seq(np.concatenate([sums, [_seq(x[nb * block:])]]).astype(x.dtype))


def model(a, b):
    """the eight figures as values of the arrays' dtype (psnr through numpy's log10: within a few ulp of libm's)"""
    T = a.dtype.type
    n = T(a.size)
    mean = T(blocked_sum(a, 16384) / n)
    c = a - mean
    var = T(blocked_sum(c * c, 16384) / n)
    lo, hi = a.min(), a.max()
    if np.array_equal(a, b):
        return dict(rmse=T(0), linfty=T(0), psnr=T(np.inf), min=lo, max=hi, mean=mean, var=var, mse=T(0))
    d = np.abs(a - b)
    mse = T(blocked_sum(d * d, 8192) / n)
    with np.errstate(divide="ignore"):
        psnr = T(np.log10(T((hi - lo) * (hi - lo)) / mse) * T(10))
    return dict(rmse=np.sqrt(mse), linfty=d.max(), psnr=psnr, min=lo, max=hi, mean=mean, var=var, mse=mse)


# ---- bit patterns ------------------------------------------------------------------------------------------------
def to_hex(v):
    v = np.asarray(v)
    return format(int(v.view(np.uint32 if v.dtype == np.float32 else np.uint64)), "x")


def from_hex(h, dt):
    ut = np.uint32 if dt == np.float32 else np.uint64
    return np.array(int(h, 16), dtype=ut).view(dt)[()]


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def ulp_distance(x, y, dt):
    """how many representable values of dt lie between x and y (0: the same value; equal infinities: 0)"""
    it = np.int32 if dt == np.float32 else np.int64
    def key(v):
        i = int(np.array(v, dtype=dt).view(it))
        return i if i >= 0 else -(i & (2 ** (31 if dt == np.float32 else 63) - 1))
    return abs(key(x) - key(y))
