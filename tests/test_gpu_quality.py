"""GPU: SperrHip.quality / quality_batch against tests/golden/quality_ref.json, the reference's own calc_stats<T> /
calc_mean_var<T> on the same inputs (tests/quality_cases.py).  mse, rmse, linfty, mean and var bit for bit; min and
max by value; psnr within 8 ulp of T -- everything feeding the logarithm is pinned exactly, two libm log10s each
within 2 ulp of the true value may differ by 4, and the multiply by 10 rounds once more."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_cases as qc   # noqa: E402

pytestmark = pytest.mark.gpu
BITWISE = ("mse", "rmse", "linfty", "mean", "var")


@pytest.fixture(scope="module")
def eng():
    from sperr_amd.api import SperrHip
    return SperrHip()


@pytest.fixture(scope="module")
def fx():
    return qc.load_fixture()


def check(q, rec, what=""):
    dt = qc.DTYPES[rec["dtype"]]
    print(what, rec["dtype"], rec["n"], {f: (getattr(q, f), float(qc.from_hex(rec[f], dt))) for f in qc.FIGURES})
    for f in BITWISE:
        assert qc.to_hex(dt(getattr(q, f))) == format(int(rec[f], 16), "x"), (what, f)
    for f in ("min", "max"):
        assert dt(getattr(q, f)) == qc.from_hex(rec[f], dt), (what, f)
    assert qc.ulp_distance(dt(q.psnr), qc.from_hex(rec["psnr"], dt), dt) <= 8, (what, "psnr")


def same_bits(q1, q2):
    return all(np.float64(getattr(q1, f)).tobytes() == np.float64(getattr(q2, f)).tobytes() for f in qc.FIGURES)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("key", ["f32", "f64"])
@pytest.mark.parametrize("n", qc.SIZES)
def test_sizes(eng, fx, n, key):
    """block edges of both block lengths; 57349: three blocks of 16384, one more of 8192, a tail of 5; 2^24 + 8197:
    1025 row sums, more than the 1024 the final sum stages per round, and 65 workgroups of 16 rows"""
    name = f"size_{n}_{key}"
    a, b = qc.cases()[name]()
    check(eng.quality(dev(a), dev(b)), fx[name], name)


@pytest.mark.parametrize("key", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["identical", "diff_first", "diff_last", "diff_tail_first", "const_a"])
def test_special_arrays(eng, fx, kind, key):
    name = f"{kind}_{key}"
    a, b = qc.cases()[name]()
    q = eng.quality(dev(a), dev(b))
    check(q, fx[name], name)
    if kind == "identical":
        assert q.psnr == np.inf and q.rmse == 0.0 and q.linfty == 0.0
    elif kind == "const_a":
        assert q.max == q.min and q.psnr == -np.inf
    else:
        assert q.rmse > 0.0 and 0.12 < q.linfty < 0.13


def test_subnormal_squares_are_kept(eng, fx):
    a, b = qc.subnormal()
    q = eng.quality(dev(a), dev(b))
    assert 0.0 < q.mse < 1.2e-38 and np.isfinite(q.psnr)      # a kernel that flushes gives 0 and +inf
    check(q, fx["subnormal_f32"], "subnormal")


@pytest.mark.parametrize("key", ["f32", "f64"])
@pytest.mark.parametrize("off_a,off_b", [(1, 0), (0, 1), (1, 1), (3, 2)])
def test_misaligned_bases(eng, fx, off_a, off_b, key):
    """views that start one (or more) elements into their buffers: the figures are those of the aligned run"""
    name = f"size_57349_{key}"
    a, b = qc.cases()[name]()
    da = torch.empty(a.size + 8, dtype=dev(a[:1]).dtype, device="cuda")
    db = torch.empty_like(da)
    va, vb = da[off_a:off_a + a.size], db[off_b:off_b + b.size]
    va.copy_(torch.from_numpy(a))
    vb.copy_(torch.from_numpy(b))
    assert va.data_ptr() % 16 == (off_a * a.itemsize) % 16 and vb.data_ptr() % 16 == (off_b * a.itemsize) % 16
    check(eng.quality(va, vb), fx[name], f"{name} +{off_a}/+{off_b}")


@pytest.mark.parametrize("key", ["f32", "f64"])
def test_batch_of_odd_volumes(eng, fx, key):
    """three volumes of 24579 values: slices 1 and 2 start off a 16-byte boundary; bit for bit the single calls"""
    a, b = qc.batch(3, qc.N_BATCH3, qc.DTYPES[key], 31)
    da, db = dev(a), dev(b)
    qs = eng.quality_batch(da, db)
    assert len(qs) == 3
    for v, q in enumerate(qs):
        check(q, fx[f"batch3_v{v}_{key}"], f"batch3 v{v}")
        assert same_bits(q, eng.quality(da[v], db[v]))


def test_batch_of_64_cubes(eng, fx):
    a, b = qc.batch(64, 32 ** 3, np.float32, 64)
    da, db = dev(a.reshape(64, 32, 32, 32)), dev(b.reshape(64, 32, 32, 32))
    qs = eng.quality_batch(da, db)
    assert len(qs) == 64
    for v in (0, 63):
        check(qs[v], fx[f"batch64_v{v}_f32"], f"batch64 v{v}")
    for v in range(64):
        assert same_bits(qs[v], eng.quality(da[v], db[v])), v


@pytest.mark.parametrize("name", sorted(qc.GOLDEN_PAIRS))
def test_golden_decodes(eng, fx, name):
    tag, inp, shape = qc.GOLDEN_PAIRS[name]
    a = np.fromfile(os.path.join(qc.GOLDEN, inp + ".f32"), dtype=np.float32).reshape(shape)
    stream = np.fromfile(os.path.join(qc.GOLDEN, tag + ".sperr"), dtype=np.uint8)
    da = dev(a)
    check(eng.quality(da, eng.decompress(dev(stream), output_float=True)), fx[name + "_f32"], name)


def test_end_to_end_smoke_volume(eng, fx):
    """compress -> decompress -> quality with nothing copied to the host in between"""
    vol = dev(qc.smoke_volume())
    stream = eng.compress(vol, qc.SMOKE_CHUNKS, 2.0)
    q = eng.quality(vol, eng.decompress(stream, output_float=True), nbytes=stream.numel())
    check(q, fx["smoke_bpp2_f32"], "smoke 2 bpp")
    assert q.sigma == float(np.sqrt(np.float64(q.var)))
    assert q.bitrate == 8.0 * stream.numel() / vol.numel()
    assert q.accuracy_gain == float(np.log2(np.float64(q.sigma) / np.float64(q.rmse))) - q.bitrate
    assert eng.quality(vol, vol).accuracy_gain is None
    pwe = eng.compress(vol, qc.SMOKE_CHUNKS, 1e-3, mode=3)
    qp = eng.quality(vol, eng.decompress(pwe, output_float=True), nbytes=pwe.numel())
    print("PWE 1e-3: linfty", qp.linfty, "psnr", qp.psnr, "gain", qp.accuracy_gain)
    assert 0.0 < qp.linfty <= 1e-3


def test_refusals_launch_nothing(eng):
    a = torch.ones(64, dtype=torch.float32, device="cuda")
    lib, p = eng.lib, a.data_ptr()
    eng.profile(True)
    for call in (lambda o: lib.sperrhip_quality_dev(p, p, 1, 0, o, None),
                 lambda o: lib.sperrhip_quality_dev(None, p, 1, 64, o, None),
                 lambda o: lib.sperrhip_quality_dev(p, None, 1, 64, o, None),
                 lambda o: lib.sperrhip_quality_batch_dev(p, p, 1, 0, 64, o, None),
                 lambda o: lib.sperrhip_quality_batch_dev(p, p, 1, 4, 0, o, None)):
        out = (ctypes.c_double * 32)(*([7.5] * 32))
        assert call(out) == -1
        assert list(out) == [7.5] * 32
    assert lib.sperrhip_quality_dev(p, p, 1, 64, None, None) == -1
    assert eng.profile_report() == {}
    eng.quality(a, a)                                    # ... and a call that is taken does launch
    rep = eng.profile_report()
    eng.profile(False)
    assert sum(cnt for _, cnt in rep.values()) == 3, rep
