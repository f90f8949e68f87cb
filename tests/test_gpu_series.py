"""GPU (-m gpu): time series (series.h) -- the two kernels alone and the two calls.  The yardsticks
are tests/series_model.py and the CPU oracle; every compare is on bytes or bit patterns, and the one bound is the
call's own: every sample of a double decode within tol.

  forward    k_series_fwd against the model, bit for bit: fp32 and fp64; 17^3, 20 x 18 x 16 and 8 steps of 128^3 (the
             grid-stride loop runs more than once); N in {1, 2, 3, 5, 8, 11, 16, 21}, L in 0 .. 4; the steps cut from
             one allocation at odd element offsets, and aligned
  inverse    k_series_inv against the model on the same grid; every [t0, t0 + nt) of N = 11, L = 3 with a canary
             behind every output and in every step outside the range
  tol        wmag17 and vort_crop as a base plus drifting copies, fp32 and fp64, N = 11, L = 3, one chunk and ragged
             chunks: every band container is the oracle's comp_3d(model band, mode 3, tau); the double decode is the
             model's inverse of the oracle's decoded bands and within tol everywhere; the fp32 decode is that, narrowed
  psnr       the band containers' chunk streams are the oracle's at the series' range (test_gpu_psnr_vol's yardstick),
             once with range= given; a constant series; a series of identical steps (detail bands all zero)
  partial    every step range equals the slice of the whole decode; a box equals the crop; pct=50 equals the model's
             inverse of the bands decoded at 50; containers the range does not need may hold garbage
  refusals   everything the header lists; the outputs stay untouched
  children   SPERR_HIP_SERIES_MAX_MB so that N = 11 runs in three windows, with a split and poisoned workspace"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import series_model as sm
from test_gpu_psnr_vol import check_streams, est, oracle_chunks   # noqa: F401  (est is a fixture)
from test_gpu_size import bits, cuda, host

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    return SperrHip()


def torch_dtype(dtype):
    import torch
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def odd_steps(steps):
    """the steps of a numpy (N, ...) array as dense cuda views cut from ONE allocation at odd element offsets: none of
    them is 16-byte aligned, and their phases differ"""
    import torch
    n = steps[0].size
    pitch = n + 2 + (n % 2)                     # even, so that every step starts at an odd element
    buf = torch.zeros(1 + len(steps) * pitch, dtype=torch_dtype(steps.dtype), device="cuda")
    views = []
    for t, s in enumerate(steps):
        v = buf[1 + t * pitch: 1 + t * pitch + n].view(s.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(s)))
        assert v.data_ptr() % 16 != 0
        views.append(v)
    return views


SHAPES = {"17": (17, 17, 17), "20x18x16": (16, 18, 20)}   # (z, y, x)
NSTEPS = (1, 2, 3, 5, 8, 11, 16, 21)


def noise(n, shape, dtype, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n,) + tuple(shape)) * 10.0 ** rng.uniform(-3, 3, (n,) + (1,) * len(shape))).astype(dtype)


# ---- a. the forward stage ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [False, True], ids=["odd", "aligned"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_forward_is_the_models(eng, shape, dtype, aligned):
    x = noise(max(NSTEPS), SHAPES[shape], dtype)
    for n in NSTEPS:
        d = cuda(x[:n]) if aligned else odd_steps(x[:n])
        for levels in range(5):
            got = eng.series_forward(d, levels).cpu().numpy()
            assert np.array_equal(bits(got), bits(sm.forward(x[:n], levels))), (n, levels)


def big(dtype):
    return cached(("big", np.dtype(dtype).name), lambda: noise(8, (128, 128, 128), dtype, seed=2))


@pytest.mark.parametrize("levels", range(5))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_forward_of_8_steps_of_128_cubed(eng, dtype, levels):
    x = big(dtype)
    d = cached(("bigdev", np.dtype(dtype).name), lambda: odd_steps(x))
    got = eng.series_forward(d, levels).cpu().numpy()
    assert np.array_equal(bits(got), bits(sm.forward(x, levels)))
    if levels == 3:
        got = eng.series_forward(cuda(x), levels).cpu().numpy()   # (aligned: the 16-byte loads)
        assert np.array_equal(bits(got), bits(sm.forward(x, levels)))


# ---- b. the inverse stage ---------------------------------------------------------------------------------------------

CANARY = -12345.5


def canary_outputs(nt, shape, out_dtype):
    """nt dense outputs at odd element offsets of one buffer filled with the canary"""
    import torch
    n = int(np.prod(shape))
    pitch = n + 2 + (n % 2)
    buf = torch.full((1 + nt * pitch + 7,), CANARY, dtype=torch_dtype(out_dtype), device="cuda")
    return buf, [buf[1 + t * pitch: 1 + t * pitch + n].view(shape) for t in range(nt)], pitch


def check_canary(buf, nt, n, pitch):
    h = buf.cpu().numpy()
    mask = np.ones(h.size, bool)
    for t in range(nt):
        mask[1 + t * pitch: 1 + t * pitch + n] = False
    assert np.all(h[mask] == CANARY)


@pytest.mark.parametrize("out_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_inverse_is_the_models(eng, shape, out_dtype):
    b = noise(max(NSTEPS), SHAPES[shape], np.float64, seed=3)
    n = b[0].size
    for ns in NSTEPS:
        d = cuda(b[:ns])
        for levels in range(5):
            buf, outs, pitch = canary_outputs(ns, SHAPES[shape], out_dtype)
            eng.series_inverse(d, levels, output_float=out_dtype == np.float32, out=outs)
            want = sm.inverse(b[:ns], levels, out_dtype=out_dtype)
            got = np.stack([o.cpu().numpy() for o in outs])
            assert np.array_equal(bits(got), bits(want)), (ns, levels)
            check_canary(buf, ns, n, pitch)


@pytest.mark.parametrize("out_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_inverse_of_every_step_range(eng, shape, out_dtype):
    import torch
    ns, levels = 11, 3
    b = noise(ns, SHAPES[shape], np.float64, seed=4)
    n = b[0].size
    for t0 in range(ns):
        for nt in range(1, ns - t0 + 1):
            # the bands the range does not need are NaNs: the kernel must not load them
            need = sm.needs(ns, levels, t0, nt)
            poisoned = b.copy()
            for k in range(ns):
                if k not in need:
                    poisoned[k] = np.nan
            buf, outs, pitch = canary_outputs(nt, SHAPES[shape], out_dtype)
            eng.series_inverse(cuda(poisoned), levels, t0=t0, nt=nt, output_float=out_dtype == np.float32, out=outs)
            want = sm.inverse(b, levels, t0, nt, out_dtype=out_dtype)
            got = np.stack([o.cpu().numpy() for o in outs])
            assert np.array_equal(bits(got), bits(want)), (t0, nt)
            check_canary(buf, nt, n, pitch)
    torch.cuda.synchronize()


@pytest.mark.parametrize("out_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_inverse_of_8_steps_of_128_cubed(eng, out_dtype):
    b = big(np.float64)
    for t0, nt in ((0, 8), (5, 2)):
        got = eng.series_inverse(cuda(b), 3, t0=t0, nt=nt, output_float=out_dtype == np.float32).cpu().numpy()
        assert np.array_equal(bits(got), bits(sm.inverse(b, 3, t0, nt, out_dtype=out_dtype)))


# ---- c. the series the calls are tested on ------------------------------------------------------------------------------

def base_of(data):
    if data == "wmag17":
        return np.fromfile(os.path.join(GOLD, "wmag17.f32"), dtype=np.float32).reshape(17, 17, 17)
    return np.fromfile(os.path.join(GOLD, "vort_crop.f32"), dtype=np.float32).reshape(33, 36, 40)


def series_of(data, dtype, n=11, drift=0.25):
    """a base plus drifting copies: step t is the base moved by drift * t samples along x (linear interpolation, periodic)"""
    def make():
        base = base_of(data).astype(np.float64)
        steps = []
        for t in range(n):
            s = drift * t
            k, a = int(np.floor(s)), s - np.floor(s)
            steps.append(((1 - a) * np.roll(base, k, axis=2) + a * np.roll(base, k + 1, axis=2)).astype(dtype))
        return np.stack(steps)
    return cached(("series", data, np.dtype(dtype).name, n, drift), make)


CHUNKINGS = {"wmag17": {"one": (17, 17, 17), "ragged": (10, 8, 6)}, "vort_crop": {"one": (40, 36, 33), "ragged": (16, 10, 8)}}
TOL_CASES = [(d, t, c) for d in ("wmag17", "vort_crop") for t in ("f32", "f64") for c in ("one", "ragged")]


def tol_case(eng, oracle, data, tname, chunking):
    """(steps, tol, containers as bytes, info, the oracle's decoded bands) of a tol-mode compression, made once"""
    def make():
        dtype = np.float32 if tname == "f32" else np.float64
        steps = series_of(data, dtype)
        tol = 1e-3 * (float(steps.max()) - float(steps.min()))
        conts, info = eng.compress_series(odd_steps(steps), CHUNKINGS[data][chunking], tol=tol, levels=3)
        conts = [host(c) for c in conts]
        decoded = np.stack([oracle.decomp_3d(c, False) for c in conts])
        return steps, tol, conts, info, decoded
    return cached(("tolcase", data, tname, chunking), make)


@pytest.mark.parametrize("data,tname,chunking", TOL_CASES, ids=["%s-%s-%s" % c for c in TOL_CASES])
def test_tol_mode_containers_are_the_oracles(eng, oracle, data, tname, chunking):
    steps, tol, conts, info, _ = tol_case(eng, oracle, data, tname, chunking)
    M = float(np.abs(steps.astype(np.float64)).max())
    rho, _ = sm.tolerance(tol, M, 3)
    rng = float(steps.max()) - float(steps.min())
    assert info == sm.write_info(11, 3, steps.shape[:0:-1], tname == "f32", 0, tol, rng, M, rho)
    bands = sm.forward(steps, 3)
    taus = sm.band_tolerances(11, 3, tol, M)
    for b in range(11):
        want = oracle.comp_3d(np.ascontiguousarray(bands[b]), CHUNKINGS[data][chunking], 3, float(taus[b]))
        assert conts[b] == want, b


@pytest.mark.parametrize("data,tname,chunking", TOL_CASES, ids=["%s-%s-%s" % c for c in TOL_CASES])
def test_tol_mode_decode_is_the_models_and_within_tol(eng, oracle, data, tname, chunking):
    steps, tol, conts, info, decoded = tol_case(eng, oracle, data, tname, chunking)
    dc = [cuda(np.frombuffer(c, dtype=np.uint8)) for c in conts]
    want = sm.inverse(decoded, 3)
    got = eng.decompress_series(dc, info, output_float=False).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    worst = float(np.abs(got - steps.astype(np.float64)).max())
    print("%s %s %s: worst error %.6f tol, %d bytes" % (data, tname, chunking, worst / tol, sum(len(c) for c in conts)))
    assert worst <= tol
    got32 = eng.decompress_series(dc, info, output_float=True).cpu().numpy()
    assert np.array_equal(bits(got32), bits(want.astype(np.float32)))


def test_levels_zero_is_the_plain_batch(eng):
    steps = series_of("wmag17", np.float32, n=5)
    conts, info = eng.compress_series(cuda(steps), (17, 17, 17), tol=1e-3, levels=0)
    plain = eng.compress_batch(cuda(steps.astype(np.float64)), (17, 17, 17), 1e-3, mode=3)
    assert [host(c) for c in conts] == [host(c) for c in plain]
    assert sm.parse_info(info)["rho"] == 0.0


# ---- d. PSNR mode ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("given", [False, True], ids=["own", "range="])
@pytest.mark.parametrize("tname", ["f32", "f64"])
def test_psnr_mode_streams_are_the_oracles(eng, oracle, est, tname, given):
    dtype = np.float32 if tname == "f32" else np.float64
    steps = series_of("vort_crop", dtype, n=5)
    chunks, psnr, levels = (20, 18, 16), 70.0, 2
    own = float(steps.max()) - float(steps.min())
    rng = 2.0 * own if given else own
    conts, info = eng.compress_series(odd_steps(steps), chunks, psnr=psnr, levels=levels, range=rng if given else None)
    h = sm.parse_info(info)
    assert (h["kind"], h["quality"], h["range"], h["rho"], h["levels"]) == (1, psnr, rng, 0.0, levels)
    bands = sm.forward(steps, levels)
    decoded = []
    for b in range(5):
        c = host(conts[b])
        check_streams(c, oracle_chunks(oracle, est, bands[b], chunks, rng, psnr))
        decoded.append(oracle.decomp_3d(c, False))
    want = sm.inverse(np.stack(decoded), levels)
    got = eng.decompress_series(conts, info, output_float=False).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    mse = float(((got - steps.astype(np.float64)) ** 2).mean())
    print("psnr asked %.1f dB of %g, reached %.2f dB" % (psnr, rng, 10 * np.log10(rng * rng / mse)))
    got32 = eng.decompress_series(conts, info, output_float=True).cpu().numpy()
    assert np.array_equal(bits(got32), bits(want.astype(np.float32)))


@pytest.mark.parametrize("kind", ["constant", "identical"])
def test_psnr_mode_of_steps_that_do_not_change(eng, oracle, kind):
    base = base_of("wmag17")
    steps = np.stack([np.full_like(base, 2.5) if kind == "constant" else base] * 8)
    conts, info = eng.compress_series(cuda(steps), (17, 17, 17), psnr=80.0, levels=3)
    decoded = np.stack([oracle.decomp_3d(host(c), False) for c in conts])
    assert not decoded[1:].any()                      # the detail bands are all zero
    assert len({host(c) for c in conts[1:]}) == 1      # ... and their containers, of constant chunks, are one and the same
    got = eng.decompress_series(conts, info, output_float=False).cpu().numpy()
    assert np.array_equal(bits(got), bits(sm.inverse(decoded, 3)))
    if kind == "constant":
        assert len(host(conts[0])) == len(host(conts[1]))
        # (a constant chunk keeps its value exactly: what is left is the two butterflies' rounding, rho of series.h)
        assert np.abs(got - 2.5).max() <= sm.ROUND_K[3] * 2.0 ** -53 * 2.5
    else:
        assert len(host(conts[1])) < len(host(conts[0])) // 10
        # only the approximation band carries an error, at most q_0^2 / 4 = 3 t per coefficient (psnr_vol.h); the
        # spatial wavelet is not orthonormal, so no more is claimed than 80 dB less 10 log10(3), rounded down
        rng = float(base.max()) - float(base.min())
        assert 10 * np.log10(rng * rng / float(((got - steps) ** 2).mean())) > 75.0


# ---- e. partial decodes ------------------------------------------------------------------------------------------------------

def partial_case(eng, oracle):
    steps, tol, conts, info, decoded = tol_case(eng, oracle, "vort_crop", "f32", "ragged")
    dc = [cuda(np.frombuffer(c, dtype=np.uint8)) for c in conts]
    whole = cached("partial_whole", lambda: eng.decompress_series(dc, info, output_float=False).cpu().numpy())
    return conts, dc, info, whole


def test_every_step_range_is_the_slice_of_the_whole_decode(eng, oracle):
    import torch
    conts, dc, info, whole = partial_case(eng, oracle)
    for t0 in range(11):
        for nt in range(1, 11 - t0 + 1):
            need = sm.needs(11, 3, t0, nt)
            assert eng.series_needs(11, 3, t0, nt) == need
            # the containers the range does not need hold garbage: they are neither parsed nor decoded.  They lie back
            # to back in one buffer, so the call gets all eleven byte ranges
            buf = torch.cat([dc[b] if b in need else torch.full_like(dc[b], 0xFF) for b in range(11)])
            ends = np.cumsum([0] + [c.numel() for c in dc])
            src = [buf[ends[b]:ends[b + 1]] for b in range(11)]
            got = eng.decompress_series(src, info, t0=t0, nt=nt, output_float=False).cpu().numpy()
            assert np.array_equal(bits(got), bits(whole[t0:t0 + nt])), (t0, nt)
    assert len(sm.needs(11, 3, 5, 1)) == 4


def launches(eng, call):
    import torch
    eng.profile(True)
    try:
        call()
        torch.cuda.synchronize()
        return {k: n for k, (_, n) in eng.profile_report().items() if n > 0}
    finally:
        eng.profile(False)


def count_of(counts, name):
    return sum(n for k, n in counts.items() if name in k)


def test_launches_of_a_call(eng, oracle):
    conts, dc, info, whole = partial_case(eng, oracle)
    steps = series_of("vort_crop", np.float32)
    d = cuda(steps)
    counts = launches(eng, lambda: eng.compress_series(d, CHUNKINGS["vort_crop"]["ragged"], tol=1e-2, levels=3))
    assert count_of(counts, "k_series_fwd") == 3 and count_of(counts, "k_vol_range") == 11, sorted(counts)   # 8, 2, 1
    counts = launches(eng, lambda: eng.decompress_series(dc, info, output_float=False))
    assert count_of(counts, "k_series_inv") == 3, sorted(counts)
    one = launches(eng, lambda: eng.decompress_series(dc, info, t0=5, nt=1, output_float=False))
    assert count_of(one, "k_series_inv") == 1 and count_of(one, "k_series_fwd") == 0, sorted(one)
    # The decoder's launches, kernel by kernel, are those of a boxes decode of exactly the containers series_needs names
    # -- four for one step, all eleven for the whole series -- and one step launches no more than the whole does
    dims = (40, 36, 33)

    def decoder(c):
        return {k: n for k, n in c.items() if "k_series" not in k}

    for t0, nt, got in ((5, 1, one), (0, 11, counts)):
        need = sm.needs(11, 3, t0, nt)
        want = launches(eng, lambda: eng.decompress_boxes([dc[b] for b in need], (0, 0, 0), dims, output_float=False))
        assert decoder(got) == decoder(want) and sum(decoder(got).values()) > 0, (t0, nt, decoder(got), decoder(want))
    assert len(sm.needs(11, 3, 5, 1)) == 4
    assert sum(decoder(one).values()) <= sum(decoder(counts).values())
    print("decoder launches: one step %d, whole series %d" % (sum(decoder(one).values()), sum(decoder(counts).values())))


@pytest.mark.parametrize("out_float", [False, True], ids=["f64", "f32"])
def test_a_box_is_the_crop_and_a_portion_is_the_models(eng, oracle, out_float):
    conts, dc, info, whole = partial_case(eng, oracle)
    lo, dims = (7, 5, 3), (21, 18, 17)   # (x, y, z): meets several ragged chunks
    crop = whole[:, lo[2]:lo[2] + dims[2], lo[1]:lo[1] + dims[1], lo[0]:lo[0] + dims[0]]
    dt = np.float32 if out_float else np.float64
    for t0, nt in ((0, 11), (3, 4), (10, 1)):
        got = eng.decompress_series(dc, info, t0=t0, nt=nt, box_lo_xyz=lo, box_dims_xyz=dims,
                                    output_float=out_float).cpu().numpy()
        assert got.shape == (nt, dims[2], dims[1], dims[0])
        assert np.array_equal(bits(got), bits(np.ascontiguousarray(crop[t0:t0 + nt]).astype(dt))), (t0, nt)
    half = np.stack([eng.decompress(c, output_float=False, pct=50).cpu().numpy() for c in dc])
    got = eng.decompress_series(dc, info, pct=50, output_float=out_float).cpu().numpy()
    assert np.array_equal(bits(got), bits(sm.inverse(half, 3, out_dtype=dt)))
    assert not np.array_equal(got, whole.astype(dt))


# ---- f. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(eng, oracle):
    import torch
    from sperr_amd.api import SperrHipError
    conts, dc, info, whole = partial_case(eng, oracle)
    steps = series_of("vort_crop", np.float32)
    d = cuda(steps)
    chunks = CHUNKINGS["vort_crop"]["ragged"]
    # -- compression
    for kw in (dict(tol=1e-3, levels=5), dict(tol=0.0), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")),
               dict(psnr=float("nan")), dict(psnr=60.0, range=-1.0), dict(psnr=60.0, range=float("inf")),
               dict(), dict(tol=1e-3, psnr=60.0)):
        with pytest.raises(SperrHipError):
            eng.compress_series(d, chunks, **kw)
    with pytest.raises(SperrHipError):
        eng.compress_series([], chunks, tol=1e-3)
    with pytest.raises(SperrHipError):
        eng.compress_series([d[0], d[1][:, :, :39].contiguous()], chunks, tol=1e-3)
    for pos, bad in ((0, np.nan), (steps[0].size * 7 + 4321, np.nan), (steps.size - 1, np.nan), (99, np.inf)):
        w = steps.copy()
        w.flat[pos] = bad
        for kw in (dict(tol=1e-3), dict(psnr=60.0), dict(psnr=60.0, range=2.0)):
            with pytest.raises(SperrHipError):
                eng.compress_series(cuda(w), chunks, **kw)
    # a tolerance within 2 rho of zero
    M = float(np.abs(steps).max())
    rho = sm.ROUND_K[3] * 2.0 ** -53 * M
    with pytest.raises(SperrHipError):
        eng.compress_series(d, chunks, tol=2.0 * rho)
    with pytest.raises(SperrHipError):
        eng.series_tolerance(2.0 * rho, M, 3)
    assert eng.series_tolerance(1e-3, M, 3) == sm.tolerance(1e-3, M, 3)
    # -- host calls
    for n, lv in ((0, 3), (11, 5)):
        with pytest.raises(SperrHipError):
            eng.series_plan(n, lv)
    assert eng.series_plan(11, 3) == sm.plan(11, 3)
    for t0, nt in ((11, 1), (0, 12), (5, 0), (10, 2)):
        with pytest.raises(SperrHipError):
            eng.series_needs(11, 3, t0, nt)
    assert eng.series_parse(info)["shape_zyx"] == (33, 36, 40)
    # -- decode: the outputs keep their bytes
    out = torch.full((11, 33, 36, 40), CANARY, dtype=torch.float32, device="cuda")

    def refused(**kw):
        with pytest.raises(SperrHipError):
            eng.decompress_series(kw.pop("conts", dc), kw.pop("info", info), out=kw.pop("out", out), **kw)
        assert bool((out == CANARY).all())

    refused(info=b"SPTX" + info[4:])
    refused(info=info[:4] + b"\x02" + info[5:])
    refused(info=info[:5] + b"\x05" + info[6:])
    refused(t0=11, nt=1, out=out[:1])
    refused(t0=9, nt=3, out=out[:3])
    refused(t0=0, nt=0, out=[])
    refused(box_lo_xyz=(30, 0, 0), box_dims_xyz=(11, 4, 4), out=out[:, :4, :4, :11].contiguous())
    refused(box_lo_xyz=(0, 0, 0), box_dims_xyz=(0, 4, 4), out=out[:, :4, :4, :0].contiguous())
    # containers whose dims differ from the record's, and from each other
    other = eng.compress(cuda(steps[0][:, :, :39].astype(np.float64)), chunks, 1e-3, mode=3)
    refused(conts=[other] * 11)
    refused(conts=dc[:10] + [other])
    # a damaged container, found by the decoder: the staging buffer took the decode, not the outputs
    refused(conts=dc[:3] + [torch.full_like(dc[3], 0xFF)] + dc[4:])
    refused(conts=dc[:3] + [dc[3][:20]] + dc[4:])
    # ... and the stage calls
    with pytest.raises(SperrHipError):
        eng.series_forward(d, 5)
    bands = cuda(np.zeros((11, 4, 4, 4)))
    with pytest.raises(SperrHipError):
        eng.series_inverse(bands, 3, t0=9, nt=3, out=[bands[0], bands[1], bands[2]], output_float=False)
    with pytest.raises(SperrHipError):
        eng.series_inverse(bands, 3, t0=0, nt=1, out=[bands[4]], output_float=False)   # an output inside the bands
    # after all that the call still works
    got = eng.decompress_series(dc, info, out=out).cpu().numpy()
    assert np.array_equal(bits(got), bits(whole.astype(np.float32)))


def test_arguments_refused_before_anything_is_launched(eng, oracle):
    """Straight on the C ABI, past the Python wrappers' own checks: a NULL pointer (each one, and a NULL entry of a
    pointer table), N = 0, levels = 5, a zero dimension, a step range outside the series, containers whose dims differ.
    Each returns -1; offsets, the info record, the containers' buffer, the bands and the outputs keep their bytes, and
    no kernel of the series calls is launched."""
    import ctypes as C
    import torch
    lib, st = eng.lib, eng._stream()
    sz, vp = C.c_size_t, C.c_void_p
    steps = series_of("wmag17", np.float32, n=5)
    d = cuda(steps)
    n = steps[0].size
    ptrs = (vp * 5)(*[d[t].data_ptr() for t in range(5)])
    holed = (vp * 5)(*[d[t].data_ptr() if t != 3 else None for t in range(5)])

    def refused(call, ok, changes):
        for i, v in changes:
            a = list(ok)
            a[i] = v
            assert call(*a) == -1, (call.__name__, i, v)

    def check_launches(body):
        counts = launches(eng, body)
        assert count_of(counts, "k_series") == 0 and count_of(counts, "k_vol_range") == 0, sorted(counts)

    # -- sperrhip_compress_series_dev
    dst = torch.full((eng.max_compressed_size_batch(5, (17, 17, 17), (17, 17, 17), 1e-3, 3),), 0xA5, dtype=torch.uint8,
                     device="cuda")
    offs, info = (sz * 6)(*[777] * 6), (C.c_ubyte * 64)(*[0x5A] * 64)
    ok = (ptrs, 1, 5, 17, 17, 17, 17, 17, 17, 2, 0, 1e-3, 0.0, dst.data_ptr(), dst.numel(), offs, info, st)
    check_launches(lambda: refused(lib.sperrhip_compress_series_dev, ok, [
        (0, None), (0, holed), (13, None), (15, None), (16, None),          # NULL pointers, a NULL step
        (2, 0), (9, 5), (3, 0), (4, 0), (5, 0),                             # N = 0, levels, a zero dimension
        (10, 2), (11, 0.0), (11, float("nan")), (12, -1.0), (12, float("inf"))]))
    assert list(offs) == [777] * 6 and bytes(info) == b"\x5a" * 64 and bool((dst == 0xA5).all())
    assert lib.sperrhip_compress_series_dev(*ok) == 0 and offs[0] == 0 and bytes(info)[:4] == b"SPTS"
    rec = bytes(info)
    # -- sperrhip_decompress_series_dev
    out = torch.full((5, 17, 17, 17), CANARY, dtype=torch.float64, device="cuda")
    outs = (vp * 5)(*[out[t].data_ptr() for t in range(5)])
    out_holed = (vp * 5)(*[out[t].data_ptr() if t != 2 else None for t in range(5)])
    lo, dims, zero = (sz * 3)(1, 2, 3), (sz * 3)(4, 5, 6), (sz * 3)(4, 0, 6)
    ok = (rec, dst.data_ptr(), offs, 0, 5, None, None, 0, 0, outs, st)
    # (the same series with one band's container replaced by one of a 16 x 17 x 17 volume: dims that differ)
    other = eng.compress(cuda(np.zeros((17, 17, 16))), (17, 17, 17), 1e-3, mode=3)
    conts = [dst[offs[b]:offs[b + 1]] for b in range(5)]
    mixed = torch.cat(conts[:4] + [other])
    moffs = (sz * 6)(*([offs[b] for b in range(5)] + [offs[4] + other.numel()]))
    alien = torch.cat([other] * 5)
    aoffs = (sz * 6)(*[b * other.numel() for b in range(6)])
    check_launches(lambda: refused(lib.sperrhip_decompress_series_dev, ok, [
        (0, None), (1, None), (2, None), (9, None), (9, out_holed),         # NULL pointers, a NULL output
        (5, lo), (6, dims), (6, zero),                                      # half a box
        (3, 5), (4, 6), (4, 0), (3, 4), (0, b"SPTX" + rec[4:]), (0, rec[:8] + bytes(4) + rec[12:]),   # ranges, magic, N = 0
        (0, rec[:12] + bytes(4) + rec[16:])]))                             # a zero dimension in the record
    a = list(ok)
    a[5], a[6] = lo, zero                                                   # a zero box extent
    assert lib.sperrhip_decompress_series_dev(*a) == -1
    for src, so in ((mixed, moffs), (alien, aoffs)):                         # containers whose dims differ
        a = list(ok)
        a[1], a[2] = src.data_ptr(), so
        counts = launches(eng, lambda: lib.sperrhip_decompress_series_dev(*a))
        assert lib.sperrhip_decompress_series_dev(*a) == -1 and count_of(counts, "k_series") == 0
    assert bool((out == CANARY).all())
    assert lib.sperrhip_decompress_series_dev(*ok) == 0 and not bool((out == CANARY).any())
    # -- the stage calls
    bands = torch.full((5, 17, 17, 17), CANARY, dtype=torch.float64, device="cuda")
    inside = (vp * 5)(*[d[t].data_ptr() if t != 1 else bands[2].data_ptr() for t in range(5)])
    ok = (ptrs, 1, 5, 2, n, bands.data_ptr(), st)
    check_launches(lambda: refused(lib.sperrhip_series_forward_dev, ok, [
        (0, None), (0, holed), (5, None), (2, 0), (3, 5), (4, 0), (0, inside)]))
    assert bool((bands == CANARY).all())
    assert lib.sperrhip_series_forward_dev(*ok) == 0
    out.fill_(CANARY)
    in_bands = (vp * 5)(*[out[t].data_ptr() if t != 4 else bands[0].data_ptr() for t in range(5)])
    ok = (bands.data_ptr(), 5, 2, n, 0, 5, 0, outs, st)
    check_launches(lambda: refused(lib.sperrhip_series_inverse_dev, ok, [
        (0, None), (7, None), (7, out_holed), (1, 0), (2, 5), (3, 0), (4, 5), (5, 6), (5, 0), (7, in_bands)]))
    assert bool((out == CANARY).all())
    assert lib.sperrhip_series_inverse_dev(*ok) == 0
    assert np.array_equal(bits(out.cpu().numpy()), bits(sm.inverse(sm.forward(steps, 2), 2)))


# ---- g. windows of the staging buffer, a split and poisoned workspace: in a process of its own ------------------------

CHILD = r"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from sperr_amd.api import SperrHip
import test_gpu_series as T
eng = SperrHip()
steps = T.series_of("vort_crop", np.float32)
tol = 1e-3 * (float(steps.max()) - float(steps.min()))
chunks = T.CHUNKINGS["vort_crop"]["ragged"]
before = eng.lib.sperrhip_debug_counter(8)
conts, info = eng.compress_series(T.odd_steps(steps), chunks, tol=tol, levels=3)
windows = eng.lib.sperrhip_debug_counter(8) - before
pc, pinfo = eng.compress_series(T.odd_steps(steps), chunks, psnr=70.0, levels=3)
back = eng.decompress_series(conts, info, output_float=False).cpu().numpy()
part = eng.decompress_series(conts, info, t0=5, nt=4, box_lo_xyz=(7, 5, 3), box_dims_xyz=(21, 18, 17)).cpu().numpy()
pback = eng.decompress_series(pc, pinfo, output_float=False).cpu().numpy()
json.dump({"windows": windows, "conts": [bytes(c.cpu().numpy()).hex() for c in conts], "info": info.hex(),
           "pconts": [bytes(c.cpu().numpy()).hex() for c in pc],
           "back": back.tobytes().hex(), "part": part.tobytes().hex(), "pback": pback.tobytes().hex()}, open(sys.argv[2], "w"))
"""


def test_children_in_windows_make_the_same_series(eng, oracle, tmp_path):
    eng.lib.sperrhip_debug_counter.restype = __import__("ctypes").c_ulonglong
    steps, tol, conts, info, decoded = tol_case(eng, oracle, "vort_crop", "f32", "ragged")
    dc = [cuda(np.frombuffer(c, dtype=np.uint8)) for c in conts]
    pc, pinfo = eng.compress_series(cuda(steps), CHUNKINGS["vort_crop"]["ragged"], psnr=70.0, levels=3)
    want = {"back": eng.decompress_series(dc, info, output_float=False).cpu().numpy().tobytes(),
            "part": eng.decompress_series(dc, info, t0=5, nt=4, box_lo_xyz=(7, 5, 3),
                                          box_dims_xyz=(21, 18, 17)).cpu().numpy().tobytes(),
            "pback": eng.decompress_series(pc, pinfo, output_float=False).cpu().numpy().tobytes()}
    out = tmp_path / "child.json"
    e = dict(os.environ)
    # a band is 33 * 36 * 40 * 8 bytes = 0.36 MiB: under 1 MiB the groups of 8, 2 and 1 bands are a window each
    e.update({"SPERR_HIP_SERIES_MAX_MB": "1", "SPERR_HIP_ARENA_MAX_MB": "1", "SPERR_HIP_POISON": "0xFF"})
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(ROOT), str(out)], env=e, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = json.load(open(out))
    assert got["windows"] == 3
    assert [bytes.fromhex(c) for c in got["conts"]] == conts and bytes.fromhex(got["info"]) == info
    assert [bytes.fromhex(c) for c in got["pconts"]] == [host(c) for c in pc]
    for k in want:
        assert bytes.fromhex(got[k]) == want[k], k
