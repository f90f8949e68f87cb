"""CPU: the LOG kind of point-wise relative error on its numpy statement (tests/rel_log_model.py), without the library.

  accuracy     the measurement the slack s rests on.  Against mpmath at 256 bits: log2 over 24 000 magnitudes spread
               over [2^-1022, 2^1023] and 6 000 near 1 and near sqrt(2) (where the fold switches), split into the
               floats' range and beyond it; exp2 over the clamp range; the tolerance over eps from the floor to 0.5.
               With dL the worst absolute error of y, dX the worst relative error of 2^y' (as log2(1 + dX)) and dT the
               worst absolute error of t + s, the rule's inequality (rel.h)
                   2^(t + dL) (1 + dX) (1 + 2^-24) <= 1 + eps
               holds when dL + log2(1 + dX) + dT + log2(1 + 2^-24) <= s; the test asks for FOUR times the measured
               sum, plus the narrowing term (float output only), under s: 2^-22 for fp32 data, 2^-40 for fp64 data.
  the bound    as tests/test_rel_model.py: fp32 and fp64 data, eps in {this kind's floor, 1e-4, 1e-2, 0.5}, d in
               {+t, -t, 0} over the adversarial samples, rechecked in exact rational arithmetic: none fails
  the oracle   tests/golden/vort_crop.f32 with its zeros in chunks (20, 18, 16) through the oracle: the coder's bound
               on y, then no violation and no class mismatch for float and double output
  the sizes    the oracle's container of this kind's y at its t is smaller than the oracle's container of the linear
               kind's y at its t: vort_with_zeros at eps 1e-2 and 1e-4, and tools/rel_bench.py's field at 32^3"""
import numpy as np
import pytest

import mask_model as M
import rel_log_model as L
import rel_model as R
from test_rel_model import EPS, PATHS, bound_failures

NARROW = float(np.log2(1.0 + 2.0 ** -24))   # what narrowing to a normal float adds, in the y domain


@pytest.fixture(scope="module")
def measured():
    """{name: worst error} of the two maps and the tolerance against mpmath, in the y domain"""
    import mpmath as mp
    mp.mp.prec = 256
    rng = np.random.default_rng(2024)

    def log_err(mag):
        got = L.log2(mag)
        return max(abs(mp.mpf(float(g)) - mp.log(mp.mpf(float(m)), 2)) for g, m in zip(got, mag))

    # (a random mantissa under a random exponent: 2^u of a double u would have a logarithm that is nearly a double)
    wide = np.ldexp(rng.uniform(1.0, 2.0, 24000), rng.integers(-1022, 1024, 24000).astype(np.int32))
    wide = np.concatenate([wide, [2.0 ** -1022, np.finfo(np.float64).max, 1.0]])
    floats = (wide < 2.0 ** 128) & (wide >= 2.0 ** -149)
    near = np.concatenate([1.0 + rng.uniform(-2.0 ** -8, 2.0 ** -8, 3000),
                           np.sqrt(2.0) * (1.0 + rng.uniform(-2.0 ** -8, 2.0 ** -8, 3000)),
                           np.float64(L.SQRT2) + np.arange(-8, 9) * 2.0 ** -52])
    near = near * np.exp2(rng.integers(-149, 128, near.size).astype(np.float64))
    out = {"log2, the floats' range": max(log_err(wide[floats]), log_err(near)),
           "log2, all doubles": log_err(wide)}
    y = np.concatenate([rng.uniform(R.Y_MIN + 60.0, R.Y_MAX, 20000), rng.uniform(-1.0, 1.0, 4000),
                        np.arange(-200, 200) + 0.5, np.nextafter(np.arange(-200, 200) + 0.5, np.inf)])
    got = L.exp2(y)
    assert np.isfinite(got).all() and (got > 0).all()
    # (the relative error of 2^y' as a distance in the y domain; the lowest binades round on the subnormals' absolute
    #  grid, which is ldexp's one rounding and not the map's: they are left to the bound's own test)
    keep = y >= -1021.0
    out["exp2"] = max(abs(mp.log(mp.mpf(float(g)), 2) - mp.mpf(float(v))) for g, v in zip(got[keep], y[keep]))
    for is_float in (True, False):
        lo = L.tolerance_floor(is_float)
        eps = np.concatenate([np.exp(rng.uniform(np.log(lo), np.log(0.5), 3000)), [lo, 1e-4, 1e-2, 0.5]])
        s = R.slack(is_float)
        out["t, fp32 data" if is_float else "t, fp64 data"] = max(
            abs(mp.mpf(L.tolerance(e, is_float)) + mp.mpf(s) - mp.log(1 + mp.mpf(float(e)), 2)) for e in eps)
    for k, v in out.items():
        print(f"worst error of {k}: 2^{float(mp.log(v, 2)):.2f}")
    return {k: float(v) for k, v in out.items()}


@pytest.mark.parametrize("is_float", [True, False], ids=["f32", "f64"])
def test_four_times_the_measured_errors_fit_under_the_slack(measured, is_float):
    dL = measured["log2, the floats' range" if is_float else "log2, all doubles"]
    dX, dT = measured["exp2"], measured["t, fp32 data" if is_float else "t, fp64 data"]
    narrow = NARROW if is_float else 0.0   # (fp64 data comes back as doubles)
    s = R.slack(is_float)
    print(f"dL 2^{np.log2(dL):.2f}, dX 2^{np.log2(dX):.2f} (y domain), dT 2^{np.log2(dT):.2f}; 4 x sum + narrowing = "
          f"2^{np.log2(4.0 * (dL + dX + dT) + narrow):.2f} against s = 2^{np.log2(s):.0f}")
    assert 4.0 * (dL + dX + dT) + narrow <= s


@pytest.mark.parametrize("eps_name", list(EPS))
@pytest.mark.parametrize("path", list(PATHS))
def test_bound_on_the_adversarial_samples(path, eps_name):
    dtype, output_float = PATHS[path]
    is_float = dtype == np.float32
    eps = EPS[eps_name] if EPS[eps_name] is not None else L.tolerance_floor(is_float)
    t = L.tolerance(eps, is_float)
    assert t is not None and t >= R.slack(is_float)
    x = R.adversarial(dtype)
    y, zero, neg = L.forward(x)
    bad = {}
    for name, d in (("+t", t), ("-t", -t), ("0", 0.0)):
        xr = L.inverse(y + d, zero, neg, output_float, is_float)
        assert np.isfinite(xr).all()
        fails, ratio = bound_failures(x, xr, eps)
        print(f"{path} eps={eps!r} d={name}: worst error / bound {ratio:.6f}, {len(fails)} of {x.size} fail")
        if fails:
            bad[name] = (len(fails), [float(x[i]).hex() for i in fails[:4]])
    assert not bad, bad


def test_tolerance_and_its_refusals():
    for is_float in (True, False):
        s = R.slack(is_float)
        floor = L.tolerance_floor(is_float)
        below = float(np.nextafter(np.float64(floor), np.float64(0.0)))
        assert L.tolerance(floor, is_float) >= s and L.tolerance(below, is_float) is None
        # t = s where log2(1 + eps) = 2 s: eps a hair over 2 s ln 2
        assert 2.0 * s * np.log(2.0) < floor < 2.0 * s * np.log(2.0) * (1.0 + 8.0 * s) + 2.0 ** -52
        for eps in (0.0, -0.0, -1e-2, -1.0, -2.0, 0.6, np.inf, -np.inf, np.nan):
            assert L.tolerance(eps, is_float) is None
        for eps in (1e-4, 1e-2, 0.5):   # log2(1 + eps) against eps / (1 + eps): 1.44 to 1.75 times the linear kind's
            assert 1.44 < L.tolerance(eps, is_float) / R.tolerance(eps, is_float) < 1.76
        # this kind's floor is below the linear kind's: an eps between them is this kind's alone
        assert L.tolerance(R.tolerance_floor(is_float), is_float) is not None and R.tolerance(floor, is_float) is None


def test_inverse_of_forward_is_the_sample_for_floats_and_close_for_doubles():
    x = R.adversarial(np.float32)
    y, zero, neg = L.forward(x)
    back = L.inverse(y, zero, neg, True, True)
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))
    x = R.adversarial(np.float64)
    y, zero, neg = L.forward(x)
    back = L.inverse(y, zero, neg, False, False)
    nz = ~zero
    assert (back[zero] == 0).all() and np.array_equal(np.signbit(back), np.signbit(x))
    with np.errstate(over="ignore"):
        assert (np.abs(back[nz] - x[nz]) <= 2.0 ** -43 * np.abs(x[nz])).all()


def test_both_ends_of_the_clamp_decode_to_finite_values():
    one, no = np.zeros(1, dtype=bool), np.zeros(1, dtype=bool)
    for yp in (R.Y_MIN, R.Y_MAX, -np.inf, np.inf, np.nan, -5000.0, 5000.0, 1024.0, float(np.nextafter(R.Y_MAX, 0.0))):
        for output_float in (True, False):
            for is_float in (True, False):
                a = L.inverse(np.array([yp]), one, no, output_float, is_float)
                assert np.isfinite(a).all() and a[0] >= 0, (yp, output_float, is_float)
    top = L.exp2(np.array([R.Y_MAX, float(np.nextafter(R.Y_MAX, 0.0))]))
    assert 2.0 ** 1023 < top[1] <= top[0] <= L.DBL_MAX
    assert L.exp2(np.array([R.Y_MIN]))[0] == 0.0 and L.exp2(np.array([-1074.0]))[0] == 2.0 ** -1074
    assert L.inverse(np.array([R.Y_MAX]), one, no, True, False)[0] == np.finfo(np.float32).max
    # the powers of two are exact both ways
    e = np.arange(-1022, 1024).astype(np.float64)
    assert np.array_equal(L.exp2(e), np.exp2(e)) and np.array_equal(L.log2(np.exp2(e)), e)


@pytest.fixture(scope="module")
def vort():
    vol = R.vort_with_zeros()
    return vol, L.forward(vol), R.forward(vol)


def filled(y, zero, shape):
    yf = M.filled(y.reshape(shape), zero.reshape(shape))
    assert yf is not None and np.isfinite(yf).all()
    return yf


@pytest.mark.parametrize("eps", [1e-2, 1e-4])
def test_through_the_oracle_within_the_bound_and_smaller_than_the_linear_kind(oracle, vort, eps):
    vol, (y, zero, neg), (ylin, zlin, nlin) = vort
    assert np.array_equal(zero, zlin) and np.array_equal(neg, nlin)
    t, tlin = L.tolerance(eps, True), R.tolerance(eps, True)
    container = oracle.comp_3d(filled(y, zero, vol.shape), (20, 18, 16), 3, t)
    linear = oracle.comp_3d(filled(ylin, zero, vol.shape), (20, 18, 16), 3, tlin)
    yp = oracle.decomp_3d(container, output_float=False)
    assert yp.shape == vol.shape and yp.dtype == np.float64
    nz = ~zero
    assert (np.abs(yp.reshape(-1)[nz] - y[nz]) <= t).all(), "the coder's own point-wise bound"
    for output_float in (True, False):
        xr = L.inverse(yp.reshape(-1), zero, neg, output_float, True)
        fails, ratio = bound_failures(vol.reshape(-1), xr, eps)
        worst, viol, mis, cnt = R.check(vol, xr, eps)
        print(f"eps={eps!r} float={output_float}: log {len(container)} bytes, linear {len(linear)}; worst error / bound "
              f"{ratio:.6f}, worst relative error {worst:.3e}")
        assert not fails and viol == 0 and mis == 0 and cnt == int(nz.sum())
    assert len(container) < len(linear)


def test_smaller_than_the_linear_kind_on_the_bench_field(oracle):
    vol = L.synthetic(32)
    eps = 1e-2
    y, zero, neg = L.forward(vol)
    ylin, _, _ = R.forward(vol)
    assert int(zero.sum()) > 100 and int(neg.sum()) > 1000
    container = oracle.comp_3d(filled(y, zero, vol.shape), (32, 32, 32), 3, L.tolerance(eps, True))
    linear = oracle.comp_3d(filled(ylin, zero, vol.shape), (32, 32, 32), 3, R.tolerance(eps, True))
    print(f"32^3 bench field, eps {eps}: log {len(container)} bytes, linear {len(linear)}")
    assert len(container) < len(linear)
    xr = L.inverse(oracle.decomp_3d(container, output_float=False).reshape(-1), zero, neg, True, True)
    assert R.check(vol, xr, eps)[1:3] == (0, 0)
