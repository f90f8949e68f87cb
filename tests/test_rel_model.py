"""CPU: the guarantee of point-wise relative error on the numpy statement of the rule (tests/rel_model.py), without the
library.

  the bound    for fp32 and fp64 data and eps in {the floor, 1e-4, 1e-2, 0.5}: x' = inverse(forward(x) + d) for d in
               {+t, -t, 0} over the adversarial samples -- the powers of two from 2^-149 to 2^127 with both neighbours,
               float subnormals, the largest values, both signs; for fp64 data also doubles far outside the floats'
               range -- must satisfy |x' - x| <= eps |x|.  The check runs in doubles; every sample that fails it or
               comes within 2^-30 of the bound is checked again in exact rational arithmetic, and none may fail there.
  the oracle   tests/golden/vort_crop.f32 with a ball of zeros and a few -0.0, in chunks (20, 18, 16): the model's y,
               in-filled, through the oracle's fp64 point-wise error compress at t and its decode, then the model's
               inverse: every sample within the bound, zeros and signs exact.  The reference alone stays within it.

The subnormal floats are why fp32 data is stretched by 2 below y = -126 (rel.h): without the stretch x = 2^-143, 64
units of the floats' absolute grid there, at eps = 1e-2 and y' = y + t narrows to 65 units, an error of 1.5625 %;
test_unstretched_subnormal_floats_would_break_the_bound keeps that on record."""
from fractions import Fraction

import numpy as np
import pytest

import mask_model as M
import rel_model as R

EPS = {"floor": None, "1e-4": 1e-4, "1e-2": 1e-2, "0.5": 0.5}
PATHS = {"f32-to-f32": (np.float32, True), "f32-to-f64": (np.float32, False), "f64-to-f64": (np.float64, False)}


def exact_failures(x, xr, eps, idx):
    """the samples of idx with |x' - x| > eps |x| in rational arithmetic"""
    e = Fraction(float(eps))
    return [int(i) for i in idx
            if abs(Fraction(float(xr[i])) - Fraction(float(x[i]))) > e * abs(Fraction(float(x[i])))]


def bound_failures(x, xr, eps):
    """(samples that break the bound, exactly; the worst ratio of error to bound in doubles)"""
    a, b = x.astype(np.float64), xr.astype(np.float64)
    zero, neg, _ = R.classes(a)
    assert np.array_equal(np.signbit(b), neg) and (b[zero] == 0).all(), "zeros and signs are exact"
    with np.errstate(over="ignore"):   # (the largest doubles against each other)
        err, room = np.abs(b - a), np.float64(eps) * np.abs(a)
    flagged = np.flatnonzero(~zero & ~(err <= room * (1.0 - 2.0 ** -30)))
    ratio = float((err[~zero] / room[~zero]).max())
    return exact_failures(a, b, eps, flagged), ratio


@pytest.mark.parametrize("eps_name", list(EPS))
@pytest.mark.parametrize("path", list(PATHS))
def test_bound_on_the_adversarial_samples(path, eps_name):
    dtype, output_float = PATHS[path]
    is_float = dtype == np.float32
    eps = EPS[eps_name] if EPS[eps_name] is not None else R.tolerance_floor(is_float)
    t = R.tolerance(eps, is_float)
    assert t is not None and t >= R.slack(is_float)
    x = R.adversarial(dtype)
    y, zero, neg = R.forward(x)
    bad = {}
    for name, d in (("+t", t), ("-t", -t), ("0", 0.0)):
        xr = R.inverse(y + d, zero, neg, output_float, is_float)
        assert np.isfinite(xr).all()
        fails, ratio = bound_failures(x, xr, eps)
        print(f"{path} eps={eps!r} d={name}: worst error / bound {ratio:.6f}, {len(fails)} of {x.size} fail")
        if fails:
            worst = max(fails, key=lambda i: abs(float(xr[i]) - float(x[i])) / abs(float(x[i])))
            bad[name] = (len(fails), float(x[worst]).hex(), abs(float(xr[worst]) - float(x[worst])) / abs(float(x[worst])))
    assert not bad, bad


def test_unstretched_subnormal_floats_would_break_the_bound():
    x = np.array([2.0 ** -143, 2.0 ** -136], dtype=np.float32)
    y64, zero, neg = R.forward(x.astype(np.float64))   # (as doubles: the map without the stretch)
    for k, eps in enumerate((1e-2, 1e-4)):
        t = R.tolerance(eps, True)
        plain = R.inverse(y64 + t, zero, neg, True, False)
        assert abs(float(plain[k]) - float(x[k])) > eps * float(x[k])
        y, _, _ = R.forward(x)
        assert y[k] == -126.0 + 2.0 * (y64[k] + 126.0)
        kept = R.inverse(y + t, zero, neg, True, True)
        assert abs(float(kept[k]) - float(x[k])) <= eps * float(x[k])


def test_inverse_of_forward_is_the_sample_for_floats_and_close_for_doubles():
    x = R.adversarial(np.float32)
    y, zero, neg = R.forward(x)
    back = R.inverse(y, zero, neg, True, True)
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))
    x = R.adversarial(np.float64)
    y, zero, neg = R.forward(x)
    back = R.inverse(y, zero, neg, False, False)
    nz = ~zero
    assert (back[zero] == 0).all() and np.array_equal(np.signbit(back), np.signbit(x))
    with np.errstate(over="ignore"):
        assert (np.abs(back[nz] - x[nz]) <= 2.0 ** -43 * np.abs(x[nz])).all()   # (y is rounded once: 2^-44 of a slope <= |x|)


@pytest.mark.parametrize("eps", [1e-2, 1e-4])
def test_the_oracle_alone_stays_within_the_bound(oracle, eps):
    vol = R.vort_with_zeros()
    t = R.tolerance(eps, True)
    y, zero, neg = R.forward(vol)
    assert int(zero.sum()) > 3000 and int((zero & neg).sum()) >= 4
    yf = M.filled(y.reshape(vol.shape), zero.reshape(vol.shape))
    assert yf is not None and np.isfinite(yf).all()
    container = oracle.comp_3d(yf, (20, 18, 16), 3, t)
    yp = oracle.decomp_3d(container, output_float=False)
    assert yp.shape == vol.shape and yp.dtype == np.float64
    nz = ~zero
    assert (np.abs(yp.reshape(-1)[nz] - y[nz]) <= t).all(), "the coder's own point-wise bound"
    for output_float in (True, False):
        xr = R.inverse(yp.reshape(-1), zero, neg, output_float, True)
        fails, ratio = bound_failures(vol.reshape(-1), xr, eps)
        worst, viol, mis, cnt = R.check(vol, xr, eps)
        print(f"eps={eps!r} float={output_float}: {len(container)} bytes, worst error / bound {ratio:.6f}, "
              f"worst relative error {worst:.3e}")
        assert not fails and viol == 0 and mis == 0 and cnt == int(nz.sum())
