"""CPU: tests/psnr_vol_model.py against the oracle's own search, orc_estimate_q_psnr(coeffs, n, range, psnr), started
from a range that is not the chunk's: the q is the oracle's bit for bit, on inputs built so that every rung of the
ladder, 0 to 4, is where the search stops -- and none beyond.

The inputs: a chunk whose coefficients are all about +-1 (the inverse transform of random signs, plus 3.0), at 60 dB
and a range chosen so that 1 / q_0 is 0.26, 0.60, 0.50, 0.35 or 0.30.  A coefficient of 1 quantised with a step of
1 / 0.26 rounds to 0 and leaves an error of 1, under t = q_0^2 / 12 = 1.23: rung 0.  The others round to 1 and leave
1 - q, which falls under t after 1, 2, 3 and 4 steps respectively."""
import ctypes as C

import numpy as np
import pytest

import psnr_vol_model as pm


@pytest.fixture(scope="module")
def est(oracle):
    f = oracle.lib.orc_estimate_q_psnr
    f.restype = C.c_double
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_double]
    g = oracle.lib.orc_estimate_mse_midtread
    g.restype = C.c_double
    g.argtypes = [C.c_void_p, C.c_size_t, C.c_double]
    return f, g


_coeffs = {}


def coeffs_of(oracle, shape):
    if shape not in _coeffs:
        vol = pm.ladder_chunk(oracle, pm.LADDER_SHAPES[shape])
        v, _, const = oracle.condition(vol)
        assert not const
        w = np.ascontiguousarray(oracle.dwt3d(v))
        w.setflags(write=False)
        _coeffs[shape] = w
    return _coeffs[shape]


def test_the_ladder_is_the_references_sequence():
    t, qs = pm.ladder(2.5, 80.0)
    assert t == (2.5 * 2.5) * 10.0 ** -8.0 or abs(t / 6.25e-8 - 1) < 1e-15
    assert qs[0] == 2.0 * np.sqrt(t * 3.0) and len(qs) == 5
    q = qs[0]
    for k in range(1, 5):
        q /= 2.0 ** 0.25
        assert abs(qs[k] / q - 1) < 4e-16
    # four steps halve q, to the rounding of four divisions: the fifth rung's bound q^2 / 4 is 0.75 t
    assert abs(qs[4] / (qs[0] / 2.0) - 1) < 1e-15 and qs[4] * qs[4] / 4.0 < 0.7500001 * t


@pytest.mark.parametrize("shape", sorted(pm.LADDER_SHAPES))
def test_the_coefficients_are_about_one(oracle, shape):
    w = coeffs_of(oracle, shape)
    a = np.abs(w)
    print(shape, "min |w|", a.min(), "max |w|", a.max())
    assert 0.9 < a.min() and a.max() < 1.1


@pytest.mark.parametrize("rung,inv_q0", list(enumerate(pm.LADDER_INV_Q0)))
@pytest.mark.parametrize("shape", sorted(pm.LADDER_SHAPES))
def test_model_stops_where_the_oracle_stops(oracle, est, shape, rung, inv_q0):
    f, g = est
    w = coeffs_of(oracle, shape)
    rng = pm.range_for(inv_q0, pm.LADDER_PSNR)
    t, qs = pm.ladder(rng, pm.LADDER_PSNR)
    q_orc = f(w.ctypes.data, w.size, rng, pm.LADDER_PSNR)
    # the condition: the oracle stops at this rung
    assert q_orc in qs, (q_orc, qs)
    assert qs.index(q_orc) == rung, (qs.index(q_orc), rung)
    # the model agrees, estimate by estimate
    for k in range(rung + 1):
        assert pm.estimate(w, qs[k]) == g(w.ctypes.data, w.size, qs[k]), k
    q, k = pm.chunk_q(w, rng, pm.LADDER_PSNR)
    assert k == rung and q == q_orc
    assert k <= 4


def test_width_rule():
    assert pm.width(4294967295.4, 1.0) == 4 and pm.width(4294967295.6, 1.0) == 8
    assert pm.width(2.0 ** 63, 1.0) is None and pm.width(np.nextafter(2.0 ** 63, 0.0), 1.0) == 8
    assert pm.width(float("nan"), 1.0) is None and pm.width(0.0, 1.0) == 4
