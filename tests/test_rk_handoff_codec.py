"""The codec that hands New from RK4 stage 1 to stage 2 as one byte per value (moka_set_tuning key 12; rk_handoff_* in
csrc/kernels_common.hpp), through its host build moka_rk_handoff_codec: no GPU.

Stage 1 forms P = C + a t and N = C + b t (a = dt / 2, b = dt / 6) from one tendency; the code is the distance of the bit patterns
of N and of the prediction C + (P - C) * (b / a), or the escape -128, in which case N itself travels.  Whatever the inputs, what
stage 2 rebuilds must be N bit for bit; the byte is worth having only if escapes are rare on model-like values, and the escape
path has to be exercised by something, which the cancellation family does.  Inputs are formed here with numpy's plain
multiply and add, the arithmetic of the kernels (-ffp-contract=off)."""
import ctypes as C

import numpy as np
import pytest

from moka_hip import lib as L

N_VALUES = 1_000_000
ESCAPE = -128
DTS = (30.0, 37.123, 0.0)
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")      # inf - inf, 0 * inf in the special rows: meant


def coefficients(dt):
    a, b = dt / 2.0, dt / 6.0
    return a, b, (b / a if a != 0.0 else 0.0)


def codec(Cv, P, N, rho):
    Cv, P, N = (np.ascontiguousarray(x, dtype=np.float64) for x in (Cv, P, N))
    code, dec = np.empty(Cv.size, dtype=np.int8), np.empty(Cv.size, dtype=np.float64)
    f64p = C.POINTER(C.c_double)
    rc = L.lib().moka_rk_handoff_codec(Cv.ctypes.data_as(f64p), P.ctypes.data_as(f64p), N.ctypes.data_as(f64p), rho, Cv.size,
                                       code.ctypes.data_as(C.POINTER(C.c_int8)), dec.ctypes.data_as(f64p))
    assert rc == 0
    return code, dec


def family(name, dt, rng):
    """(C, t) of one input family; the specials carry every combination of a special C with ordinary and special t."""
    n = N_VALUES
    _, b, _ = coefficients(dt)
    if name == "h-like":                  # layerThickness: 5 .. 50 m, increments a t of about 1e-4
        return rng.uniform(5.0, 50.0, n), 1e-5 * rng.standard_normal(n)
    if name == "u-like":                  # normalVelocity: about 0.1 m/s either sign
        return 0.1 * rng.standard_normal(n), 1e-5 * rng.standard_normal(n)
    if name == "zero":                    # a state at rest: New and Provis are pure increments
        return np.zeros(n), 1e-4 * rng.standard_normal(n)
    if name == "decades":                 # magnitudes of C and t independent over 15 decades, either sign
        mag = lambda: 10.0 ** rng.uniform(-8.0, 7.0, n) * rng.choice([-1.0, 1.0], n)
        return mag(), mag()
    if name == "cancellation":            # New = C + b t cancels to its last bits: nothing predicts those
        t = rng.standard_normal(n)
        return -b * t * (1.0 + 1e-9 * rng.standard_normal(n)), t
    assert name == "special"
    tiny = np.float64(5e-324)
    pool = np.array([np.nan, np.inf, -np.inf, tiny, -tiny, 1000 * tiny, 2.0 ** -1022, -2.0 ** -1030, 0.0, -0.0, 1.0, -3.5e300, 1.7e308])
    return rng.choice(pool, n), np.where(rng.random(n) < 0.5, rng.choice(pool, n), rng.standard_normal(n))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["h-like", "u-like", "zero", "decades", "cancellation", "special"])
def test_decoded_is_new_bit_for_bit(name, dt):
    rng = np.random.default_rng(7 + DTS.index(dt))
    a, b, rho = coefficients(dt)
    Cv, t = family(name, dt, rng)
    P, N = Cv + a * t, Cv + b * t
    code, dec = codec(Cv, P, N, rho)
    assert np.array_equal(dec.view(np.uint64), N.view(np.uint64))
    # a code that is no escape is the distance of the two bit patterns: the prediction of the same expression in numpy, plus the code
    pred = Cv + (P - Cv) * rho
    keep = code != ESCAPE
    assert np.array_equal((pred.view(np.int64)[keep] + code[keep].astype(np.int64)).view(np.float64).view(np.uint64), N.view(np.uint64)[keep])
    share = float(np.mean(code == ESCAPE))
    print(f"{name} dt={dt}: escape share {share:.3e}, exact {float(np.mean(code == 0)):.5f}")
    if name in ("h-like", "u-like", "zero"):
        assert share <= 1e-3, share
    if name == "cancellation" and dt != 0.0:         # (dt = 0: b = 0, the family is C = 0 without increments and has nothing to cancel)
        assert share > 0.1, share
    if name == "special":
        assert (code[np.isnan(N)] == ESCAPE).all() and keep.any()


def test_argument_errors():
    lib = L.lib()
    assert lib.moka_rk_handoff_codec(None, None, None, 1.0 / 3.0, 4, None, None) == L.ERR_ARG
    assert lib.moka_rk_handoff_codec(None, None, None, 1.0 / 3.0, 0, None, None) == 0
    v = C.c_int()
    assert lib.moka_get_tuning(12, C.byref(v)) == 0 and v.value in (0, 1)
    for bad in (2, -1):
        assert lib.moka_set_tuning(12, bad) == L.ERR_ARG
    assert lib.moka_get_tuning(12, C.byref(v)) == 0 and v.value in (0, 1)
