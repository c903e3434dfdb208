"""CPU: the oracle's exp / log / sincos2pi / softplus / sigmoid / norm_ppf / pow on the edge tables of tests/math_edges.py against mpmath at 250 bits.
The error is counted in ulp of the correctly rounded result; special values (NaN, infinities, zeros with their sign) must be exact.  The arithmetic
is IEEE-only and deterministic, so each bound is the maximum measured on the committed table, rounded up to the next half ulp (DESIGN.md section 3
carries the figures); the margin absorbs nothing but the rounding of the figure.  Run with -s to see the measured maxima."""
import ctypes
import math
from fractions import Fraction

import mpmath
import numpy as np

import math_edges as me
import orc

mpmath.mp.prec = 250
mp = mpmath.mp
TWO_PI = 2 * mp.pi


def _round(v):
    """an mpf correctly rounded to binary64 (through Fraction: one rounding, also in the subnormal range and at overflow)"""
    if v == 0:
        return 0.0
    man, exp = int(v.man), int(v.exp)
    fr = Fraction(man * 2 ** exp) if exp >= 0 else Fraction(man, 2 ** -exp)
    try:
        r = abs(float(fr))
    except OverflowError:
        r = me.INF
    return -r if v < 0 else r


def _mp_norm_ppf(p):
    """the root of Phi(z) = p: z = -sqrt(2) erfcinv(2 p), by Newton steps on Phi from an asymptotic start (mpmath's erfinv covers the centre only)"""
    p = mp.mpf(p)
    if p > 0.5:
        return -_mp_norm_ppf_lower(1 - p)                  # 1 - p is exact at this precision for every binary64 p
    return _mp_norm_ppf_lower(p)


def _mp_norm_ppf_lower(p):
    if p == 0.5:
        return mp.mpf(0)
    z = -mp.sqrt(-2 * mp.log(p)) if p < 0.1 else mp.mpf(float(p) - 0.5) * 2.5
    for _ in range(200):
        cdf = mp.erfc(-z / mp.sqrt(2)) / 2
        step = (cdf - p) / (mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi))
        z -= step
        if abs(step) <= abs(z) * mp.mpf(2) ** -200:
            return z
    raise AssertionError(f"no convergence at p = {p}")


# reference(x) -> a float (a special value, exact by rule) or an mpf (a finite non-zero true value, or a true zero)
def _ref_exp(x):
    if x != x:
        return me.NAN
    if math.isinf(x):
        return me.INF if x > 0 else 0.0
    return mp.exp(mp.mpf(x))


def _ref_log(x):
    if x != x or x < 0:
        return me.NAN
    if x == 0:
        return -me.INF
    if math.isinf(x):
        return me.INF
    return mp.log(mp.mpf(x))


def _ref_softplus(x):
    if x != x:
        return me.NAN
    if math.isinf(x):
        return me.INF if x > 0 else 0.0
    return mp.log1p(mp.exp(mp.mpf(x)))


def _ref_sigmoid(x):
    if x != x:
        return me.NAN
    if math.isinf(x):
        return 1.0 if x > 0 else 0.0
    return 1 / (1 + mp.exp(-mp.mpf(x)))


def _ref_norm_ppf(p):
    if p != p:
        return me.NAN
    if p <= 0:
        return -me.INF
    if p >= 1:
        return me.INF
    return _mp_norm_ppf(p)


def _ref_pow(x, y):
    if x != x or y != y:
        return me.NAN
    if x == 0:
        return me.INF if y < 0 else me.NAN
    if math.isinf(x):
        return 0.0 if y < 0 else me.NAN
    if math.isinf(y):
        return me.NAN
    return mp.power(mp.mpf(x), mp.mpf(y))


def _errors(got, refs, absolute_floor=None):
    """ulp errors of got against the references; special values are asserted exact here.  absolute_floor: the unit is max(ulp(result), floor)"""
    errs = np.zeros(len(got))
    for i, (g, r) in enumerate(zip(got, refs)):
        g = float(g)
        if isinstance(r, float):                                           # a special value by rule
            assert (g != g) if r != r else (g == r and math.copysign(1, g) == math.copysign(1, r)), f"entry {i}: {g!r}, expected exactly {r!r}"
            continue
        cr = _round(r)
        if r == 0 or cr == 0 or math.isinf(cr):                            # a true zero, an underflow to zero, an overflow: exact, with the sign
            if absolute_floor is None or math.isinf(cr):
                assert g == cr and math.copysign(1, g) == math.copysign(1, cr), f"entry {i}: {g!r}, expected exactly {cr!r}"
                continue
        assert math.isfinite(g), f"entry {i}: {g!r} where the true value rounds to {cr!r}"
        unit = float(np.spacing(abs(cr)))
        if absolute_floor is not None:
            unit = max(unit, absolute_floor)
        errs[i] = float(abs(mp.mpf(g) - r) / mp.mpf(unit))
    return errs


def _half_ulp_above(m):
    return math.floor(m * 2) / 2 + 0.5


def _check(name, errs, bound, x):
    i = int(np.argmax(errs))
    print(f"{name}: max {errs[i]:.4f} ulp at entry {i} (x = {np.ravel(x)[i]!r}), bound {bound}")
    assert errs[i] <= bound
    assert bound == _half_ulp_above(errs[i]), f"{name}: the bound {bound} is not the next half ulp above the measured {errs[i]:.4f}"


def test_exp_table_against_mpmath():
    x = me.exp_table()
    errs = _errors(orc.math_eval(0, x)[0], [_ref_exp(float(v)) for v in x])
    _check("exp", errs, 1.0, x)
    sub = x < -708.39
    print(f"exp, subnormal results alone: max {errs[sub].max():.4f} ulp")


def test_log_table_against_mpmath():
    x = me.log_table()
    _check("log", _errors(orc.math_eval(1, x)[0], [_ref_log(float(v)) for v in x]), 1.5, x)


def test_sincos_table_against_mpmath():
    """In units of max(ulp(result), 2^-53): next to an octant edge the true sine or cosine is of the size of the argument's own rounding, and the reduced
    angle t pi/4 carries the relative error of the double pi/4.  At u = 1/2 the sine is -0.0 by the octant table (sn = -s for octants 4..7): sign not held."""
    u = me.sincos_table()
    s, c = orc.math_eval(2, u)
    rs = [mp.sin(TWO_PI * mp.mpf(float(v))) for v in u]
    rc = [mp.cos(TWO_PI * mp.mpf(float(v))) for v in u]
    _check("sin2pi", _errors(s, rs, absolute_floor=2.0 ** -53), 1.0, u)
    _check("cos2pi", _errors(c, rc, absolute_floor=2.0 ** -53), 1.0, u)
    assert s[0] == 0.0 and not np.signbit(s[0]) and c[0] == 1.0                      # u = 0 exactly


def test_softplus_table_against_mpmath():
    """softplus(eta) = log(1 + exp(eta)) returns exactly 0 once 1 + exp(eta) rounds to 1 (eta below about -36.7), where the true value is e^eta: the
    defined arithmetic, not a bug.  Its error is therefore absolute, in units of max(ulp(result), 2^-53)."""
    x = me.logistic_table()
    got = orc.math_eval(3, x)[0]
    _check("softplus", _errors(got, [_ref_softplus(float(v)) for v in x], absolute_floor=2.0 ** -53), 1.0, x)
    assert np.all(got[x < -37.5] == 0.0) and not np.signbit(got[x < -37.5]).any()


def test_sigmoid_table_against_mpmath():
    x = me.logistic_table()
    _check("sigmoid", _errors(orc.math_eval(4, x)[0], [_ref_sigmoid(float(v)) for v in x]), 1.5, x)


def test_norm_ppf_table_against_mpmath():
    p = me.norm_ppf_table()
    got = orc.math_eval(5, p)[0]
    _check("norm_ppf", _errors(got, [_ref_norm_ppf(float(v)) for v in p]), 4.5, p)


def test_host_norm_ppf_equals_the_oracle_bit_for_bit():
    """mi_mcmc_norm_ppf (the engine header's statement, compiled for the host) against orc_norm_ppf (the oracle's own statement of AS 241)"""
    import mcmc_amd
    p = me.norm_ppf_table()
    a, b = mcmc_amd.norm_ppf(p), orc.math_eval(5, p)[0]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a.view(np.uint64)[~np.isnan(a)], b.view(np.uint64)[~np.isnan(b)])


def test_pow_table_against_mpmath():
    x, y = me.pow_table()
    n = len(me.POW_NAN_BY_DEFINITION)
    got = orc.math_eval(6, x, y)[0]
    assert np.isnan(got[-n:]).all()                                                    # exp(y log x) with 0 * inf inside: NaN, stated in math_edges.py
    assert [(float(a), float(b)) for a, b in zip(x[-n:], y[-n:])] == me.POW_NAN_BY_DEFINITION
    _check("pow", _errors(got[:-n], [_ref_pow(float(a), float(b)) for a, b in zip(x[:-n], y[:-n])]), 5.5, x[:-n])



def test_exact_fma_of_the_tile_reference_is_the_hosts_fma():
    """math_edges.fma_ieee (exact rationals, IEEE rules for the non-finite steps written out) against libm's fma on every step of every tile's chain"""
    libm = ctypes.CDLL("libm.so.6")
    libm.fma.restype, libm.fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    for name, (A, B, C) in me.mfma_tiles().items():
        assert A.shape == (16, 4) and B.shape == (4, 16) and C.shape == (16, 16)
        for i in range(16):
            for j in range(16):
                acc = float(C[i, j])
                for k in range(4):
                    want = libm.fma(float(A[i, k]), float(B[k, j]), acc)
                    acc = me.fma_ieee(float(A[i, k]), float(B[k, j]), acc)
                    assert (acc != acc and want != want) or (acc == want and math.copysign(1, acc) == math.copysign(1, want)), (name, i, j, k)


def test_tiles_reach_what_their_names_say():
    tiny = 2.2250738585072014e-308
    t = me.mfma_tiles()
    D = {n: me.mfma_reference(*abc) for n, abc in t.items()}
    for n in ("sub_all", "sub_products", "sub_cancel"):
        assert ((np.abs(D[n]) < tiny) & (D[n] != 0)).sum() >= 200                      # subnormal results
    for n in ("sub_operand_normal_product", "sub_operand_b"):
        A, B, _ = t[n]
        assert (np.abs(A) < tiny).all() or (np.abs(B) < tiny).all()
        assert (np.abs(D[n]) > tiny).all()
    assert (np.signbit(D["zeros_only"]) & (D["zeros_only"] == 0)).sum() == 128
    assert np.isinf(D["overflow_mid_chain"]).all() and np.isfinite(D["near_overflow"]).all()
    assert np.isnan(D["inf_rules"]).sum() > 4 and np.isinf(D["inf_rules"]).sum() > 4
    assert np.isnan(D["nan_in_a"]).sum() == 16 and np.isnan(D["nan_in_b"]).sum() == 16 and np.isnan(D["nan_in_c"]).sum() == 2
