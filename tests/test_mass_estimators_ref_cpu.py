"""CPU: the numpy mirrors of the two mass-estimator kernels (tests/mass_estimators_ref.py) against the exact variance in rational arithmetic.

THE BOUND (two-pass variance; u = 2^-53, gamma_k = k u / (1 - k u); N samples x_k, exact mean mu, exact V = sum (x_k - mu)^2 / (N - 1)):

1. The mean.  A sample passes through at most A additions and one division before it is part of the computed mean (the first addition, to +0, is exact), so
   mean^ = mu + delta,  |delta| <= gamma_(A + 1) * sum |x_k| / N.
     pooled kernel:    a lane adds ceil(N / 256) samples (ceil(N / 256) - 1 inexact additions), the halving tree adds 8 times:  A = ceil(N / 256) + 7
     per-chain kernel: one ascending sum of N samples:                                                                      A = N - 1
2. The centred sum.  e_k = fl(x_k - mean^) carries one rounding, its square two; the fma chain rounds once per term (B terms at most after e_k joins, itself
   included), the tree (pooled kernel) 8 times, the division once.  Every term is >= 0, so the relative perturbations do not cancel:
   V^ = (1 + theta) * sum (x_k - mean^)^2 / (N - 1),  |theta| <= gamma_R,   R = 2 + B + T + 1   (pooled: B = ceil(N / 256), T = 8;  per chain: B = N, T = 0).
3. sum (x_k - mean^)^2 = (N - 1) V + N delta^2 exactly (sum (x_k - mu) = 0).  Together
   |V^ - V| <= gamma_R * V + (1 + gamma_R) * N / (N - 1) * delta^2.
   (The first-order form of the issue's starting point, (N / 256 + 10) u + N / (N - 1) delta^2 / V with delta = (N / 256 + 9) u sum|x| / N, counts one rounding
   fewer for the square of e_k and takes ceil(N / 256) as N / 256; ceil(N / 256) <= N / 256 + 1 gives R <= N / 256 + 12 and A + 1 <= N / 256 + 9.)
   The model is rounding without underflow or overflow: a dimension with spread 1e-170 (its squares underflow to 0) or one that holds an inf is outside it; the
   mirrors' answers there (variance 0 / NaN -> mass 1) are asserted as such.
4. The per-chain mass.  reg = (n V^ + c) / (n + 5) with c = the double 5e-3, then 1 / reg: a product, a sum of two positive terms, two divisions -- four more
   roundings, and n |V^ - V| / (n V + c) from the variance:  |mass^ - mass| / mass <= E / (1 - E),  E = n dV / (n V + c) + gamma_4."""
from fractions import Fraction

import numpy as np
import pytest

import mass_estimators_ref as ref
import orc

U = Fraction(1, 2 ** 53)
DOT = lambda a, b: orc.dot(np.ascontiguousarray(a), np.ascontiguousarray(b), 1)         # the oracle's fma chain


def gamma(k):
    return k * U / (1 - k * U)


def exact_variance(x):
    xs = [Fraction(float(v)) for v in x]
    n = len(xs)
    mu = sum(xs) / n
    return sum((v - mu) ** 2 for v in xs) / (n - 1), sum(abs(v) for v in xs)


def variance_bound(V, sum_abs, N, pooled):
    lane = -(-N // ref.LANES)
    A, R = (lane + 7, 2 + lane + 8 + 1) if pooled else (N - 1, 2 + N + 1)
    delta = gamma(A + 1) * sum_abs / N
    return gamma(R) * V + (1 + gamma(R)) * Fraction(N, N - 1) * delta ** 2


@pytest.mark.parametrize("C", ref.C_POOLED)
def test_pooled_variance_mirror_is_within_the_two_pass_bound(C):
    x = ref.pooled_input(C)
    var = ref.pooled_variance_ref(x, DOT)
    mass = ref.pooled_mass_ref(x, DOT)
    for name in ref.FINITE_DIMS:
        i = ref.DIMS.index(name)
        V, sum_abs = exact_variance(x[i])
        err, bound = abs(Fraction(float(var[i])) - V), variance_bound(V, sum_abs, C, pooled=True)
        print(f"C = {C} {name}: |var^ - var| / bound = {float(err / bound) if bound else 0.0:.3g}")
        assert err <= bound, (name, float(err), float(bound))
    i = ref.DIMS.index("constant")
    assert var[i] == 0.0 and mass[i] == 1.0                       # variance exactly 0 -> 1 / 0 = inf -> mass 1
    assert np.isnan(var[ref.DIMS.index("one_inf")]) and mass[ref.DIMS.index("one_inf")] == 1.0
    i = ref.DIMS.index("spread_1e-170")
    assert var[i] == 0.0 and mass[i] == 1.0                       # every square underflows; the reciprocal overflows
    for name in ("unit", "offset_1e8"):
        i = ref.DIMS.index(name)
        assert mass[i] == 1.0 / var[i] and 0.0 < mass[i] < np.inf


@pytest.mark.parametrize("n", ref.PART_LENGTHS)
def test_per_chain_mirror_is_within_the_two_pass_bound(n):
    x = ref.chain_input(n)
    var = ref.chain_variance_ref(x, DOT)
    mass = ref.chain_mass_ref(x, DOT)
    c5 = Fraction(5.0e-3)
    C = x.shape[2]
    for name in ref.FINITE_DIMS:
        i = ref.DIMS.index(name)
        for c in range(C):
            V, sum_abs = exact_variance(x[:, i, c])
            dV = variance_bound(V, sum_abs, n, pooled=False)
            assert abs(Fraction(float(var[i, c])) - V) <= dV, (name, c)
            M = (n + 5) / (n * V + c5)
            E = n * dV / (n * V + c5) + gamma(4)
            assert abs(Fraction(float(mass[i, c])) - M) <= M * E / (1 - E), (name, c)
    assert np.isfinite(mass).all() and (mass > 0).all()
    stuck = mass[:, 1]                                            # q = 0 (or the few ulps an inexact mean leaves): the regularised mass, finite
    assert stuck[ref.DIMS.index("constant")] == 1.0 / (5.0e-3 / (n + 5.0))
    assert np.all(stuck > 0.99 * (n + 5.0) / 5.0e-3) and np.all(stuck <= 1.0 / (5.0e-3 / (n + 5.0)))
    assert (mass[ref.DIMS.index("one_inf")][np.arange(C) != 1] == 1.0).all()       # a NaN variance -> mass 1
    assert np.all(mass[ref.DIMS.index("spread_1e-170")] == 1.0 / (5.0e-3 / (n + 5.0)))
