"""No GPU: the host arithmetic that mi_mcmc_draw_stats and mi_mcmc_draw_stats_lags share (mcmc_amd/csrc/draw_stats_host.hpp), through the hook
mi_mcmc_test_stats_host.  Geyer's sum and R-hat are the same IEEE double operations in the same order as their Python statements here and in
mcmc_amd/acov.py, and the library is built with -ffp-contract=off, so every comparison is of bytes.

(An AR(1) series with phi = -0.6 has rho_0 + rho_1 = 0.4: its sum does not stop at lag 0, it stops where the sample noise of the later, small pairs
says.  The column STOP_AT_0 below is the one whose first pair is non-positive.)"""
import math

import numpy as np
import pytest

import draw_stats_ref as R
import mcmc_amd
from mcmc_amd import acov as A

SHAPES = ((3, 2, 5), (4, 2, 5), (17, 3, 8), (40, 3, 8))
PHIS = (0.0, 0.5, 0.95, -0.6)
RHAT_SHAPES = ((1, 2, 10, 1), (1, 2, 10, 7), (3, 4, 50, 130))          # G, d, n, C


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def met_of(acov_j, n, K):
    """geyer_window's `met`: its second value without the K == n - 1 term (and False for n < 4, where the loop does not run)"""
    den = acov_j[0] if acov_j[0] > 0 else 1.0
    return n >= 4 and any(acov_j[t] / den + acov_j[t + 1] / den <= 0 for t in range(0, K, 2))       # t + 1 <= K; the loop stops at the first one


def check_geyer(acov, n):
    """every prefix of lags the issue names, every dimension: ess in bytes, hit as the loop's met"""
    d = acov.shape[1]
    for known in sorted({1, 2, 3, n - 1, n}):
        if not 1 <= known <= n:
            continue
        got = mcmc_amd.test_stats_host(acov=acov[:known], n=n)
        for j in range(d):
            with np.errstate(invalid="ignore"):
                ess, ended = A.geyer_window(acov[:, j], n, known - 1)
                met = met_of(acov[:, j], n, known - 1)
            assert ended == int(met or known - 1 == n - 1 or n < 4)
            assert bits(got["ess"][j]) == bits(ess), (n, known, j, got["ess"][j], ess)
            assert got["hit"][j] == int(met), (n, known, j)
    assert got["rhat"] is None


@pytest.mark.parametrize("phi", PHIS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_geyer_sum_has_the_bytes_of_the_python_loop(shape, phi):
    n, d, C = shape
    check_geyer(A.acov_ref(R.ar1(n, d, C, phi, seed=n + C)), n)


def test_geyer_sum_of_the_odd_columns():
    """acov_0 = 0 (den = 1), a first pair that is non-positive, and a NaN among the lags: whatever the Python loop gives, in bytes"""
    n = 17
    acov = np.array(A.acov_ref(R.ar1(n, 3, 8, 0.5, seed=n)))
    acov[0, 0] = 0.0
    acov[1, 1] = -1.5 * acov[0, 1]                      # STOP_AT_0
    acov[4, 2] = np.nan
    check_geyer(acov, n)
    got = mcmc_amd.test_stats_host(acov=acov, n=n)
    assert got["hit"][1] == 1 and got["ess"][1] == n    # tau stays -1: ess = n


def rhat_py(mp, n, C):
    """draw_stats_host.hpp's expression in Python floats, the groups added in ascending g"""
    G, d, _ = mp.shape
    out = np.zeros(d)
    for j in range(d):
        sm = sm2 = sv = 0.0
        for g in range(G):
            sm += float(mp[g, j, 0]); sm2 += float(mp[g, j, 1]); sv += float(mp[g, j, 2])
        W = sv / float(C)
        mbar = sm / float(C)
        B_over_n = (sm2 - float(C) * mbar * mbar) / float(C - 1) if C > 1 else 0.0
        var_plus = (float(n - 1) / float(n)) * W + B_over_n
        out[j] = math.sqrt(var_plus / W) if W > 0.0 else 1.0
    return out


def moments(G, d, n, C, seed):
    """[G][d][3]: sums over the chains of group g (ranges of ceil(C / G) chains) of a chain mean, its square and a chain variance"""
    rng = np.random.default_rng(seed)
    m, v = rng.standard_normal((d, C)) / np.sqrt(n) + 3.0, rng.chisquare(n - 1, (d, C)) / (n - 1)
    per = (C + G - 1) // G
    return np.stack([np.stack([m[:, g * per:(g + 1) * per].sum(axis=1), (m[:, g * per:(g + 1) * per] ** 2).sum(axis=1), v[:, g * per:(g + 1) * per].sum(axis=1)],
                              axis=1) for g in range(G)])


@pytest.mark.parametrize("shape", RHAT_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_rhat_has_the_bytes_of_the_expression(shape):
    G, d, n, C = shape
    mp = moments(G, d, n, C, seed=C)
    assert mp.shape == (G, d, 3)
    mp[:, d - 1, 2] = 0.0                               # a dimension whose chains do not move: W = 0
    got = mcmc_amd.test_stats_host(n=n, moments=mp, n_chains=C)
    want = rhat_py(mp, n, C)
    assert np.array_equal(bits(got["rhat"]), bits(want)), (got["rhat"], want)
    assert got["rhat"][d - 1] == 1.0 and got["ess"] is None and got["hit"] is None
    if C == 1:                                          # B_over_n = 0: R-hat is sqrt(((n - 1) / n W) / W)
        assert np.all(got["rhat"][:d - 1] < 1.0)


def test_both_at_once_and_the_symbol():
    n, C = 40, 8
    acov = A.acov_ref(R.ar1(n, 4, C, 0.5, seed=1))
    mp = moments(3, 4, n, C, seed=2)
    both = mcmc_amd.test_stats_host(acov=acov, n=n, moments=mp, n_chains=C)
    assert np.array_equal(bits(both["ess"]), bits(mcmc_amd.test_stats_host(acov=acov, n=n)["ess"]))
    assert np.array_equal(bits(both["rhat"]), bits(rhat_py(mp, n, C)))
    assert hasattr(mcmc_amd.lib(), "mi_mcmc_test_stats_host")
