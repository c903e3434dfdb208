"""mcmc_amd/csrc/settings_host.hpp -- the one host derivation of the bounds, mass and Sigma tables -- piece by piece against numpy, bit for bit
where IEEE defines the result exactly (tests/lit_host.hip: lit_host_settings).  LOG_DET is the project's own det_log: test_literal_replay_cpu.py
holds it against the oracle through lit_prepare, which is composed of these pieces."""
import numpy as np

import lit_host

D = 5
INF, NAN = np.inf, np.nan


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def test_bounds_types_follow_determine_bounds_type_and_a_nan_bound_is_not_finite():
    lower = np.array([-INF, -1.5, -INF, 0.25, NAN])
    upper = np.array([INF, INF, 2.0, 0.75, 3.0])
    o = lit_host.settings(D, lower=lower, upper=upper)
    assert o["bt"].tolist() == [1, 2, 3, 4, 3]
    assert _same(o["lb"], lower) and _same(o["ub"], upper)                 # the bounds themselves, NaN and infinities included
    o = lit_host.settings(D)                                               # vals_bound = 0
    assert o["bt"].tolist() == [1] * D and _same(o["lb"], np.zeros(D)) and _same(o["ub"], np.zeros(D))


def test_precond_kind_identity_diagonal_and_dense():
    diag = np.diag([2.0, 0.5, 3.0, 1.25, 7.0])
    assert lit_host.settings(D)["kind"] == 0
    assert lit_host.settings(D, precond=diag)["kind"] == 1
    neg_zero = diag.copy(); neg_zero[3, 1] = -0.0                          # -0.0 != 0.0 is false: still diagonal
    assert np.signbit(neg_zero[3, 1]) and lit_host.settings(D, precond=neg_zero)["kind"] == 1
    tiny = diag.copy(); tiny[4, 0] = 1e-300
    assert lit_host.settings(D, precond=tiny)["kind"] == 2


def test_diag_mass_is_the_elementwise_sqrt_and_reciprocal():
    v = np.array([2.0, 5e-324, 1e300, 0.3, 4.9e-310])                      # the smallest subnormal, a large value, another subnormal
    o = lit_host.settings(D, precond=np.diag(v))
    assert o["kind"] == 1
    with np.errstate(over="ignore"):
        assert _same(o["m"], v) and _same(o["m_sqrt"], np.sqrt(v)) and _same(o["m_inv"], 1.0 / v)
    assert np.isinf(o["m_inv"][1]) and np.isfinite(o["m_inv"][2])
    # the diagonal of a DENSE matrix gives the same tables (what the general kernel variants read next to INV / CHOL_LOWER)
    M = np.diag([2.0, 0.5, 3.0, 1.25, 7.0]); M[0, 1] = M[1, 0] = 0.25
    o = lit_host.settings(D, precond=M)
    assert o["kind"] == 2 and _same(o["m_sqrt"], np.sqrt(np.diag(M))) and _same(o["m_inv"], 1.0 / np.diag(M))
    assert np.allclose(o["Minv"] @ M, np.eye(D), atol=1e-14) and np.allclose(o["L"] @ o["L"].T, M, atol=1e-14) and np.array_equal(o["L"], np.tril(o["L"]))


def test_mala_sigma_of_a_diagonal_matrix():
    eps = 0.3
    m = np.array([2.0, 0.5, 3.0, 1.25, 7.0])
    o = lit_host.settings(D, eps=eps, precond=np.diag(m))
    assert _same(o["sinv_diag"], 1.0 / ((eps * eps) * m))
    assert _same(o["rs"], 1.0 / (eps * eps))
    assert _same(o["cons_term"], -0.5 * float(D) * 1.83787706640934548356)
    assert np.isclose(o["log_det"], np.sum(np.log((eps * eps) * m)), rtol=1e-13)      # (the bits: test_literal_replay_cpu.py, against the oracle)
    o0 = lit_host.settings(D, eps=eps)                                                # the identity: the same constants, no table
    assert _same(o0["rs"], o["rs"]) and _same(o0["cons_term"], o["cons_term"]) and np.all(np.isnan(o0["sinv_diag"]))


def test_padding_keeps_the_entries_and_fills_the_tail():
    lower = np.array([-INF, -1.5, -INF, 0.25, -2.0])
    upper = np.array([INF, INF, 2.0, 0.75, 3.0])
    m = np.array([2.0, 0.5, 3.0, 1.25, 7.0])
    for fill in (1.0, 0.0):
        o = lit_host.settings(D, lower=lower, upper=upper, precond=np.diag(m), n_padded=16, fill=fill)
        assert o["bt_padded"].tolist() == [1, 2, 3, 4, 4] + [1] * 11
        assert _same(o["m_sqrt_padded"][:D], np.sqrt(m)) and _same(o["m_sqrt_padded"][D:], np.full(11, fill))
