"""CPU: bridge sampling (mcmc_amd/bridge.py, the numpy statement of mi_mcmc_bridge_proposal / mi_mcmc_bridge_estimate / mi_mcmc_draws_bridge) against the
truth, the refusals of the three entries that need no device, and the mirror's own conventions.

(a) a dense Gaussian: log Z = 0.5 d log 2 pi - 0.5 log det P, exact i.i.d. draws, so the estimator's own error terms hold as they are: the bound is
    5 sqrt(cv1 + cv2), five standard errors of the estimate itself.
(b) a logistic regression with d = 2: log Z by trapezoid quadrature on a grid whose extent, doubled, moves log Z by less than 1e-8; draws from the CPU
    oracle's hmc, so the posterior term of the error carries N1 / ESS of f2 (mcmc_amd/ess.py): 5 sqrt(cv1 + (N1 / ESS) cv2).
Both run with NUMPY_MATH: the orders of the header over numpy's own functions.  Neither bound is tuned: it is the estimator's 5 sigma."""
import ctypes as C
import functools

import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import bridge, ess, psis, quantiles, synth, waic


@functools.lru_cache(maxsize=None)
def _gauss_case():
    d, n_keep, Cn = 5, 4, 500
    P = synth.dense_gaussian_precision(d)
    Lc = np.linalg.cholesky(np.linalg.inv(P))
    rng = np.random.default_rng(20240607)
    draws = np.einsum("ab,tbc->tac", Lc, rng.standard_normal((n_keep, d, Cn)))
    truth = 0.5 * d * bridge.LOG_2PI - 0.5 * np.linalg.slogdet(P)[1]
    return P, np.ascontiguousarray(draws), truth


def test_gaussian_truth_within_the_estimators_own_five_sigma():
    P, draws, truth = _gauss_case()
    res = bridge.bridge_ref(bridge.DENSE, draws, prec=P, seed=11)
    s = dict(zip(bridge.SUMMARY, res["summary"]))
    err, bound = abs(s["logml"] - truth), 5.0 * np.sqrt(s["cv1"] + s["cv2"])
    print(f"gaussian d=5: logml {s['logml']:.6f} truth {truth:.6f} error {err:.3e} bound {bound:.3e} it {int(s['it'])}")
    assert s["status"] == 0 and s["n_prop"] == 1000 and 1 <= s["it"] < 50
    assert err <= bound
    assert res["f2"].shape == (2, 500) and np.isfinite(res["f2"]).all()


def _logit_grid_logz(X, y, centre, half, n):
    """log of the trapezoid sum of exp(log-kernel) over centre +- half in both coordinates, n + 1 points each"""
    g0 = np.linspace(centre[0] - half[0], centre[0] + half[0], n + 1)
    g1 = np.linspace(centre[1] - half[1], centre[1] + half[1], n + 1)
    T0, T1 = np.meshgrid(g0, g1, indexing="ij")
    eta = T0[..., None] * X[:, 0] + T1[..., None] * X[:, 1]
    lk = (y * eta - np.logaddexp(0.0, eta)).sum(-1) - 0.5 * (T0 * T0 + T1 * T1)
    m = lk.max()
    w0 = np.full(n + 1, 1.0); w0[[0, -1]] = 0.5
    tot = np.einsum("i,ij,j->", w0, np.exp(lk - m), w0)
    return m + np.log(tot * (g0[1] - g0[0]) * (g1[1] - g1[0]))


def test_logistic_truth_by_quadrature_within_the_ess_corrected_five_sigma():
    d, n_rows, Cn, n_keep = 2, 30, 64, 40
    X, y = synth.logistic_problem(d, n_rows)
    spec = orc.TargetSpec(orc.TARGET_LOGISTIC, d, X=X, y=y, W=4)
    st = orc.make_settings(seed=5, n_burnin=100, n_keep=n_keep, n_leap=4, step=0.3)
    draws, _ = orc.run_many(orc.ALGO_HMC, spec, synth.initial_states(Cn, d), st)
    centre, sd = draws.mean(axis=(0, 2)), draws.std(axis=(0, 2))
    z_a = _logit_grid_logz(X, y, centre, 12.0 * sd, 480)
    z_b = _logit_grid_logz(X, y, centre, 24.0 * sd, 960)              # twice the extent, the same spacing
    print(f"logistic d=2: quadrature log Z {z_a:.10f} (12 sd), {z_b:.10f} (24 sd)")
    assert abs(z_a - z_b) < 1e-8
    res = bridge.bridge_ref(bridge.LOGISTIC, draws, X=X, y=y, seed=3)
    s = dict(zip(bridge.SUMMARY, res["summary"]))
    n_it = n_keep - n_keep // 2
    e = ess.ess_per_chain(res["f2"][:, None, :])[0]
    err, bound = abs(s["logml"] - z_b), 5.0 * np.sqrt(bridge.rel_mse(res["summary"], n_it, e))
    print(f"logistic d=2: logml {s['logml']:.6f} error {err:.3e} bound {bound:.3e} ESS per chain {e:.1f} of {n_it} it {int(s['it'])}")
    assert s["status"] == 0
    assert err <= bound


# ---- (c) the refusals, before any HIP call ----

def _needs_lib():
    import os
    if not os.path.exists(mcmc_amd.LIB_PATH):
        pytest.skip("libmi_mcmc.so not built (run __graft_entry__.build())")


def _rc_proposal(slab, n_keep, d, Cn, n_fit=0, n_prop=0, outs=True):
    info = np.zeros(2)
    return mcmc_amd.lib().mi_mcmc_bridge_proposal(None if slab is None else slab.ctypes.data, mcmc_amd.MEM_HOST, n_keep, d,
                                                  Cn, n_fit, n_prop, 1, None, None, None, None, None,
                                                  info.ctypes.data if outs else None, None)


def _rc_estimate(n_it, Cn, n_prop, n_eff=0.0, tol=0.0, null_input=False, outs=True):
    a = np.zeros(max(n_it * Cn, 1) if n_it * Cn < 1 << 20 else 1)
    b = np.zeros(max(n_prop, 1) if n_prop < 1 << 20 else 1)
    summ = np.zeros(8)
    p = lambda v: v.ctypes.data
    return mcmc_amd.lib().mi_mcmc_bridge_estimate(None if null_input else p(a), p(a), p(b), p(b), mcmc_amd.MEM_HOST, n_it, Cn,
                                                  n_prop, n_eff, tol, 0, None, p(summ) if outs else None, None)


def _rc_bridge(target, slab, n_keep, Cn, n_fit=0, n_prop=0, n_eff=0.0, tol=0.0, outs=True):
    summ = np.zeros(8)
    return mcmc_amd.lib().mi_mcmc_draws_bridge(None if target is None else C.byref(target), None if slab is None else slab.ctypes.data, mcmc_amd.MEM_HOST,
                                               n_keep, Cn, n_fit, n_prop, 1, n_eff, tol,
                                               0, None, None, None, summ.ctypes.data if outs else None, None)


def test_bad_arguments_are_refused_without_a_device():
    _needs_lib()
    BAD = mcmc_amd.MI_ERR_BAD_ARG
    slab = np.zeros((4, 3, 5))
    big = 1 << 32
    # mi_mcmc_bridge_proposal
    assert _rc_proposal(None, 4, 3, 5) == BAD                          # a NULL slab
    assert _rc_proposal(slab, 4, 3, 5, outs=False) == BAD              # all outputs NULL
    assert _rc_proposal(slab, 4, 0, 5) == BAD and _rc_proposal(slab, 4, 65537, 5) == BAD
    assert _rc_proposal(slab, 1, 3, 5) == BAD                          # n_keep < 2
    assert _rc_proposal(slab, 4, 3, 5, n_fit=4) == BAD and _rc_proposal(slab, 4, 3, 5, n_fit=7) == BAD
    assert _rc_proposal(slab, 2, 3, 1) == BAD                          # K0 = N1 = 1
    assert _rc_proposal(slab, 4, 3, 5, n_prop=1) == BAD                # N2 < 2
    assert _rc_proposal(slab, big, 3, 5) == BAD and _rc_proposal(slab, 4, 3, big) == BAD and _rc_proposal(slab, 4, 3, 5, n_prop=big) == BAD
    # mi_mcmc_bridge_estimate
    assert _rc_estimate(2, 5, 10, null_input=True) == BAD
    assert _rc_estimate(2, 5, 10, outs=False) == BAD
    assert _rc_estimate(1, 1, 10) == BAD                               # N1 < 2
    assert _rc_estimate(2, 5, 1) == BAD                                # N2 < 2
    assert _rc_estimate(big, 5, 10) == BAD and _rc_estimate(2, big, 10) == BAD and _rc_estimate(2, 5, big) == BAD
    for bad in (-1.0, float("nan")):
        assert _rc_estimate(2, 5, 10, tol=bad) == BAD and _rc_estimate(2, 5, 10, n_eff=bad) == BAD
    # mi_mcmc_draws_bridge
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_ISO, 3)
    assert _rc_bridge(None, slab, 4, 5) == BAD and _rc_bridge(t, None, 4, 5) == BAD
    assert _rc_bridge(t, slab, 4, 5, outs=False) == BAD
    assert _rc_bridge(t, slab, 1, 5) == BAD and _rc_bridge(t, slab, 4, 5, n_fit=4) == BAD and _rc_bridge(t, slab, 2, 1) == BAD
    assert _rc_bridge(t, slab, 4, 5, n_prop=1) == BAD and _rc_bridge(t, slab, big, 5) == BAD and _rc_bridge(t, slab, 4, big) == BAD
    for bad in (-1.0, float("nan")):
        assert _rc_bridge(t, slab, 4, 5, tol=bad) == BAD and _rc_bridge(t, slab, 4, 5, n_eff=bad) == BAD
    t.struct_size = 3
    assert _rc_bridge(t, slab, 4, 5) == BAD
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_ISO, 3)
    t.kind = 77
    assert _rc_bridge(t, slab, 4, 5) == BAD
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_ISO, 3)
    t.d = 0
    assert _rc_bridge(t, slab, 4, 5) == BAD
    t.d = 65537
    assert _rc_bridge(t, slab, 4, 5) == BAD
    # the two targets whose support is not R^d / that the reducers leave out: refused as unsupported, also without a device
    tn = mcmc_amd.make_target(mcmc_amd.TARGET_NORMAL_MODEL, 2, y=np.ones(4))
    assert _rc_bridge(tn, np.zeros((4, 2, 5)), 4, 5) == mcmc_amd.MI_ERR_UNSUPPORTED
    if mcmc_amd.lib().mi_mcmc_device_count() == 0:
        assert _rc_bridge(mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_ISO, 3), slab, 4, 5) == mcmc_amd.MI_ERR_NO_DEVICE      # no CPU path


# ---- (d) the mirror's conventions ----

def test_sump_is_the_body_fold_of_psis():
    rng = np.random.default_rng(1)
    v = np.exp(rng.standard_normal(2 * psis.BODY_PIECE + 777))
    want = np.float64(0.0)
    for e0 in range(0, v.size, psis.BODY_PIECE):
        want = want + psis.tree_sum(v[e0:e0 + psis.BODY_PIECE])
    assert bridge.sump(v) == want and bridge.PIECE == 16384
    assert bridge.sump(v[:300]) == psis.tree_sum(v[:300])


def test_the_median_is_quantiles_ref_and_the_moments_are_row_stats_merge():
    rng = np.random.default_rng(2)
    n_it, Cn = 3, 1501                                                 # 4 503 values: three chunks of 2 048, the last ragged
    lp1, lg1 = rng.standard_normal((n_it, Cn)), rng.standard_normal((n_it, Cn))
    lp2, lg2 = rng.standard_normal(700), rng.standard_normal(700)
    res = bridge.estimate_ref(lp1, lg1, lp2, lg2)
    s = dict(zip(bridge.SUMMARY, res["summary"]))
    assert s["lstar"] == quantiles.quantiles_ref((lp1 - lg1).reshape(n_it, 1, Cn), [0.5])[0, 0]
    assert s["lstar"] == np.median(lp1 - lg1)                          # (an odd count: the middle value itself)
    f2 = res["f2"]
    mean, M2 = bridge.moments(f2)
    _, p_waic = waic.row_stats(f2.reshape(1, -1))
    assert M2 / np.float64(f2.size - 1) == p_waic[0]                   # the same chunks, slots, tree and merge
    assert abs(mean - f2.mean()) < 1e-12 * abs(mean) + 1e-300
    assert s["cv2"] == (M2 / np.float64(f2.size - 1)) / ((mean * mean) * np.float64(f2.size))
    # the fixed point: r reproduces itself
    r = np.exp(s["logml"] - s["lstar"])
    a, b = np.exp((lp2 - lg2) - s["lstar"]), np.exp((lp1 - lg1).ravel() - s["lstar"])
    s1, s2 = 4503.0 / (4503.0 + 700.0), 700.0 / (4503.0 + 700.0)
    assert abs(np.mean(a / (s1 * a + s2 * r)) / np.mean(1.0 / (s1 * b + s2 * r)) / r - 1.0) < 1e-9
    assert s["status"] == 0 and s["rel"] <= 1e-10


def test_max_iter_and_non_finite_inputs_set_the_status():
    rng = np.random.default_rng(3)
    lp1, lg1, lp2, lg2 = rng.standard_normal((2, 40)), rng.standard_normal((2, 40)), rng.standard_normal(50), rng.standard_normal(50)
    s = dict(zip(bridge.SUMMARY, bridge.estimate_ref(lp1, lg1, lp2, lg2, max_iter=1)["summary"]))
    assert s["status"] == 2 and s["it"] == 1
    bad = lp1.copy(); bad[0, 0] = np.nan
    s = dict(zip(bridge.SUMMARY, bridge.estimate_ref(bad, lg1, lp2, lg2)["summary"]))
    assert s["status"] == 3 and np.isnan(s["logml"])
    gone = lp2.copy(); gone[3] = -np.inf                               # a proposal draw outside the support contributes 0
    s = dict(zip(bridge.SUMMARY, bridge.estimate_ref(lp1, lg1, gone, lg2)["summary"]))
    assert s["status"] == 0 and np.isfinite(s["logml"])


def test_a_singular_or_non_finite_fit_is_status_one():
    rng = np.random.default_rng(4)
    p = bridge.proposal_ref(rng.standard_normal((4, 17, 3)))           # K0 = 6 <= d
    assert p["status"] == 1 and np.isnan(p["prop"]).all() and np.isnan(p["logg_post"]).all() and np.isnan(p["mean"]).all()
    x = rng.standard_normal((4, 3, 20)); x[0, 1, 2] = np.nan
    assert bridge.proposal_ref(x)["status"] == 1
    x = rng.standard_normal((4, 3, 20)); x[3, 1, 2] = np.inf            # in the iteration part only: the fit stands
    p = bridge.proposal_ref(x)
    assert p["status"] == 0 and np.isfinite(p["logg_prop"]).all()
