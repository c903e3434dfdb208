"""GPU: mcmc::aees (mi_mcmc_aees_run) bit for bit against the CPU transcription tests/aees_ref.py -- draws, final states of every level,
and both counters."""
import ctypes as C

import numpy as np
import pytest

import mcmc_amd
import orc
import aees_ref
import de_ref
from mcmc_amd import synth

pytestmark = pytest.mark.gpu

MIX_MEANS = np.array([[-2.0, -2.0], [2.0, 2.0]])
MIX_VARS = np.array([0.1, 0.1])
MIX_W = np.array([0.5, 0.5])


def _init(P, d, seed):
    return np.random.default_rng(seed).normal(size=(P, d))


def _target(kind, d, prec=None, X=None, y=None):
    """(device target, reference log kernel)"""
    if kind == mcmc_amd.TARGET_GAUSS_MIXTURE:
        return mcmc_amd.mixture_target(MIX_MEANS, MIX_VARS, MIX_W), aees_ref.mixture_fn(MIX_MEANS, MIX_VARS, MIX_W)
    okind = {mcmc_amd.TARGET_GAUSS_ISO: orc.TARGET_ISO, mcmc_amd.TARGET_GAUSS_DIAG: orc.TARGET_DIAG,
             mcmc_amd.TARGET_GAUSS_DENSE: orc.TARGET_DENSE, mcmc_amd.TARGET_LOGISTIC: orc.TARGET_LOGISTIC}[kind]
    return mcmc_amd.make_target(kind, d, prec=prec, X=X, y=y), de_ref.target_spec(okind, d, prec=prec, X=X, y=y)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check(kind, init, seed, n_initial, n_burnin, n_keep, runs=None, lower=None, upper=None, prec=None, X=None, y=None, run0=0, **kw):
    """one call over every row of init; the runs listed (default: all) re-run by the reference"""
    P, d = init.shape
    s = mcmc_amd.default_settings(rng_seed_value=seed, n_burnin_draws=n_burnin, n_keep_draws=n_keep)
    if lower is not None:
        s.vals_bound = 1
        lb, ub = np.ascontiguousarray(lower, dtype=np.float64), np.ascontiguousarray(upper, dtype=np.float64)
        s.lower_bounds, s.upper_bounds = lb.ctypes.data, ub.ctypes.data
    a = mcmc_amd.aees_settings(n_initial_draws=n_initial, **kw)
    t, ref_kernel = _target(kind, d, prec=prec, X=X, y=y)
    draws, info = mcmc_amd.aees(t, init, s, a, run0=run0)
    assert mcmc_amd.last_kernel() == "aees_literal_kernel"
    rk = {k: v for k, v in kw.items() if k in ("par_scale", "cov_mat", "n_rings", "temper_vec")}
    if "ee_prob_par" in kw:
        rk["ee_prob"] = kw["ee_prob_par"]
    for r in (range(P) if runs is None else runs):
        rd, rX, racc, ree = aees_ref.aees_ref(ref_kernel, init[r], n_burnin, n_keep, seed=seed, run=run0 + r, lower=lower, upper=upper,
                                              n_initial=n_initial, **rk)
        assert _same(draws[..., r], rd), f"run {r}: draws differ"
        assert _same(info["final_states"][..., r], rX), f"run {r}: final states differ"
        assert np.array_equal(info["n_accept"][:, r], racc) and np.array_equal(info["n_ee_accept"][:, r], ree), f"run {r}: counters differ"
    return draws, info


def test_iso_four_levels():
    _check(mcmc_amd.TARGET_GAUSS_ISO, _init(3, 3, 1), 5, 6, 4, 40, temper_vec=[2.0, 5.0, 3.5], n_rings=5, ee_prob_par=0.3)


def test_diag_two_levels_dense_cov():
    d = 4
    prec = np.array([1.0, 2.0, 0.5, 4.0])
    cov = np.array([[1.0, 0.3, 0.0, 0.1], [0.3, 2.0, 0.2, 0.0], [0.0, 0.2, 0.5, 0.1], [0.1, 0.0, 0.1, 1.5]])
    _check(mcmc_amd.TARGET_GAUSS_DIAG, _init(3, d, 2), 7, 10, 5, 60, prec=prec, temper_vec=[8.0], n_rings=2, ee_prob_par=0.05,
           cov_mat=cov, par_scale=0.7)


def test_dense_bounds_ee_always():
    d = 5
    prec = synth.dense_gaussian_precision(d)
    lower = np.array([-1.0, -np.inf, 0.0, -2.0, -np.inf])
    upper = np.array([1.0, 0.5, np.inf, 2.0, np.inf])
    init = np.clip(_init(3, d, 3) * 0.3, -0.4, 0.4) + np.array([0.0, 0.0, 0.5, 0.0, 0.0])
    _check(mcmc_amd.TARGET_GAUSS_DENSE, init, 9, 8, 4, 30, prec=prec, lower=lower, upper=upper, temper_vec=[4.0, 16.0, 2.0], n_rings=11,
           ee_prob_par=1.0)


def test_logistic_no_ee():
    d, n = 3, 20
    rng = np.random.default_rng(4)
    X = rng.normal(size=(n, d))
    y = (rng.random(n) < 0.5).astype(np.float64)
    _check(mcmc_amd.TARGET_LOGISTIC, _init(2, d, 4) * 0.2, 11, 5, 5, 30, X=X, y=y, temper_vec=[3.0], n_rings=5, ee_prob_par=0.0)


def test_mixture_example_settings():
    init = np.tile(MIX_MEANS[0], (4, 1))
    _, info = _check(mcmc_amd.TARGET_GAUSS_MIXTURE, init, 13, 40, 40, 200, temper_vec=[60.0, 9.0], n_rings=11, ee_prob_par=0.05,
                     cov_mat=0.35 * np.eye(2))
    assert info["n_ee_accept"][1:].sum() > 0


def test_one_level_and_one_ring():
    _check(mcmc_amd.TARGET_GAUSS_ISO, _init(3, 2, 5), 17, 5, 5, 30, n_rings=1)


def test_no_initial_draws_one_ring():
    """S = 0: every level is active from draw 1 on, and with one ring ind_mix = n happens (the unwritten entry: zeros)"""
    _check(mcmc_amd.TARGET_GAUSS_MIXTURE, np.tile(MIX_MEANS[1], (3, 1)), 19, 0, 0, 80, temper_vec=[6.0, 3.0], n_rings=1, ee_prob_par=0.5)


def test_nonfinite_starts():
    init = np.array([[np.inf, 0.0, 1.0], [np.nan, 0.5, 0.0], [-np.inf, np.inf, np.nan], [0.1, 0.2, 0.3]])
    _check(mcmc_amd.TARGET_GAUSS_ISO, init, 23, 4, 4, 25, temper_vec=[5.0, 2.0], n_rings=3, ee_prob_par=0.4)


def test_sharding_by_run0():
    """runs 0..5 in one call equal runs 0..2 and 3..5 in two calls (run0 = 3)"""
    init = _init(6, 2, 7)
    kw = dict(temper_vec=[10.0, 3.0], n_rings=4, ee_prob_par=0.2)
    s = mcmc_amd.default_settings(rng_seed_value=29, n_burnin_draws=5, n_keep_draws=40)
    t = mcmc_amd.mixture_target(MIX_MEANS, MIX_VARS, MIX_W)
    a = mcmc_amd.aees_settings(n_initial_draws=5, **kw)
    full, fi = mcmc_amd.aees(t, init, s, a)
    lo, li = mcmc_amd.aees(t, init[:3], s, a)
    hi, hi_i = mcmc_amd.aees(t, init[3:], s, a, run0=3)
    assert _same(np.concatenate([lo, hi], axis=-1), full)
    for key in ("final_states", "n_accept", "n_ee_accept"):
        assert _same(np.concatenate([li[key], hi_i[key]], axis=-1), fi[key])
    _check(mcmc_amd.TARGET_GAUSS_MIXTURE, init[4:5], 29, 5, 5, 40, run0=4, **kw)


def test_device_memory():
    import torch
    d, P, nk = 2, 8, 30
    init = _init(P, d, 8)
    s = mcmc_amd.default_settings(rng_seed_value=31, n_burnin_draws=5, n_keep_draws=nk)
    a = mcmc_amd.aees_settings(n_initial_draws=5, temper_vec=[4.0, 2.0], n_rings=3, ee_prob_par=0.3)
    K = 3
    ref, iref = mcmc_amd.aees(mcmc_amd.TARGET_GAUSS_ISO, init, s, a)
    dev = torch.device("cuda", 0)
    iv = torch.as_tensor(np.ascontiguousarray(init.T), device=dev)
    draws = torch.zeros((nk, d, P), dtype=torch.float64, device=dev)
    fin = torch.zeros((K, d, P), dtype=torch.float64, device=dev)
    acc = torch.zeros((K, P), dtype=torch.int64, device=dev)
    ee = torch.zeros((K, P), dtype=torch.int64, device=dev)
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_ISO, d)
    r = mcmc_amd.mi_aees_runs()
    r.struct_size, r.mem, r.n_runs = C.sizeof(mcmc_amd.mi_aees_runs), mcmc_amd.MEM_DEVICE, P
    r.initial_vals, r.draws, r.final_states = iv.data_ptr(), draws.data_ptr(), fin.data_ptr()
    r.n_accept, r.n_ee_accept = acc.data_ptr(), ee.data_ptr()
    st = torch.cuda.current_stream(dev).cuda_stream
    assert mcmc_amd.lib().mi_mcmc_aees_run(C.byref(t), C.byref(s), C.byref(a), C.byref(r), st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(draws.cpu().numpy(), ref) and np.array_equal(fin.cpu().numpy(), iref["final_states"])
    assert np.array_equal(acc.cpu().numpy().astype(np.uint64), iref["n_accept"])
    assert np.array_equal(ee.cpu().numpy().astype(np.uint64), iref["n_ee_accept"])


def test_long_windows_with_ties():
    """windows of several thousand values, many of them equal (a hot level that rejects most of its moves repeats its value): the
    lazy merge against the full stable sort of every step"""
    init = np.tile(MIX_MEANS[0], (2, 1))
    _, info = _check(mcmc_amd.TARGET_GAUSS_MIXTURE, init, 37, 2000, 500, 300, temper_vec=[400.0, 30.0], n_rings=7, ee_prob_par=0.08,
                     par_scale=3.0)
    assert info["n_ee_accept"][2].sum() > 0


def test_many_runs_sampled():
    """4 096 runs in one call (more runs than workgroups: slots are reused); a sample re-run by the reference"""
    P = 4096
    init = np.tile(MIX_MEANS[0], (P, 1)) + _init(P, 2, 9) * 0.1
    _check(mcmc_amd.TARGET_GAUSS_MIXTURE, init, 41, 20, 20, 60, runs=[0, 1, 2047, 2048, 4095], temper_vec=[60.0, 9.0], n_rings=11,
           ee_prob_par=0.05, cov_mat=0.35 * np.eye(2))
