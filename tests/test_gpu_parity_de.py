"""GPU: mi_mcmc_de_run bit for bit against the CPU reference of mcmc::de (tests/de_ref.py) on both kernels."""
import ctypes as C

import numpy as np
import pytest

import mcmc_amd
import orc
import de_ref
from mcmc_amd import synth

pytestmark = pytest.mark.gpu

_ORC_KIND = {mcmc_amd.TARGET_GAUSS_ISO: orc.TARGET_ISO, mcmc_amd.TARGET_GAUSS_DIAG: orc.TARGET_DIAG,
             mcmc_amd.TARGET_GAUSS_DENSE: orc.TARGET_DENSE, mcmc_amd.TARGET_LOGISTIC: orc.TARGET_LOGISTIC}


def _init(P, d, seed):
    return np.random.default_rng(seed).normal(size=(P, d))


def _ref(kind, init, n_pop, nb, nk, seed, pops=None, population0=0, prec=None, X=None, y=None, lower=None, upper=None, **kw):
    d = init.shape[1]
    spec = de_ref.target_spec(_ORC_KIND[kind], d, prec=prec, X=X, y=y)
    out = []
    for p in (range(init.shape[0]) if pops is None else pops):
        out.append((p,) + de_ref.de_ref(spec, init[p], n_pop, nb, nk, seed=seed, pop=population0 + p, lower=lower, upper=upper, **kw))
    return out


def _check(kind, d, P, n_pop, nb, nk, seed=3, prec=None, X=None, y=None, lower=None, upper=None, jumps=False, initial_lb=None,
           initial_ub=None, hint=mcmc_amd.KERNEL_AUTO, pops=None, kernel=None):
    init = _init(P, d, seed + d)
    s = mcmc_amd.default_settings(rng_seed_value=seed, n_burnin_draws=nb, n_keep_draws=nk,
                                  **({} if lower is None else dict(vals_bound=1, lower_bounds=lower, upper_bounds=upper)))
    ds = mcmc_amd.de_settings(n_pop=n_pop, jumps=int(jumps), initial_lb=initial_lb, initial_ub=initial_ub)
    draws, info = mcmc_amd.de(kind, init, s, ds, prec=prec, X=X, y=y, kernel_hint=hint)
    if kernel is not None:
        assert mcmc_amd.last_kernel().startswith(kernel), mcmc_amd.last_kernel()
    for p, rd, rX, racc in _ref(kind, init, n_pop, nb, nk, seed, pops=pops, prec=prec, X=X, y=y, lower=lower, upper=upper, jumps=jumps,
                                initial_lb=initial_lb, initial_ub=initial_ub):
        assert np.array_equal(draws[..., p], rd, equal_nan=True), f"population {p}: draws"
        assert np.array_equal(info["population"][..., p], rX, equal_nan=True), f"population {p}: population"
        assert int(info["n_accept"][p]) == racc, f"population {p}: n_accept"
    return draws, info


def test_iso_d3():
    _check(mcmc_amd.TARGET_GAUSS_ISO, 3, 20, 5, 3, 4, kernel="de_gauss_mfma_kernel<1, false>")


def test_dense_d128():
    _check(mcmc_amd.TARGET_GAUSS_DENSE, 128, 16, 4, 2, 2, prec=synth.dense_gaussian_precision(128), kernel="de_gauss_mfma_kernel<8, false>")


def test_dense_d100_ragged_tile():
    _check(mcmc_amd.TARGET_GAUSS_DENSE, 100, 37, 3, 2, 3, prec=synth.dense_gaussian_precision(100), pops=[0, 15, 16, 31, 36])


def test_diag_d40_bounded():
    d = 40
    prec = np.linspace(0.5, 3.0, d)
    lower = np.where(np.arange(d) % 3 == 0, -1.0, -np.inf)
    upper = np.where(np.arange(d) % 4 == 0, 1.5, np.inf)
    _check(mcmc_amd.TARGET_GAUSS_DIAG, d, 20, 4, 2, 3, prec=prec, lower=lower, upper=upper, kernel="de_gauss_mfma_kernel<4, true>")


def test_dense_d200_on_the_literal_kernel():
    _check(mcmc_amd.TARGET_GAUSS_DENSE, 200, 4, 3, 1, 2, prec=synth.dense_gaussian_precision(200), kernel="de_literal_kernel")


@pytest.mark.parametrize("d", [8, 64])
def test_logistic_on_the_literal_kernel(d):
    rng = np.random.default_rng(d)
    X = rng.normal(size=(40, d)) / np.sqrt(d)
    y = (rng.random(40) < 0.5).astype(np.float64)
    _check(mcmc_amd.TARGET_LOGISTIC, d, 4, 4, 2, 2, X=X, y=y, kernel="de_literal_kernel")


def test_jumps():
    _check(mcmc_amd.TARGET_GAUSS_ISO, 3, 8, 4, 5, 8, jumps=True)


def test_huge_initial_box_gives_nonfinite_values():
    d = 4
    draws, info = _check(mcmc_amd.TARGET_GAUSS_ISO, d, 8, 5, 1, 3, initial_lb=np.full(d, -1e300), initial_ub=np.full(d, 1e300))
    assert np.abs(info["population"]).max() > 1e160                  # x^2 overflows: the members start at -inf


def test_literal_hint_gives_the_same_bits():
    d = 24
    prec = synth.dense_gaussian_precision(d)
    init = _init(12, d, 1)
    lower, upper = np.full(d, -2.0), np.full(d, np.inf)
    s = mcmc_amd.default_settings(rng_seed_value=5, n_burnin_draws=3, n_keep_draws=4, vals_bound=1, lower_bounds=lower, upper_bounds=upper)
    ds = mcmc_amd.de_settings(n_pop=6)
    a, ia = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_DENSE, init, s, ds, prec=prec)
    assert mcmc_amd.last_kernel() == "de_gauss_mfma_kernel<2, true>"
    b, ib = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_DENSE, init, s, ds, prec=prec, kernel_hint=mcmc_amd.KERNEL_LITERAL)
    assert mcmc_amd.last_kernel() == "de_literal_kernel"
    assert np.array_equal(a, b) and np.array_equal(ia["population"], ib["population"]) and np.array_equal(ia["n_accept"], ib["n_accept"])


def test_sharding_by_population0():
    d, P = 5, 40
    init = _init(P, d, 2)
    s = mcmc_amd.default_settings(rng_seed_value=8, n_burnin_draws=2, n_keep_draws=3)
    ds = mcmc_amd.de_settings(n_pop=4)
    a, ia = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_ISO, init, s, ds)
    b1, i1 = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_ISO, init[:17], s, ds)
    b2, i2 = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_ISO, init[17:], s, ds, population0=17)
    assert np.array_equal(a, np.concatenate([b1, b2], axis=-1))
    assert np.array_equal(ia["n_accept"], np.concatenate([i1["n_accept"], i2["n_accept"]]))


@pytest.mark.parametrize("bounded", [False, True])
def test_cut_run_equals_the_uncut_run(bounded):
    d, P = 6, 10
    init = _init(P, d, 4)
    bk = dict(vals_bound=1, lower_bounds=np.full(d, -1.0), upper_bounds=np.full(d, 2.0)) if bounded else {}
    ds = mcmc_amd.de_settings(n_pop=5, jumps=1)
    full, ifull = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_ISO, init, mcmc_amd.default_settings(rng_seed_value=2, n_burnin_draws=4, n_keep_draws=9, **bk), ds)
    a, ia = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_ISO, init, mcmc_amd.default_settings(rng_seed_value=2, n_burnin_draws=4, n_keep_draws=3, **bk), ds)
    b, ib = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_ISO, init, mcmc_amd.default_settings(rng_seed_value=2, n_burnin_draws=0, n_keep_draws=6, **bk), ds,
                        draw0=7, population=ia["population"])
    assert np.array_equal(full, np.concatenate([a, b]))
    assert np.array_equal(ifull["population"], ib["population"])
    assert np.array_equal(ifull["n_accept"], ia["n_accept"] + ib["n_accept"])


def test_without_draws():
    init = _init(9, 7, 5)
    s = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=2, n_keep_draws=3)
    ds = mcmc_amd.de_settings(n_pop=4)
    a, ia = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_ISO, init, s, ds)
    b, ib = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_ISO, init, s, ds, want_draws=False)
    assert b is None and np.array_equal(ia["population"], ib["population"]) and np.array_equal(ia["n_accept"], ib["n_accept"])


def test_device_memory():
    import torch
    d, P, n_pop, nk = 16, 24, 5, 3
    init = _init(P, d, 6)
    s = mcmc_amd.default_settings(rng_seed_value=6, n_burnin_draws=2, n_keep_draws=nk)
    ds = mcmc_amd.de_settings(n_pop=n_pop)
    ref, iref = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_ISO, init, s, ds)
    dev = torch.device("cuda", 0)
    iv = torch.as_tensor(np.ascontiguousarray(init.T), device=dev)
    pop = torch.zeros((n_pop, d, P), dtype=torch.float64, device=dev)
    draws = torch.zeros((nk, n_pop, d, P), dtype=torch.float64, device=dev)
    acc = torch.zeros(P, dtype=torch.int64, device=dev)
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_ISO, d)
    p = mcmc_amd.mi_populations()
    p.struct_size, p.mem, p.n_populations = C.sizeof(mcmc_amd.mi_populations), mcmc_amd.MEM_DEVICE, P
    p.initial_vals, p.population, p.draws, p.n_accept = iv.data_ptr(), pop.data_ptr(), draws.data_ptr(), acc.data_ptr()
    st = torch.cuda.current_stream(dev).cuda_stream
    assert mcmc_amd.lib().mi_mcmc_de_run(C.byref(t), C.byref(s), C.byref(ds), C.byref(p), st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(draws.cpu().numpy(), ref) and np.array_equal(pop.cpu().numpy(), iref["population"])
    assert np.array_equal(acc.cpu().numpy().astype(np.uint64), iref["n_accept"])


def test_full_width_d128():
    """16 384 populations in one call; four of them (both ends of the grid, a tile edge) re-run by the reference"""
    d, P = 128, 16384
    prec = synth.dense_gaussian_precision(d)
    _check(mcmc_amd.TARGET_GAUSS_DENSE, d, P, 3, 1, 2, prec=prec, pops=[0, 63, 64, P - 1], kernel="de_gauss_mfma_kernel<8, false>")
