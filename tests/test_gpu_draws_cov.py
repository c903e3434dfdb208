"""GPU: mi_mcmc_draws_covariance -- pooled mean and covariance of a draws slab [n_keep][d][C] on the matrix cores (draws_cov.hip).

Accuracy is checked against exact arithmetic (a two-pass covariance in np.longdouble) with DERIVED bounds, every element of every case:
  |cov_ij - ref_ij| <= (K + 64) 2^-52 sum_k |e_ik e_jk| / (K - 1)   twice the standard gamma_K bound of a length-K fma sum of once-rounded
                                                                   operands; the mean's own error enters at second order (sum_k e_jk = 0)
  |mean_i - mu_i|   <= (K + 2) 2^-53 mean_k |x_ik|
(numpy's own float64 np.cov / mean stay below 0.015 resp. 0.21 of them on these inputs; the covariance bound is <= 5e-12 relative on the
diagonal while one dropped or doubled sample moves an element by >= 1 / K ~ 5e-5.)  The bound's own sum of magnitudes is taken in float64.
The kernel walks no persistent grid -- one workgroup per (tile, chunk), both functions of the shape --, so there is no grid cap to vary.
The covariance bound holds for inputs whose mean error is negligible against the spread, as these are; tests/test_covariance_ref_cpu.py derives and
checks the extended bound (+ K / (K - 1) mean_bound_i mean_bound_j) that holds at any offset.

BIT FOR BIT (the second half of this file): mean and covariance are compared as uint64, any NaN matching any NaN, with mcmc_amd/covariance.py -- the
numpy statement of include/mi_mcmc.h's definition and of every reduction order in it -- run over the CPU oracle's fma chain (orc.dot(x, y, 1)).  No
tolerance there: a wrong summation order, a swapped chunk, a partial not started from +0, padding entered as 0 - mu or a sample read twice changes
bits (tests/test_covariance_ref_cpu.py measures how many).  tests/draws_cov_cases.py lists the shapes and what each reaches; the mirror covers the
full matrix except at (1, 200, 20000) and (1, 520, 512), where it covers the corners and random elements of EVERY tile."""
import functools

import numpy as np
import pytest

import draws_cov_cases as cases
import mcmc_amd

pytestmark = pytest.mark.gpu

SHAPES = cases.SHAPES            # the bound tests' inputs, as ever
_slab = cases.slab


@functools.lru_cache(maxsize=None)
def _case(shape):
    """slab, exact reference with its bounds, and ONE engine call -- shared by the tests, never modified"""
    n_keep, d, C = shape
    K = n_keep * C
    slab = _slab(n_keep, d, C)
    x = slab.transpose(1, 0, 2).reshape(d, K).astype(np.longdouble)
    mu = x.sum(axis=1) / K
    e = x - mu[:, None]
    ref = (e @ e.T) / (K - 1)
    ea = np.abs(e).astype(np.float64)
    cov_bound = (K + 64) * 2.0 ** -52 * (ea @ ea.T) / (K - 1)
    mean_bound = (K + 2) * 2.0 ** -53 * np.abs(x).mean(axis=1).astype(np.float64)
    mean, cov = mcmc_amd.draws_covariance(slab)
    for a in (slab, mean, cov):
        a.setflags(write=False)
    return dict(slab=slab, mu=mu, ref=ref, cov_bound=cov_bound, mean_bound=mean_bound, mean=mean, cov=cov)


def _worst(got, ref, bound):
    return float((np.abs(got.astype(np.longdouble) - ref) / bound).max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mean_and_covariance_meet_the_derived_bounds_in_every_element(shape):
    c = _case(shape)
    wc, wm = _worst(c["cov"], c["ref"], c["cov_bound"]), _worst(c["mean"], c["mu"], c["mean_bound"])
    print(f"(n_keep, d, C) = {shape}: worst |cov - ref| / bound {wc:.4f}, worst |mean - mu| / bound {wm:.4f}")
    assert np.isfinite(c["cov"]).all() and np.isfinite(c["mean"]).all()
    assert (np.abs(c["cov"].astype(np.longdouble) - c["ref"]) <= c["cov_bound"]).all()
    assert (np.abs(c["mean"].astype(np.longdouble) - c["mu"]) <= c["mean_bound"]).all()
    assert np.array_equal(c["cov"], c["cov"].T)                                          # exactly symmetric


@pytest.mark.parametrize("shape", [(3, 130, 333), (1, 200, 20000)], ids=lambda s: "x".join(map(str, s)))
def test_bits_do_not_depend_on_the_call(shape):
    import torch
    c = _case(shape)
    n_keep, d, C = shape
    mean2, cov2 = mcmc_amd.draws_covariance(c["slab"])                                   # a second call
    assert np.array_equal(mean2, c["mean"]) and np.array_equal(cov2, c["cov"])
    dev = torch.from_numpy(c["slab"].copy()).cuda()                                             # the same slab in device memory
    mean3, cov3 = mcmc_amd.draws_covariance(dev, n_keep, d, C, mem=mcmc_amd.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(mean3, c["mean"]) and np.array_equal(cov3, c["cov"])
    mean4, none_cov = mcmc_amd.draws_covariance(c["slab"], want_cov=False)               # one output alone
    none_mean, cov4 = mcmc_amd.draws_covariance(c["slab"], want_mean=False)
    assert none_cov is None and none_mean is None
    assert np.array_equal(mean4, c["mean"]) and np.array_equal(cov4, c["cov"])


def test_the_chains_state_is_the_case_n_keep_1():
    c = _case((1, 130, 333))
    mean, cov = mcmc_amd.draws_covariance(c["slab"][0])                                  # [d][C], as mi_chains.theta
    assert np.array_equal(mean, c["mean"]) and np.array_equal(cov, c["cov"])


def test_non_finite_samples_stay_in_their_rows_and_columns():
    shape = (3, 130, 333)
    c = _case(shape)
    slab = c["slab"].copy()
    i_nan, i_inf = 7, 100
    slab[1, i_nan, 5] = np.nan
    slab[2, i_inf, 300] = np.inf
    mean, cov = mcmc_amd.draws_covariance(slab)
    bad = np.zeros(shape[1], dtype=bool)
    bad[[i_nan, i_inf]] = True
    assert np.array_equal(~np.isfinite(mean), bad)
    assert np.array_equal(~np.isfinite(cov), bad[:, None] | bad[None, :])
    ok = ~(bad[:, None] | bad[None, :])
    assert (np.abs(cov.astype(np.longdouble) - c["ref"]) <= c["cov_bound"])[ok].all()
    assert (np.abs(mean.astype(np.longdouble) - c["mu"]) <= c["mean_bound"])[~bad].all()
    assert np.array_equal(cov[ok], c["cov"][ok]) and np.array_equal(mean[~bad], c["mean"][~bad])     # the other elements: the clean call's bits


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# bit for bit against the mirror of the header's order (mcmc_amd/covariance.py over orc.dot(x, y, 1)); the references are tests/draws_cov_cases.py's


@functools.lru_cache(maxsize=None)
def _run(shape):
    """ONE two-output engine call on the shape's slab -- shared, read-only; the bound tests' call where there is one"""
    if shape in SHAPES:
        c = _case(shape)
        return c["mean"], c["cov"]
    mean, cov = mcmc_amd.draws_covariance(cases.frozen_slab(shape))
    mean.setflags(write=False)
    cov.setflags(write=False)
    return mean, cov


@pytest.mark.parametrize("shape", SHAPES + cases.NEW_SHAPES, ids=cases.shape_id)
def test_mean_and_covariance_are_the_mirror_bit_for_bit(shape):
    mean, cov = _run(shape)
    ref = cases.reference(shape)
    d = shape[1]
    assert mean.shape == (d,) and cov.shape == (d, d)
    if ref["elements"] is not None:                                                       # sampled: every tile with tj <= ti is in the sample
        assert {(i // 128, j // 128) for i, j in ref["elements"]} == set(cases.tiles(d)) and len(ref["elements"]) >= 5 * len(cases.tiles(d))
    cases.assert_is_the_mirror(mean, cov, ref, shape)
    assert np.array_equal(cases.bits(cov), cases.bits(cov.T))                             # symmetric bit for bit
    assert np.isfinite(cov).all() and np.isfinite(mean).all() and (np.diag(cov) > 0.0).all()


def test_every_call_variant_gives_the_mirrors_bits_past_two_tile_rows():
    import torch
    shape = (2, 300, 401)
    n_keep, d, C = shape
    slab, ref = cases.frozen_slab(shape), cases.reference(shape)
    mean, cov = _run(shape)
    mean2, none_cov = mcmc_amd.draws_covariance(slab, want_cov=False)                     # one output alone
    none_mean, cov2 = mcmc_amd.draws_covariance(slab, want_mean=False)
    assert none_cov is None and none_mean is None
    cases.assert_is_the_mirror(mean2, cov2, ref, "single-output calls")
    cases.assert_same(mean2, mean, "want_cov=False")
    cases.assert_same(cov2, cov, "want_mean=False")
    dev = torch.from_numpy(np.array(slab)).cuda()                                         # the same slab in device memory
    mean3, cov3 = mcmc_amd.draws_covariance(dev, n_keep, d, C, mem=mcmc_amd.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    cases.assert_is_the_mirror(mean3, cov3, ref, "device slab")
    cases.assert_same(mean3, mean, "device slab, mean")
    cases.assert_same(cov3, cov, "device slab, cov")
    assert np.array_equal(dev.cpu().numpy(), slab)                                        # the slab is read only


def test_non_finite_samples_are_the_mirrors_past_two_tile_rows():
    """NaN in tile row 2, +inf in tile row 1: tiles (2, 0), (2, 1), (2, 2), (1, 0), (1, 1) carry them, tile (0, 0) and the rest of every tile do not"""
    shape = (2, 300, 401)
    slab = np.array(cases.frozen_slab(shape))
    i_nan, i_inf = 260, 131
    slab[1, i_nan, 5] = np.nan
    slab[0, i_inf, 400] = np.inf
    mean, cov = mcmc_amd.draws_covariance(slab)
    ref = cases.mirror(slab)
    cases.assert_is_the_mirror(mean, cov, ref, "the touched rows and columns included")
    bad = np.zeros(shape[1], dtype=bool)
    bad[[i_nan, i_inf]] = True
    touched = bad[:, None] | bad[None, :]
    assert np.array_equal(~np.isfinite(mean), bad) and np.array_equal(~np.isfinite(cov), touched)
    assert np.array_equal(~np.isfinite(ref["mean"]), bad) and np.array_equal(~np.isfinite(ref["cov"]), touched)
    clean_mean, clean_cov = _run(shape)
    assert np.array_equal(cases.bits(cov)[~touched], cases.bits(clean_cov)[~touched])     # everywhere else: the untouched run's bits
    assert np.array_equal(cases.bits(mean)[~bad], cases.bits(clean_mean)[~bad])
