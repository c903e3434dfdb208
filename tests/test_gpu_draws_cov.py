"""GPU: mi_mcmc_draws_covariance -- pooled mean and covariance of a draws slab [n_keep][d][C] on the matrix cores (draws_cov.hip).

Accuracy is checked against exact arithmetic (a two-pass covariance in np.longdouble) with DERIVED bounds, every element of every case:
  |cov_ij - ref_ij| <= (K + 64) 2^-52 sum_k |e_ik e_jk| / (K - 1)   twice the standard gamma_K bound of a length-K fma sum of once-rounded
                                                                   operands; the mean's own error enters at second order (sum_k e_jk = 0)
  |mean_i - mu_i|   <= (K + 2) 2^-53 mean_k |x_ik|
(numpy's own float64 np.cov / mean stay below 0.015 resp. 0.21 of them on these inputs; the covariance bound is <= 5e-12 relative on the
diagonal while one dropped or doubled sample moves an element by >= 1 / K ~ 5e-5.)  The bound's own sum of magnitudes is taken in float64.
The kernel walks no persistent grid -- one workgroup per (tile, chunk), both functions of the shape --, so there is no grid cap to vary."""
import functools

import numpy as np
import pytest

import mcmc_amd

pytestmark = pytest.mark.gpu

# d below one MFMA tile / the smallest K; d just past 128 (2 x 2 output tiles, a mirrored off-diagonal one) with a ragged C; the same with chunks
# that span slabs; many slabs of an odd width; more than one chunk per tile and more than one mean group; d = 1
SHAPES = [(1, 5, 2), (1, 130, 333), (3, 130, 333), (7, 17, 1001), (1, 200, 20000), (2, 1, 4097)]


def _slab(n_keep, d, C):
    rng = np.random.default_rng(1000 * n_keep + 10 * d + C)
    K = n_keep * C
    A = rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)
    x = A @ rng.standard_normal((d, K)) + rng.uniform(-10.0, 10.0, d)[:, None]          # [d][K], k = t C + c
    return np.ascontiguousarray(x.reshape(d, n_keep, C).transpose(1, 0, 2))


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
