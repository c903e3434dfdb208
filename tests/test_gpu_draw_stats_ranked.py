"""GPU: mi_mcmc_draw_stats_ranked -- rank-normalised split-R-hat, bulk-ESS and tail-ESS of a draws slab (Vehtari et al. 2021) against
mcmc_amd/rank_stats.py.

The function is the rank transform (held to numpy bit for bit by tests/test_gpu_rank_transform.py) and the 0 / 1 indicators, composed with the
EXISTING mi_mcmc_draw_stats on slabs of 2C half-chains.  The normal-score and indicator slabs are bitwise the reference's, so nothing new enters the
comparison and the tolerances are that reducer's own (tests/test_gpu_draw_stats.py): rtol 1e-10 for the three R-hat, 1e-8 for the two ESS; where
that file relaxes the ESS (phi >= 0.9 on series beyond 160 draws: the device sums 128 lags) the same relaxation applies to half-chains beyond 160."""

import numpy as np
import pytest

import mcmc_amd
from mcmc_amd import rank_stats as R

pytestmark = pytest.mark.gpu

RHATS = ("rhat", "rhat_bulk", "rhat_tail")
ESSES = ("ess_bulk", "ess_tail")


def _ar1(n, d, C_, phi, seed):
    rng = np.random.default_rng(seed)
    y = np.zeros((n, d, C_))
    y[0] = rng.standard_normal((d, C_))
    for t in range(1, n):
        y[t] = phi * y[t - 1] + np.sqrt(1 - phi ** 2) * rng.standard_normal((d, C_))
    return y + np.arange(d)[None, :, None]          # a different mean per dimension


def _agree(got, want, h, phi=0.0):
    for k in RHATS:
        assert np.allclose(got[k], want[k], rtol=1e-10, atol=0.0, equal_nan=True), (k, got[k], want[k])
    for k in ESSES:
        if phi >= 0.9 and h > 160:                  # the sum may still be positive at lag 127: the device reports the truncated sum
            assert np.all(got[k] >= want[k] * (1 - 1e-8)) and np.all(got[k] < h), (k, got[k], want[k])
        else:
            assert np.allclose(got[k], want[k], rtol=1e-8, atol=0.0, equal_nan=True), (k, got[k], want[k])
    assert set(got) == set(RHATS + ESSES)


AR1 = [(100, 5, 700, 0.6), (41, 3, 64, 0.0), (160, 2, 1000, 0.9), (9, 4, 130, 0.3), (1000, 3, 200, 0.7)]
_REF = {}


def _case(n, d, C_, phi):
    key = (n, d, C_, phi)
    if key not in _REF:
        x = _ar1(n, d, C_, phi, seed=n)
        x.setflags(write=False)
        _REF[key] = (x, R.draw_stats_ranked_ref(x))
    return _REF[key]


@pytest.mark.parametrize("n,d,C_,phi", AR1)
def test_ranked_stats_match_the_numpy_definitions(n, d, C_, phi):
    x, want = _case(n, d, C_, phi)
    got = mcmc_amd.draw_stats_ranked(x)
    _agree(got, want, n // 2, phi)
    assert np.all(np.abs(got["rhat"] - 1.0) < 0.2) and np.all(got["rhat"] >= np.maximum(got["rhat_bulk"], got["rhat_tail"]) * (1 - 1e-15))
    assert np.all(got["ess_bulk"] > 0) and np.all(got["ess_tail"] > 0)


@pytest.mark.parametrize("n,d,C_,phi", [(100, 5, 700, 0.6), (41, 5, 64, 0.0)])
def test_dimensions_processed_in_three_groups(n, d, C_, phi):
    """d = 5 under a budget of two dimensions: groups of 2, 2, 1, each through both sorts and the four passes of the reducer.  The reducer's chain-group
    count depends on the d it is called with, so bits may differ from the one-group call; values may not."""
    x, want = _case(n, d, C_, phi)
    lib = mcmc_amd.lib()
    try:
        b = lib.mi_mcmc_test_rank_dim_bytes(n, C_, 1, 1)
        lib.mi_mcmc_test_set_rank_ws_bytes(2 * b)
        assert lib.mi_mcmc_test_rank_dims_per_group(n, d, C_, 1, 1) == 2
        got = mcmc_amd.draw_stats_ranked(x)
    finally:
        lib.mi_mcmc_test_set_rank_ws_bytes(0)
    _agree(got, want, n // 2, phi)


def _normals():
    return np.random.default_rng(0).standard_normal((41, 2, 130))


def test_a_difference_in_scale_is_seen_by_the_folded_rhat_only():
    x = _normals()
    x[:, 1, :65] *= 3                                # half of the chains have 3 x the scale, same mean
    assert mcmc_amd.draw_stats(x)["rhat"][1] < 1.01
    got = mcmc_amd.draw_stats_ranked(x)
    assert got["rhat_tail"][1] > 1.05 and got["rhat"][1] == got["rhat_tail"][1]
    _agree(got, R.draw_stats_ranked_ref(x), 20)


def test_a_shifted_first_half_is_seen_by_the_split_rhat_only():
    w = _normals()
    w[:20, 0, :] += 1                                # every chain's first half is shifted by one sigma: not yet stationary
    assert mcmc_amd.draw_stats(w)["rhat"][0] < 1.01
    got = mcmc_amd.draw_stats_ranked(w)
    assert got["rhat_bulk"][0] > 1.05
    _agree(got, R.draw_stats_ranked_ref(w), 20)


def test_infinite_draws_leave_the_ranked_stats_finite():
    x = _normals()
    x[3, 0, 7] = np.inf
    x[30, 0, 100] = -np.inf
    classic = mcmc_amd.draw_stats(x)
    assert not (np.isfinite(classic["rhat"][0]) and np.isfinite(classic["mean"][0]))
    got = mcmc_amd.draw_stats_ranked(x)
    for k in RHATS + ESSES:
        assert np.isfinite(got[k]).all(), (k, got[k])
    _agree(got, R.draw_stats_ranked_ref(x), 20)


def test_a_nan_draw_is_reported_in_its_dimension_only():
    x = _normals()
    clean = mcmc_amd.draw_stats_ranked(x)
    x[3, 0, 7] = np.nan
    got = mcmc_amd.draw_stats_ranked(x)
    for k in RHATS + ESSES:
        assert np.isnan(got[k][0]) and got[k][1] == clean[k][1], (k, got[k], clean[k])
    _agree(got, R.draw_stats_ranked_ref(x), 20)


def test_ranked_stats_of_a_real_run():
    from mcmc_amd import synth
    d, C_, keep = 16, 4096, 60
    prec = synth.dense_gaussian_precision(d)
    st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=50, n_keep_draws=keep, n_leap_steps=8, step_size=0.15)
    draws, _ = mcmc_amd.hmc(mcmc_amd.TARGET_GAUSS_DENSE, synth.initial_states(C_, d, seed=3), st, prec=prec)
    got = mcmc_amd.draw_stats_ranked(draws)
    assert np.all(got["rhat"] < 1.05)
    _agree(got, R.draw_stats_ranked_ref(draws), keep // 2)
