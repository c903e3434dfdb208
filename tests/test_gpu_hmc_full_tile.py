"""GPU: the full-tile instantiation of the plain HMC kernel (hmc_dense.hpp, FULL_TILE: d == 16 NT, scalar-base addressing of the accepted
state and of the kept rows) and its ragged neighbours on the unchanged path -- through the C ABI against the oracle, bit for bit: draws,
final theta, n_accept and leapfrog counts."""
import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import synth
from test_gpu_parity_hmc import _oracle_many

pytestmark = pytest.mark.gpu

FULL = [16, 32, 64, 128]            # d == 16 NT for NT = 1, 2, 4, 8
RAGGED = [15, 17, 127, 113]         # their neighbours: the instantiations with the `dim < d` predicates
KEEP = 3
# d > 64 with few chains is otherwise routed to the one-wave / split-tile shapes (mi_mcmc.hip: run_hmc_tile); the hint is ignored below d = 65
TWO_WAVES = mcmc_amd.KERNEL_HMC_TWO_WAVES_PER_SIMD


def _nt(d):
    return 1 if d <= 16 else 2 if d <= 32 else 4 if d <= 64 else 8


def _settings(L, burn, eps, keep=KEEP, seed=77):
    return mcmc_amd.default_settings(rng_seed_value=seed, n_burnin_draws=burn, n_keep_draws=keep, n_leap_steps=L, step_size=eps)


def _check(d, init, st, hint=TWO_WAVES, chain0=1000, wpb=8, nan_ok=False):
    """one run against the oracle; returns (gpu draws, gpu info, oracle draws, oracle info)"""
    C = init.shape[0]
    prec = synth.dense_gaussian_precision(d, seed=5)
    g_draws, g = mcmc_amd.hmc(mcmc_amd.TARGET_GAUSS_DENSE, init, st, prec=prec, chain0=chain0, kernel_hint=hint)
    kernel = mcmc_amd.last_kernel()
    o_draws, o = _oracle_many(orc.TARGET_DENSE, d, init, st, prec=prec, chain0=chain0)
    n_tot = int(st.n_burnin_draws) + int(st.n_keep_draws)
    assert np.array_equal(g["n_accept"], o["n_accept"])
    assert np.array_equal(g_draws, o_draws, equal_nan=nan_ok)
    assert np.array_equal(g["theta"], o_draws[-1], equal_nan=nan_ok)                       # state out = last kept draw
    assert np.array_equal(g["n_leap"], o["n_leap"])
    assert np.array_equal(g["n_leap"], np.full(C, n_tot * int(st.n_leap_steps), dtype=np.uint64))
    if not nan_ok:                                          # (a replayed chain leaves the literal kernel's name behind)
        assert kernel.startswith("hmc_gauss_mfma_kernel<%d, %d, false, false, false>" % (_nt(d), wpb)), kernel
    return g_draws, g, o_draws, o


@pytest.mark.parametrize("C", [16, 17, 144])               # one tile; a ragged last tile; more than one workgroup
@pytest.mark.parametrize("d", FULL + RAGGED)
def test_full_and_ragged_tiles_bit_exact_vs_oracle(d, C):
    """step 0.5: some 80 % of the proposals are accepted, so waves hold accepting and rejecting chains in the same draw"""
    init = synth.initial_states(C, d, seed=11)
    for L in (0, 1, 3):
        for burn in (0, 2):
            _, _, _, o = _check(d, init, _settings(L, burn, 0.5))
            if C == 144 and L > 0:
                assert 0 < o["n_accept"].sum() < C * KEEP


@pytest.mark.parametrize("d", FULL)
def test_every_proposal_rejected(d):
    """a step far beyond the stability limit, energies still finite: every draw takes the reload path, the kept rows repeat the initial state"""
    C = 17
    init = synth.initial_states(C, d, seed=12)
    for L in (1, 3):
        g_draws, g, _, o = _check(d, init, _settings(L, 2, 50.0))
        assert o["n_accept"].sum() == 0
        assert np.array_equal(g_draws[-1], init.T)


@pytest.mark.parametrize("d", FULL)
def test_every_proposal_accepted(d):
    """a tiny step: every draw takes the save path"""
    C = 17
    init = synth.initial_states(C, d, seed=13)
    for L in (1, 3):
        _, _, _, o = _check(d, init, _settings(L, 2, 1.0e-7))
        assert np.array_equal(o["n_accept"], np.full(C, KEEP, dtype=np.uint64))


@pytest.mark.parametrize("d", FULL)
def test_a_chain_started_at_inf_among_finite_ones_is_replayed(d):
    C = 17
    init = synth.initial_states(C, d, seed=14)
    init[5, d - 1] = np.inf
    for L in (0, 3):
        g_draws, _, o_draws, _ = _check(d, init, _settings(L, 2, 0.05), nan_ok=True)
        assert not np.isfinite(o_draws[:, :, 5]).all() and np.isfinite(np.delete(g_draws, 5, axis=2)).all()


@pytest.mark.parametrize("d", FULL + [127])
def test_draws_discarded_same_final_state(d):
    C = 17
    prec = synth.dense_gaussian_precision(d, seed=5)
    init = synth.initial_states(C, d, seed=15)
    for L in (0, 3):
        st = _settings(L, 2, 0.05)
        none, g = mcmc_amd.hmc(mcmc_amd.TARGET_GAUSS_DENSE, init, st, prec=prec, chain0=1000, kernel_hint=TWO_WAVES, want_draws=False)
        assert none is None
        o_draws, o = _oracle_many(orc.TARGET_DENSE, d, init, st, prec=prec, chain0=1000)
        assert np.array_equal(g["theta"], o_draws[-1]) and np.array_equal(g["n_accept"], o["n_accept"]) and np.array_equal(g["n_leap"], o["n_leap"])


@pytest.mark.parametrize("d", FULL + [127])
def test_run_cut_in_two_through_draw0(d):
    """5 draws in one call (the oracle), and as 2 + 3 with the first call's final state and draw0 = 2"""
    C = 17
    prec = synth.dense_gaussian_precision(d, seed=5)
    init = synth.initial_states(C, d, seed=16)
    for L in (1, 3):
        o_draws, o = _oracle_many(orc.TARGET_DENSE, d, init, _settings(L, 0, 0.05, keep=5), prec=prec, chain0=1000)
        a, ga = mcmc_amd.hmc(mcmc_amd.TARGET_GAUSS_DENSE, init, _settings(L, 0, 0.05, keep=2), prec=prec, chain0=1000, kernel_hint=TWO_WAVES)
        b, gb = mcmc_amd.hmc(mcmc_amd.TARGET_GAUSS_DENSE, np.ascontiguousarray(ga["theta"].T), _settings(L, 0, 0.05, keep=3), prec=prec, chain0=1000,
                             draw0=2, kernel_hint=TWO_WAVES)
        assert np.array_equal(np.concatenate([a, b]), o_draws)
        assert np.array_equal(ga["n_accept"] + gb["n_accept"], o["n_accept"]) and np.array_equal(ga["n_leap"] + gb["n_leap"], o["n_leap"])
        assert np.array_equal(gb["theta"], o_draws[-1])


@pytest.mark.parametrize("C", [16, 17, 144])
@pytest.mark.parametrize("d", [128, 127])
def test_one_wave_per_simd_shape(d, C):
    """hmc_gauss_mfma_kernel<8, 4, ...>: the other waves-per-workgroup instantiation of the flag, and its ragged neighbour"""
    init = synth.initial_states(C, d, seed=17)
    for L in (0, 1, 3):
        for burn in (0, 2):
            _check(d, init, _settings(L, burn, 0.5), hint=mcmc_amd.KERNEL_HMC_ONE_WAVE_PER_SIMD, wpb=4)
