"""GPU: the host files of the library share ONE state of mcmc_amd/csrc/host_linalg.hpp (tests/test_linalg_state_cpu.py holds the header to that on the
host).  The factorisations of mcmc::aees (CHOL_LOWER of cov_mat) and of the dense mass adaptations (mass_adapt.hip: INV and
CHOL_LOWER of every estimate, then the part's own in mi_mcmc.hip) run the device kernels mi_mcmc.hip installs, are counted by the counters its test
hooks read, obey the staging budget its hook sets, and meet in one memo.  What is read are the two counters around a call: factorisations computed
(not answered by the memo), and those of them that ran on the device.  A translation unit with a state of its own would compute on the host loops
(same bits), count nowhere, ignore the budget and miss the memo: the deltas below would change.

The expected deltas are those of the library as it was when these functions lived in mi_mcmc.hip (the parent commit's library, run by this file
through MI_MCMC_LIB)."""
import contextlib

import numpy as np
import pytest

import mcmc_amd
from mcmc_amd import synth

pytestmark = pytest.mark.gpu

D = 64                                                     # the smallest d the device kernels and the memo take


def _spd(seed):
    A = np.random.default_rng(seed).standard_normal((D, D))
    return A @ A.T / D + np.eye(D)


def _deltas(call):
    n0, v0 = mcmc_amd.test_linalg_computed(), mcmc_amd.test_linalg_computed_on_device()
    call()
    return mcmc_amd.test_linalg_computed() - n0, mcmc_amd.test_linalg_computed_on_device() - v0


@contextlib.contextmanager
def _stage_bytes(n):
    mcmc_amd.test_set_linalg_stage_bytes(n)
    try:
        yield
    finally:
        mcmc_amd.test_set_linalg_stage_bytes(0)


def _aees():
    init = synth.initial_states(2, D, seed=4) * 0.3
    s = mcmc_amd.default_settings(rng_seed_value=5, n_burnin_draws=1, n_keep_draws=2)
    a = mcmc_amd.aees_settings(n_initial_draws=2, temper_vec=[2.0], cov_mat=_spd(31))
    draws, info = mcmc_amd.aees(mcmc_amd.TARGET_GAUSS_ISO, init, s, a)
    assert np.isfinite(draws).all()
    return draws


def test_aees_factorises_cov_mat_on_the_device_once_and_then_from_the_memo():
    mcmc_amd.release_workspace()                           # (empties the calling thread's memo)
    out = []
    first = _deltas(lambda: out.append(_aees()))
    second = _deltas(lambda: out.append(_aees()))
    print(f"aees, cov_mat d = {D}: first call {first}, identical second call {second} (computed, on the device)")
    assert first == (1, 1) and second == (0, 0)            # (the parent commit's library: the same)
    assert np.array_equal(out[0], out[1])


def test_aees_obeys_the_staging_budget():
    """CHOL_LOWER at d = 64 stages 512 bytes: with 256 it runs the host loops (and a new budget empties the memo)"""
    out = []
    with _stage_bytes(256):
        under = _deltas(lambda: out.append(_aees()))
    again = _deltas(lambda: out.append(_aees()))
    print(f"aees, cov_mat d = {D}: under a 256-byte budget {under}, with the real one again {again} (computed, on the device)")
    assert under == (1, 0) and again == (1, 1)             # (the parent commit's library: the same)
    assert np.array_equal(out[0], out[1])


# (measured on the parent commit's library.  hmc: 2 estimates x (INV, CHOL_LOWER) + INV of the mass in each of the 2 parts, whose CHOL_LOWER the memo answers;
#  mala adds INV and CHOL_LOWER of eps^2 M per part.  A mass_adapt.hip with a state of its own would read (4, 4) / (8, 8): its estimates uncounted, no memo hit)
ADAPTED = {"mala": (mcmc_amd.mala_mass_adapted_dense, (10, 10)), "hmc": (mcmc_amd.hmc_mass_adapted_dense, (6, 6))}


@pytest.mark.parametrize("algo", list(ADAPTED))
def test_dense_mass_adaptation_factorises_on_the_device_and_its_parts_meet_the_memo(algo):
    """two estimates (INV of the shrunk covariance, CHOL_LOWER of the mass) and the two parts' own preparation of that mass"""
    fn, want = ADAPTED[algo]
    C = 80
    theta = np.ascontiguousarray((synth.initial_states(C, D, seed=6) * 0.3).T)
    draws = np.zeros((1, D, C))
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, D, prec=synth.dense_gaussian_precision(D))
    s = mcmc_amd.default_settings(rng_seed_value=9, n_burnin_draws=2, n_keep_draws=1, n_leap_steps=2, step_size=0.05)
    ch = mcmc_amd.make_chains(theta, C, draws=draws)
    mcmc_amd.release_workspace()
    M = []
    got = _deltas(lambda: M.append(fn(t, s, ch, n_windows=1)))
    print(f"{algo} (dense mass adapted), d = {D}, {C} chains, 1 window: {got} (computed, on the device)")
    assert got == want
    assert np.isfinite(M[0]).all() and np.isfinite(draws).all() and not np.array_equal(M[0], np.eye(D))
