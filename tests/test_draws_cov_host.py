"""No GPU: mi_mcmc_draws_covariance and the dense mass adaptations reject bad arguments before any device call (MI_ERR_BAD_ARG even where no
device is visible -- a call that reached the device probe would answer MI_ERR_NO_DEVICE there)."""

import numpy as np
import pytest

import mcmc_amd


def _cov_rc(slab_ptr, n_keep, d, n_chains, mean, cov):
    return mcmc_amd.lib().mi_mcmc_draws_covariance(slab_ptr, mcmc_amd.MEM_HOST, n_keep, d,
                                                   n_chains, mean, cov, None)


@pytest.mark.parametrize("case", ["K_is_1", "K_is_0_keep", "K_is_0_chains", "d_is_0", "null_slab", "both_outputs_null"])
def test_draws_covariance_rejects_bad_arguments_without_a_gpu(case):
    x = np.zeros((2, 3, 4))
    mean, cov = np.zeros(3), np.zeros((3, 3))
    args = dict(slab_ptr=x.ctypes.data, n_keep=2, d=3, n_chains=4, mean=mean.ctypes.data, cov=cov.ctypes.data)
    args.update({"K_is_1": dict(n_keep=1, n_chains=1), "K_is_0_keep": dict(n_keep=0), "K_is_0_chains": dict(n_chains=0), "d_is_0": dict(d=0),
                 "null_slab": dict(slab_ptr=None), "both_outputs_null": dict(mean=None, cov=None)}[case])
    assert _cov_rc(**args) == mcmc_amd.MI_ERR_BAD_ARG
    assert b"draws_covariance" in mcmc_amd.lib().mi_mcmc_last_error()


def test_draws_covariance_front_end_raises():
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_covariance(np.zeros((1, 3, 1)))
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_covariance(np.zeros((3, 8)), want_mean=False, want_cov=False)
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG


@pytest.mark.parametrize("algo", ["hmc", "mala"])
@pytest.mark.parametrize("case", ["precond_mat_set", "mass_diag_set", "one_chain", "more_windows_than_burnin"])
def test_dense_mass_adaptation_rejects_bad_arguments_without_a_gpu(algo, case):
    d, n_chains = 4, 6
    fn = mcmc_amd.hmc_mass_adapted_dense if algo == "hmc" else mcmc_amd.mala_mass_adapted_dense
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_ISO, d)
    skw, ckw, n_windows = dict(n_burnin_draws=10, n_keep_draws=2), {}, 2
    if case == "precond_mat_set":
        skw["precond_mat"] = np.eye(d)
    elif case == "mass_diag_set":
        ckw["mass_diag"] = np.ones((d, n_chains))
    elif case == "one_chain":
        n_chains = 1
    else:
        n_windows = 11
    theta = np.zeros((d, n_chains))
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        fn(t, mcmc_amd.default_settings(**skw), mcmc_amd.make_chains(theta, n_chains, **ckw), n_windows=n_windows)
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    assert f"{algo} (dense mass adapted)" in str(e.value)


def test_new_entry_points_are_exported():
    for name in ("mi_mcmc_draws_covariance", "mi_mcmc_hmc_run_mass_adapted_dense", "mi_mcmc_mala_run_mass_adapted_dense"):
        assert name in mcmc_amd.EXPORTS and hasattr(mcmc_amd.lib(), name)
