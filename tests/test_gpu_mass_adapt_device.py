"""GPU: the four mass-adapted entry points with mi_chains.mem = MI_MEM_DEVICE on a caller's non-blocking stream (tests/device_resident.py: guards, sentinels,
inputs produced on the stream) against the host-staged call of the same entry point, which tests/test_gpu_mass_adapt.py and tests/test_gpu_mass_adapt_dense.py
tie to the oracle; and the two estimator kernels of mcmc_amd/csrc/mass_adapt.hip bit for bit against tests/mass_estimators_ref.py, the numpy statement of their
order over the oracle's fma (tests/test_mass_estimators_ref_cpu.py holds that mirror to the exact variance)."""
import numpy as np
import pytest
import torch

import device_resident as dr
import mass_estimators_ref as ref
import mcmc_amd
import orc
from mcmc_amd import synth

pytestmark = pytest.mark.gpu
DOT = lambda a, b: orc.dot(np.ascontiguousarray(a), np.ascontiguousarray(b), 1)         # the oracle's fma chain
N_WINDOWS = 2


@pytest.fixture(scope="module")
def stream():
    s = torch.cuda.Stream()                               # non-blocking
    yield s
    mcmc_amd.release_workspace()                          # every stream's cached workspace, before the stream dies


def _pooled_diag(t, st, c, stream, extra=None):
    return mcmc_amd.hmc_mass_adapted(t, st, c, n_windows=N_WINDOWS, stream=stream)


def _dense_hmc(t, st, c, stream, extra=None):
    return mcmc_amd.hmc_mass_adapted_dense(t, st, c, n_windows=N_WINDOWS, stream=stream)


def _dense_mala(t, st, c, stream, extra=None):
    return mcmc_amd.mala_mass_adapted_dense(t, st, c, n_windows=N_WINDOWS, stream=stream)


def _per_chain(t, st, c, stream, extra=None):
    mcmc_amd.hmc_mass_adapted_per_chain(t, st, c, n_windows=N_WINDOWS, mass_out=None if extra is None else extra["mass_out"].ptr, stream=stream)


ENTRY = {  # entry point, hmc?, d, C, burn, keep, L, eps
    "hmc_pooled_diag_d24": (_pooled_diag, True, 24, 203, 8, 4, 3, 0.25),
    "hmc_pooled_dense_d24": (_dense_hmc, True, 24, 203, 8, 4, 3, 0.25),
    "mala_pooled_dense_d24": (_dense_mala, False, 24, 203, 8, 4, 1, 0.4),
    "hmc_per_chain_d24": (_per_chain, True, 24, 203, 9, 4, 3, 0.2),
    "hmc_pooled_dense_d130": (_dense_hmc, True, 130, 300, 4, 2, 3, 0.25),
}


def _host(entry, kind, prec, init, st, per_chain):
    """the host-staged call: numpy buffers, NULL stream"""
    C, d = init.shape
    theta = np.ascontiguousarray(init.T.copy())
    g = dict(theta=theta, draws=np.zeros((int(st.n_keep_draws), d, C)), n_accept=np.zeros(C, dtype=np.uint64), n_leap=np.zeros(C, dtype=np.uint64),
             n_exec=np.zeros(C, dtype=np.uint64))
    t = mcmc_amd.make_target(kind, d, prec=prec)
    c = mcmc_amd.make_chains(theta, C, draws=g["draws"], n_accept=g["n_accept"], n_leapfrogs=g["n_leap"], n_leapfrogs_executed=g["n_exec"])
    if per_chain:
        g["mass"] = np.zeros((d, C))
        mcmc_amd.hmc_mass_adapted_per_chain(t, st, c, n_windows=N_WINDOWS, mass_out=g["mass"])
    else:
        g["mass"] = entry(t, st, c, None)
    return g


@pytest.mark.parametrize("name", list(ENTRY))
def test_mass_adapted_entry_points_in_device_memory_on_a_side_stream(name, stream):
    entry, hmc, d, C, burn, keep, L, eps = ENTRY[name]
    per_chain = entry is _per_chain
    prec = synth.dense_gaussian_precision(d)
    init = synth.initial_states(C, d, seed=4)
    kind = mcmc_amd.TARGET_GAUSS_DENSE
    mk = lambda: mcmc_amd.default_settings(rng_seed_value=5, n_burnin_draws=burn, n_keep_draws=keep, n_leap_steps=L, step_size=eps)
    h = _host(entry, kind, prec, init, mk(), per_chain)
    dv = dr.run_case(stream, "hmc" if hmc else "mala", kind, init, mk(), prec=prec, call=entry,
                     extra_outputs=dict(mass_out=(dr._F64, (d, C))) if per_chain else None)
    print(f"{name}: {dv['kernel']}")
    for k in ("theta", "draws", "n_accept", "n_leap", "n_exec"):
        assert np.array_equal(dv[k], h[k]), k
    assert np.array_equal(dv["mass_out"] if per_chain else dv["returned"], h["mass"])
    assert np.isfinite(h["mass"]).all() and h["n_accept"].sum() > 0 and not np.array_equal(h["mass"], np.eye(d) if h["mass"].shape == (d, d) else np.ones(h["mass"].shape))
    total = (burn + keep) * L if hmc else 0                # the run's total, not the last part's (run_mass_adapted_parts / fill_n_leap, device branch)
    assert (dv["n_leap"] == total).all() and (dv["n_exec"] == total).all()
    assert dv["guards_ok"], "a store outside an output's extent"
    assert "step_size" in dv["untouched"] and dv["sentinel_left"] == {"step_size"}, dv["sentinel_left"]


# ---------------------------------------------------------------- pooled_variance_kernel, bit for bit
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("C", ref.C_POOLED)
def test_pooled_mass_is_the_mirror_of_the_initial_values(C, mem, stream):
    x = ref.pooled_input(C)                               # [5][C]: unit scale, offset 1e8, constant, one inf, spread 1e-170
    d = x.shape[0]
    init = np.ascontiguousarray(x.T)
    st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=1, n_leap_steps=1, step_size=0.1)
    if mem == "host":
        t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_ISO, d)
        mass = mcmc_amd.hmc_mass_adapted(t, st, mcmc_amd.make_chains(np.ascontiguousarray(x.copy()), C), n_windows=0)
    else:
        dv = dr.run_case(stream, "hmc", mcmc_amd.TARGET_GAUSS_ISO, init, st, outputs=(),
                         call=lambda t, s, c, stream_, extra: mcmc_amd.hmc_mass_adapted(t, s, c, n_windows=0, stream=stream_))
        mass = dv["returned"]
        assert dv["guards_ok"]
    want = ref.pooled_mass_ref(x, DOT)
    assert np.array_equal(mass, want), (mass, want)
    assert [want[ref.DIMS.index(k)] for k in ("constant", "one_inf", "spread_1e-170")] == [1.0, 1.0, 1.0]
    assert np.isfinite(want).all() and want[1] != 1.0 and want[0] != 1.0


# ---------------------------------------------------------------- chain_mass_estimate_kernel, bit for bit
@pytest.mark.parametrize("L", [3, 0], ids=["moving", "stuck"])
@pytest.mark.parametrize("n", ref.PART_LENGTHS)
def test_per_chain_mass_is_the_mirror_of_the_draws_of_part_0(n, L, stream):
    """One window: part 0 keeps n draws per chain, the reported masses are their estimate.  The kernel can only be fed through a run, so what it sees is
    what the sampler made of the start, not the start itself.  The chains START at the five kinds of dimension of mass_estimators_ref.pooled_input, chain 1 at
    1e200; "moving" (n_leap_steps = 3): the sampler moves every dimension at its own pace (the one started at 1e8 by about 1e6 per draw), so an offset of 1e8
    with spread 1 OVER THE DRAWS, a constant or a 1e-170 dimension do not reach the kernel here -- only tests/test_mass_estimators_ref_cpu.py holds the
    mirror on those.  "stuck" (n_leap_steps = 0 proposes the current state): EVERY chain is stuck, not one among moving ones -- no start makes a single chain of
    these targets reject every proposal --, so every dimension is constant over the draws: q = 0 up to the ulps an inexact mean leaves (the regularised mass),
    at 0.75, at 1e8 + x, at 1e-170 x alike; an inf stays an inf (mass 1)."""
    C = 37
    x = ref.pooled_input(C, seed=n)
    x[:, 1] = 1e200
    d = x.shape[0]
    init = np.ascontiguousarray(x.T)
    mk = lambda burn, keep: mcmc_amd.default_settings(rng_seed_value=4, n_burnin_draws=burn, n_keep_draws=keep, n_leap_steps=L, step_size=0.05)
    slab, _ = mcmc_amd.hmc(mcmc_amd.TARGET_GAUSS_ISO, init, mk(0, n))                  # part 0: an ordinary run with M = I
    want = ref.chain_mass_ref(slab, DOT)
    dv = dr.run_case(stream, "hmc", mcmc_amd.TARGET_GAUSS_ISO, init, mk(2 * n, 3), extra_outputs=dict(mass_out=(dr._F64, (d, C))),
                     call=lambda t, s, c, stream_, extra: mcmc_amd.hmc_mass_adapted_per_chain(t, s, c, n_windows=1, mass_out=extra["mass_out"].ptr, stream=stream_))
    assert dv["guards_ok"] and "mass_out" not in dv["sentinel_left"]
    assert np.array_equal(dv["mass_out"], want)
    assert np.isfinite(want).all() and (want > 0).all()
    if L == 0:
        stuck = (n + 5.0) / 5.0e-3
        assert np.all((want == 1.0) | ((want > 0.99 * stuck) & (want <= 1.0 / (5.0e-3 / (n + 5.0)))))
        assert want[ref.DIMS.index("constant"), 0] == 1.0 / (5.0e-3 / (n + 5.0))
    else:
        assert len(np.unique(want)) > C                   # the chains moved: masses of their own
