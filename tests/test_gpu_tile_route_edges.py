"""GPU: the tile-target route (include/mi_mcmc_tile_target.hpp, mi_mcmc_engine/tile_samplers.hpp, nuts_tile.hpp; host driver mi_mcmc_run_tile_target) at its
edges -- a deterministic battery.  The six kernel families (hmc_tile_kernel<T, WPB>, hmc_tile_gen_kernel<T>, mala_tile_kernel<T>, mala_tile_kernel<T, true>,
nuts_tile_kernel<T, false>, nuts_tile_kernel<T, true>) run the twisted Gaussian of examples/user_tile_target.hip at NT 1, 2, 4 and 8 (tests/tile_targets.hip)
and every case is compared bit for bit -- draws, n_accept, and for nuts n_leap, step sizes and the depth trace -- with the oracle driven chain by chain by the
library's host callback (tests/tile_route.py; W = 4, hoist = 1), after asserting that mi_mcmc_last_kernel names the kernel the case means to hit.

  a  the non-finite regime of every kernel (this route cannot replay a user functor: it applies the reference's dense-product NaN rule itself)
  b  global chain ids (chain0 = 4099, chain0 > 2^32)            c  continuation through draw0 / step_size / nuts_adapt_state
  d  NT and d edges                                              e  chain counts around the wave, workgroup and grid edges
  f  degenerate settings                                         g  device-resident chains on a caller's stream
  h  nuts runs cut into pieces on a capped grid
The random counterpart is tests/fuzz_tile.py (tests/test_gpu_fuzz.py)."""
import ctypes as C

import numpy as np
import pytest

import mcmc_amd
import tile_route as tr
from mcmc_amd import synth

pytestmark = pytest.mark.gpu
SLOW = pytest.mark.gpu_slow


@pytest.fixture(scope="module")
def libs():
    if not tr.have_toolchain():
        pytest.skip("no hipcc / libmi_mcmc")
    return tr.Libs()


_oracle = {}


def oracle(libs, key, case, chains=None):
    """The oracle's result of a case, computed once per key and shared (never written to)."""
    if key not in _oracle:
        _oracle[key] = tr.run_oracle(libs, case, chains)
    return _oracle[key]


def against_oracle(libs, key, case, chains=None):
    o_draws, o = oracle(libs, key, case, chains)
    g_draws, g = tr.run_gpu(libs, case)
    assert mcmc_amd.last_kernel() == case.kernel_name()
    assert tr.mismatches(case.algo, g_draws, g, o_draws, o, chains) == []
    return g_draws, g, o_draws, o


def plain_init(C_, d, scale=0.5):
    return synth.initial_states(C_, d, seed=7) * scale


def general(d, what, free=()):
    """what: "bounds", "mass" or "both" -> (lb, ub, M)"""
    lb, ub = tr.mixed_bounds(d, seed=d, free=free) if what in ("bounds", "both") else (None, None)
    M = np.diag(np.linspace(0.5, 2.0, d)) if what in ("mass", "both") else None
    return lb, ub, M


STEP = dict(hmc=dict(eps=0.25, L=4), mala=dict(eps=0.4), nuts=dict(eps=1.0, adapt=5, depth=5, burn=4))


def make_case(algo, nt, d, init, what=None, free=(), **kw):
    lb, ub, M = general(d, what, free)
    if lb is not None:                                   # the bounded dimensions inside their boxes (a non-finite entry stays: it is the data)
        boxed = (np.isfinite(lb) | np.isfinite(ub))[None, :] & np.isfinite(init)
        init = np.where(boxed, np.clip(np.where(boxed, init, 0.0) * 0.6, -1.0, 1.5), init)
    step = dict(STEP[algo], eps=0.08) if (algo == "hmc" and what) else STEP[algo]      # (with bounds or a mass the larger step is never accepted)
    return tr.Case(algo, nt, d, init, lb=lb, ub=ub, M=M, **{**step, **kw})


# ---- a. the non-finite regime -----------------------------------------------------------------------------------------------------------------------------

def poisoned_init(d, C_=20):
    """20 chains, 4 of them started in the non-finite regime: x 1e200 (chain 3), +inf in the first dimension (5), NaN in a middle one (9), -inf in the last
    real one (14)."""
    init = plain_init(C_, d)
    init[3] *= 1e200; init[5, 0] = np.inf; init[9, d // 2] = np.nan; init[14, d - 1] = -np.inf
    return init


def overflowing_init(d, C_=20):
    """20 chains: two started non-finite (+inf, NaN) and four (2, 7, 11, 16) started FINITE with a finite log kernel at scale 1e70, where the twist's gradient
    (~ 1e209) times the step size leaves the finite range inside the first trajectory: these chains go non-finite mid-run (and reject)."""
    init = plain_init(C_, d)
    init[5, 0] = np.inf; init[9, d // 2] = np.nan
    for c in (2, 7, 11, 16): init[c] *= 1e70
    return init


def regime_conditions(o_draws, o):
    """Conditions on the ORACLE's output, so that a case cannot pass by being all-NaN or all-finite."""
    finite, accepted = tr.regime(o_draws, o)
    assert (~finite).sum() >= 2                                       # at least two chains with a non-finite kept row
    assert (finite & accepted).sum() * 2 >= o_draws.shape[2]          # at least half the chains finite throughout, accepting at least once


A_CASES = [  # (kernel family, NT, d, general)    d = 13 at NT 1 and 37 at NT 4: the last real dimension is not the last padded one (the 4 s + j < d guard)
    ("hmc", 1, 13, None), ("hmc", 4, 37, None), ("hmc", 2, 32, None),
    ("hmc", 1, 13, "bounds"), ("hmc", 4, 37, "mass"), ("hmc", 2, 29, "both"),
    ("mala", 1, 13, None), ("mala", 4, 37, None),
    ("mala", 1, 13, "mass"), ("mala", 2, 29, "mass"),
    ("nuts", 1, 13, None), ("nuts", 4, 37, None),
    ("nuts", 1, 13, "bounds"), ("nuts", 4, 37, "mass"), ("nuts", 2, 29, "both"),
]


@pytest.mark.parametrize("algo,nt,d,what", A_CASES)
def test_chains_started_non_finite_on_every_tile_kernel(libs, algo, nt, d, what):
    """x 1e200, +inf, NaN and -inf starts in the first, a middle and the last real dimension (all three unbounded where the run has bounds: the transform would
    map an infinite start in a bounded dimension to a finite one)."""
    case = make_case(algo, nt, d, poisoned_init(d), what, free=(0, d // 2, d - 1), burn=0, keep=10)     # (no burn-in: the first rows after a non-finite start are kept)
    g_draws, g, o_draws, o = against_oracle(libs, ("a", algo, nt, d, what), case)
    regime_conditions(o_draws, o)


@pytest.mark.parametrize("algo,nt,d,what", [("hmc", 1, 13, None), ("hmc", 2, 29, "both"), ("hmc", 4, 37, "mass"), ("mala", 1, 13, None), ("mala", 4, 37, "mass"),
                                            ("nuts", 1, 13, None), ("nuts", 2, 29, "both"), ("nuts", 1, 2, None), ("nuts", 1, 2, "mass"), ("nuts", 1, 3, None)])
def test_finite_chains_that_leave_the_finite_range_mid_run(libs, algo, nt, d, what):
    """Chains 2, 7, 11, 16 start finite with a finite log kernel and overflow inside their first trajectory (witness below: one momentum-free leapfrog position
    update from the start, through the host callback, is already outside the finite range of the log kernel)."""
    kw = dict(L=2) if algo == "hmc" else {}              # (two leapfrog steps: the second drift is the one that meets a non-finite momentum; a third would erase the difference)
    case = make_case(algo, nt, d, overflowing_init(d), what, free=(0, 1, d // 2), burn=0, keep=10, **kw)
    eps = case.eps
    host = tr.TwistedTile(case.P.ctypes.data, d, tr.B, tr.S2)
    dp = C.POINTER(C.c_double)
    if what is None:
        for c in (2, 7, 11, 16):
            v, gr = case.init[c].copy(), np.zeros(d)
            assert np.isfinite(libs.host_kernel(v.ctypes.data_as(dp), gr.ctypes.data_as(dp), C.byref(host))) and np.isfinite(gr).all()
            with np.errstate(over="ignore", invalid="ignore"):
                v1 = v + (eps * eps / 2.0) * gr
            assert not np.isfinite(libs.host_kernel(v1.ctypes.data_as(dp), None, C.byref(host)))
    g_draws, g, o_draws, o = against_oracle(libs, ("a-mid", algo, nt, d, what), case)
    regime_conditions(o_draws, o)


# ---- b. global chain ids ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ["hmc", "mala", "nuts"])
@pytest.mark.parametrize("chain0", [4099, 2**32 + 7])         # (the oracle's chain_id is a uint64: it holds the id above 2^32)
def test_global_chain_ids(libs, algo, chain0):
    case = make_case(algo, 1, 13, plain_init(20, 13), chain0=chain0)
    g_draws, g, o_draws, o = against_oracle(libs, ("b", algo, chain0), case)
    assert o["n_accept"].sum() > 0
    # ... and they are ids, not positions: the same run numbered from 0 draws other numbers
    z_draws, _ = tr.run_gpu(libs, case, chain0=0)
    assert not np.array_equal(z_draws, g_draws)


@pytest.mark.parametrize("algo", ["hmc", "mala", "nuts"])
def test_a_run_at_chain0_16_reproduces_chains_16_to_31_of_a_run_at_chain0_0(libs, algo):
    init = plain_init(32, 13)
    whole = make_case(algo, 1, 13, init)
    part = make_case(algo, 1, 13, init[16:], chain0=16)
    w_draws, w = tr.run_gpu(libs, whole)
    p_draws, p = tr.run_gpu(libs, part)
    tail = dict(n_accept=w["n_accept"][16:], n_leap=w["n_leap"][16:], eps=w["eps"][16:], depth=w["depth"][:, 16:])
    assert tr.mismatches(algo, p_draws, p, w_draws[:, :, 16:], tail) == []
    assert w["n_accept"][16:].sum() > 0


# ---- c. continuation --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ["hmc", "mala"])
@pytest.mark.parametrize("what", [None, "mass"])
def test_hmc_and_mala_runs_cut_in_two_through_draw0(libs, algo, what):
    """(bounded runs are left out: theta is checkpointed in the natural space, and transform(inv_transform(.)) is not the identity in floating point)"""
    case = make_case(algo, 1, 13, plain_init(21, 13), what, burn=2, keep=9, chain0=9)
    g_draws, g, o_draws, o = against_oracle(libs, ("c", algo, what), case)
    c_draws, c = tr.run_gpu_cut(libs, case, 2 + 4)
    assert tr.mismatches(algo, c_draws, c, o_draws, o) == [] and np.array_equal(c["theta"], g["theta"])
    assert 0 < o["n_accept"].sum()
    # ... and draw0 is part of the counter: the second half run at draw0 = 0 draws other numbers
    z_draws, _ = tr.run_gpu(libs, case, burn=0, keep=5, init=g_draws[3].T.copy(), draw0=0)
    assert not np.array_equal(z_draws, g_draws[4:])


@pytest.mark.parametrize("what", [None, "mass"])
@pytest.mark.parametrize("cut", [3, 9, 10, 14])
def test_nuts_can_be_cut_anywhere_with_the_dual_averaging_state(libs, what, cut):
    """The pattern and cut points of tests/test_gpu_resume.py: n_adapt_draws = 10 of 18 draws, all kept; cut inside the adaptation window (3, 9), at its last
    draw (10) and after it (14); the second call gets step_size and nuts_adapt_state: bit-identical to the uncut run and to the oracle."""
    case = make_case("nuts", 1, 13, plain_init(21, 13), what, burn=0, keep=18, adapt=10, depth=5, chain0=4)
    g_draws, g, o_draws, o = against_oracle(libs, ("c-nuts", what), case)
    c_draws, c = tr.run_gpu_cut(libs, case, cut)
    assert tr.mismatches("nuts", c_draws, c, o_draws, o) == [] and np.array_equal(c["theta"], g["theta"])
    if cut <= 10:                                        # (after the window the state is no longer read, hence not carried)
        assert np.array_equal(c["adapt_state"], g["adapt_state"])
    assert g["depth"].max() >= 2


def test_a_cut_inside_the_window_without_the_state_is_refused(libs):
    case = make_case("nuts", 1, 13, plain_init(4, 13), burn=0, keep=2, adapt=6)
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        tr.run_gpu(libs, case, draw0=3, eps_in=np.ones(4), no_adapt_state=True)
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(mcmc_amd.MiMcmcError) as e:       # ... and any continuation without the step sizes
        tr.run_gpu(libs, case, draw0=9, no_step_size=True)
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG


# ---- d. NT and d edges ------------------------------------------------------------------------------------------------------------------------------------

D_HMC = [(1, 2), (1, 3), (1, 16), (2, 17), (2, 32), (4, 33), (8, 65), (8, 127), (8, 128)]
D_ENDS = [(1, 2), (1, 16), (2, 17), (2, 32), (4, 33), (8, 65), (8, 128)]
D_GEN = [(1, 3), (2, 17), (4, 33), (8, 127)]


@pytest.mark.parametrize("algo,nt,d,what", [("hmc", nt, d, None) for nt, d in D_HMC] + [(a, nt, d, None) for a in ("mala", "nuts") for nt, d in D_ENDS]
                         + [(a, nt, d, "both") for a in ("hmc", "nuts") for nt, d in D_GEN])
def test_every_tile_count_at_its_dimension_edges(libs, algo, nt, d, what):
    """d one above a slice or tile boundary (17, 33, 65), at 2 and 3, and at 16 NT for every NT: table sizes, LDS carve and nt_pad workspace of each."""
    kw = {}
    if algo == "hmc": kw = dict(eps={33: 0.05, 127: 0.02}.get(d, 0.08) if what else 0.12 if d >= 65 else 0.25)     # (steps at which chains both accept and reject)
    if algo == "mala" and d >= 65: kw = dict(eps=0.2)
    case = make_case(algo, nt, d, plain_init(17, d), what, **kw)
    g_draws, g, o_draws, o = against_oracle(libs, ("d", algo, nt, d, what), case)
    assert 0 < o["n_accept"].sum()
    if algo == "nuts" and what is None: assert g["depth"].max() >= 2


# ---- e. chain-count edges ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ["hmc", "mala", "nuts"])
@pytest.mark.parametrize("C_", [1, 15, 16, 17, 63, 64, 65])
def test_chain_counts_around_the_tile_and_workgroup_edges(libs, algo, C_):
    case = make_case(algo, 1, 5, plain_init(C_, 5))
    g_draws, g, o_draws, o = against_oracle(libs, ("e", algo, C_), case)
    assert 0 < o["n_accept"].sum()


@pytest.mark.parametrize("C_", [127, 128, 129])
def test_chain_counts_around_the_edge_of_the_two_waves_per_simd_grid(libs, C_):
    """hmc_tile_kernel<T, 8> (NT 8, d = 65): 128 chains per workgroup.  The oracle on a subset: the first tile (chains 0, 15), the last full tile (its first and
    last chain) and the tail tile (the last chain); then, at d = 33, every chain against hmc_tile_kernel<T, 4> on the NT 4 target -- an independent grid
    shape (64 chains per workgroup) with the same arithmetic (fma chains over more exact zeros)."""
    full = (C_ // 16) * 16
    subset = sorted({0, 15, full - 16, full - 1, C_ - 1})
    case = make_case("hmc", 8, 65, plain_init(C_, 65), eps=0.12)
    against_oracle(libs, ("e8", C_), case, chains=subset)
    wide = make_case("hmc", 8, 33, plain_init(C_, 33))
    narrow = make_case("hmc", 4, 33, plain_init(C_, 33))
    w_draws, w = tr.run_gpu(libs, wide)
    assert mcmc_amd.last_kernel() == "hmc_tile_kernel<user target, 8>"
    n_draws, n = tr.run_gpu(libs, narrow)
    assert mcmc_amd.last_kernel() == "hmc_tile_kernel<user target, 4>"
    assert tr.mismatches("hmc", w_draws, w, n_draws, n) == [] and np.array_equal(w["theta"], n["theta"])
    assert 0 < n["n_accept"].sum() < 6 * C_


# ---- f. degenerate settings -------------------------------------------------------------------------------------------------------------------------------

F_CASES = {
    "hmc_no_leapfrog_steps": ("hmc", dict(L=0)),
    "hmc_gen_no_leapfrog_steps": ("hmc", dict(L=0, what="both")),
    "hmc_one_draw": ("hmc", dict(burn=0, keep=1)),
    "mala_one_draw": ("mala", dict(burn=0, keep=1)),
    "nuts_one_draw": ("nuts", dict(burn=0, keep=1)),
    "nuts_depth_0": ("nuts", dict(depth=0)),
    "nuts_depth_10": ("nuts", dict(depth=10, C_=4, burn=0, keep=3, adapt=0, eps=0.004)),
    "nuts_no_adaptation": ("nuts", dict(adapt=0, eps=0.1)),
    "nuts_window_longer_than_the_run": ("nuts", dict(adapt=50)),
}


@pytest.mark.parametrize("name", sorted(F_CASES))
def test_degenerate_settings(libs, name):
    algo, kw = F_CASES[name]
    kw = dict(kw)
    C_, what = kw.pop("C_", 20), kw.pop("what", None)
    case = make_case(algo, 1, 13, plain_init(C_, 13), what, **kw)
    g_draws, g, o_draws, o = against_oracle(libs, ("f", name), case)
    if name == "nuts_depth_10": assert g["depth"].max() == 10          # the deepest tree of this route's records
    if name == "nuts_depth_0": assert g["depth"].max() == 0
    if "no_leapfrog" in name: assert (g["n_leap"] == 0).all()


# ---- g. device-resident chains ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo,what", [("hmc", None), ("hmc", "both"), ("nuts", None), ("nuts", "mass")])
def test_device_resident_chains_on_a_caller_stream(libs, algo, what):
    """mem = MI_MEM_DEVICE on a non-default stream: theta, draws, n_accept, n_leapfrogs, step sizes, depth trace and adapt state equal the host-memory call's."""
    import torch
    case = make_case(algo, 1, 13, plain_init(20, 13), what)
    h_draws, h = tr.run_gpu(libs, case)
    stream = torch.cuda.Stream()
    d_draws, dv = tr.run_gpu(libs, case, mem=mcmc_amd.MEM_DEVICE, stream=stream.cuda_stream)
    assert mcmc_amd.last_kernel() == case.kernel_name()
    assert np.array_equal(d_draws, h_draws) and 0 < h["n_accept"].sum()
    for k in ("theta", "n_accept", "n_leap") + (("eps", "depth", "adapt_state") if algo == "nuts" else ()):
        assert np.array_equal(dv[k], h[k]), k


# ---- h. pieces --------------------------------------------------------------------------------------------------------------------------------------------

def test_bounded_nuts_runs_with_a_chain_started_non_finite_are_cut_into_pieces(libs):
    """More chains (150) than the chain slots of a grid capped at one workgroup (64), 9 draws: nuts_tile_setup_pieces on the NT 4 twisted target with bounds and a
    diagonal precond_mat, chain 70 started at +inf in an unbounded dimension.  Equal to the same call uncapped; the oracle on a subset: the first and last chain
    of the first 64, the first chain handed out afterwards, the non-finite chain, the last chain."""
    d, C_ = 37, 150
    init = plain_init(C_, d)
    init[70, 0] = np.inf
    case = make_case("nuts", 4, d, init, "both", free=(0, 1), burn=4, keep=5, adapt=6, depth=5)
    u_draws, u = tr.run_gpu(libs, case)
    mcmc_amd.test_set_grid_cap(1)
    try:
        g_draws, g = tr.run_gpu(libs, case)
    finally:
        mcmc_amd.test_set_grid_cap(0)
    assert mcmc_amd.last_kernel() == case.kernel_name()
    assert tr.mismatches("nuts", g_draws, g, u_draws, u) == []
    subset = [0, 63, 64, 70, 149]
    o_draws, o = oracle(libs, ("h",), case, subset)
    assert tr.mismatches("nuts", g_draws, g, o_draws, o, subset) == []
    assert not np.isfinite(o_draws[:, :, 70]).all() and np.isfinite(o_draws[:, :, [0, 63, 64, 149]]).all() and o["depth"].max() >= 2
