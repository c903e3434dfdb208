"""GPU: mcmc::nuts beyond d = 512 on the matrix-product route (mcmc_amd/csrc/gemm_nuts.hpp; ref: src/nuts.cpp:30-332, include/mcmc/nuts.ipp:30-241): per-chain
memoised trees -- every chain at its own point of its own doubling of its own draw -- with the gradients of ALL chains as one fp64 matrix product per tick
(gemm_step_kernel<12, .>: the second half-kick with the step read per column).  Before, such a call ran on literal_kernel<2>.  Bit for bit against the oracle
(W = 4, one block: the engine's reduction order beyond d = 512), against the literal kernel of the same library on more chains, in the non-finite regime, across a
continuation, across shards, and at the capacity edge (ranges of chains; the literal kernel where not even one range fits)."""
import functools

import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import synth

pytestmark = pytest.mark.gpu
SEED, STEP = 7, 0.1
N_EXEC_CHAINS = 12          # chains per case whose executed leapfrogs and depths are checked against the memoised oracle (one oracle run per chain)


def _problem(target, d, N, C, seed_t=5):
    """tests/test_gpu_parity_gemm_bounds.py::_problem's recipe, unclipped"""
    if target == "dense":
        prec = synth.dense_gaussian_precision(d, seed=d % 89)
        init = synth.initial_states(C, d, seed=d + 2) * 0.5
        return mcmc_amd.TARGET_GAUSS_DENSE, dict(prec=prec), orc.TargetSpec(orc.TARGET_DENSE, d, prec=prec, W=4), init
    X, y = synth.logistic_problem(d, N, seed=seed_t)
    init = synth.initial_states(C, d, seed=d + 2) * 0.1
    return mcmc_amd.TARGET_LOGISTIC, dict(X=X, y=y), orc.TargetSpec(orc.TARGET_LOGISTIC, d, X=X, y=y, W=4), init


def _diag_mass(d):
    return np.diag(np.random.default_rng(d + 1).uniform(0.5, 2.0, d))


def _settings(depth, n_adapt, burn, keep, M=None, seed=SEED, step=STEP):
    return mcmc_amd.default_settings(rng_seed_value=seed, n_burnin_draws=burn, n_keep_draws=keep, n_adapt_draws=n_adapt, max_tree_depth=depth, step_size=step, precond_mat=M)


def _oracle_settings(depth, n_adapt, burn, keep, M=None, seed=SEED, step=STEP, chain_id=0):
    return orc.make_settings(seed=seed, n_burnin=burn, n_keep=keep, n_adapt=n_adapt, max_depth=depth, step=step, W=4, hoist=1, precond=M, chain_id=chain_id)


def _same(g_draws, g, o_draws, o, nan=False):
    """draws, accepts, the reference's leapfrog counts, step sizes and the final state.  Against the oracle's run_many, which returns no final state, theta is its last kept
    row.  Depths are NOT compared here (run_many returns none): _same_depth_as_the_library / _same_depth_as_the_oracle below."""
    assert np.array_equal(g["n_accept"], o["n_accept"])
    assert np.array_equal(g["n_leap"], o["n_leap"])
    assert np.array_equal(g_draws, o_draws, equal_nan=nan)
    assert np.array_equal(g["eps"], o["eps"], equal_nan=nan)
    assert np.array_equal(g["theta"], o["theta"] if "theta" in o else o_draws[-1], equal_nan=nan)


def _same_depth_as_the_library(g, l):
    assert np.array_equal(g["depth"], l["depth"])


def _same_depth_as_the_oracle(g, spec, init, chains, so, chain0=0):
    """tree depths per draw of the given chains, one oracle run per chain (orc.run_chain with traces); so(chain_id) makes the oracle's settings"""
    for c in chains:
        _, oc = orc.run_chain(orc.ALGO_NUTS, spec, init[c], so(chain0 + c), traces=True)
        assert np.array_equal(g["depth"][:, c], oc["depth"]), c


def _on_route(kern, target, diag=False):
    assert kern.startswith("gemm_step_kernel<") and "nuts" in kern and "memoised" in kern, kern
    assert (", 1>" in kern) == (target == "logit"), kern
    assert ("diagonal precond_mat" in kern) == diag, kern


CASES = [  # target, d, N, C, max_tree_depth, n_adapt, burn, keep, diagonal precond_mat, chain0: ragged d and N, ragged chain tiles (C = 45; C = 130: two tiles of 128)
    ("dense", 513, 0, 45, 5, 3, 2, 4, False, 0), ("dense", 640, 0, 130, 4, 4, 2, 3, True, 11), ("dense", 1100, 0, 45, 4, 4, 2, 4, False, 0),
    ("logit", 513, 40, 130, 4, 4, 2, 3, True, 11), ("logit", 600, 70, 45, 5, 3, 2, 4, False, 0), ("logit", 700, 300, 45, 4, 6, 2, 4, False, 5),
]


@functools.lru_cache(maxsize=None)
def _oracle_case(target, d, N, C, depth, n_adapt, burn, keep, diag, chain0):
    _, _, spec, init = _problem(target, d, N, C)
    M = _diag_mass(d) if diag else None
    return orc.run_many(orc.ALGO_NUTS, spec, init, _oracle_settings(depth, n_adapt, burn, keep, M), chain0=chain0)


@pytest.mark.parametrize("target,d,N,C,depth,n_adapt,burn,keep,diag,chain0", CASES)
def test_nuts_beyond_d512_equals_the_oracle(target, d, N, C, depth, n_adapt, burn, keep, diag, chain0):
    kind, tkw, spec, init = _problem(target, d, N, C)
    M = _diag_mass(d) if diag else None
    g_draws, g = mcmc_amd.sample("nuts", kind, init, _settings(depth, n_adapt, burn, keep, M), chain0=chain0, **tkw)
    _on_route(mcmc_amd.last_kernel(), target, diag)      # (on the commit before this: literal_kernel<2>)
    o_draws, o = _oracle_case(target, d, N, C, depth, n_adapt, burn, keep, diag, chain0)
    print(f"nuts {target} d={d} C={C} depth {depth}: oracle accepts {int(o['n_accept'].sum())} of {keep * C}, n_leap {int(o['n_leap'].min())}..{int(o['n_leap'].max())}")
    assert 0 < o["n_accept"].sum() < keep * C
    _same(g_draws, g, o_draws, o)
    # the leapfrogs it really made and the depths: what the memoised oracle makes -- one per distinct point of a doubling + the step-size search
    for c in range(min(C, N_EXEC_CHAINS)):
        _, oc = orc.run_chain(orc.ALGO_NUTS_MEMO, spec, init[c], _oracle_settings(depth, n_adapt, burn, keep, M, chain_id=chain0 + c), traces=True)
        assert int(g["n_exec"][c]) == oc["n_exec"], c
        assert np.array_equal(g["depth"][:, c], oc["depth"]), c
    assert (g["n_exec"] <= g["n_leap"]).all() and g["n_exec"].sum() < g["n_leap"].sum()      # (the literal kernel executes every leaf it counts)


@pytest.mark.parametrize("target,N", [("dense", 0), ("logit", 200)])
def test_nuts_equals_the_literal_kernel_on_more_chains(target, N):
    """three chain tiles (one ragged) x six row tiles: the same call on the literal kernel (one workgroup per chain; the oracle takes 12 s here)"""
    d, C = 700, 300
    kind, tkw, _, init = _problem(target, d, N, C)
    st = _settings(4, 4, 2, 4, seed=21)
    g_draws, g = mcmc_amd.sample("nuts", kind, init, st, chain0=1000, **tkw)
    _on_route(mcmc_amd.last_kernel(), target)
    l_draws, l = mcmc_amd.sample("nuts", kind, init, st, chain0=1000, kernel_hint=mcmc_amd.KERNEL_LITERAL, **tkw)
    assert mcmc_amd.last_kernel().startswith("literal_kernel<2>")
    print(f"nuts {target}: literal kernel accepts {int(l['n_accept'].sum())} of {4 * C}")
    assert 0 < l["n_accept"].sum() < 4 * C
    _same(g_draws, g, l_draws, l)
    _same_depth_as_the_library(g, l)
    assert g["n_exec"].sum() < l["n_exec"].sum() == l["n_leap"].sum()


def _poison(init):
    d = init.shape[1]
    init[3] *= 1e200
    init[7, 5] = np.inf
    init[12, d - 1] = np.nan
    init[20] *= 1e160


@pytest.mark.parametrize("target,N", [("dense", 0), ("logit", 64)])
def test_nuts_non_finite_regime_equals_the_oracle(target, N):
    """chains that reach the non-finite regime are flagged and replayed by literal_kernel<2> right behind the route; their neighbours in the product do not notice"""
    d, C = 640, 45
    kind, tkw, spec, init = _problem(target, d, N, C)
    _poison(init)
    g_draws, g = mcmc_amd.sample("nuts", kind, init, _settings(4, 4, 2, 3, seed=5), **tkw)
    _on_route(mcmc_amd.last_kernel(), target)
    o_draws, o = orc.run_many(orc.ALGO_NUTS, spec, init, _oracle_settings(4, 4, 2, 3, seed=5))
    _same(g_draws, g, o_draws, o, nan=True)
    _same_depth_as_the_oracle(g, spec, init, [3, 7, 12, 20, 0, 44], lambda cid: _oracle_settings(4, 4, 2, 3, seed=5, chain_id=cid))      # the poisoned chains and two others
    clean = np.setdiff1d(np.arange(C), [3, 7, 12, 20])
    assert np.all(np.isfinite(g_draws[:, :, clean])) and np.all(np.isfinite(g["eps"][clean]))
    print(f"nuts {target} poisoned: {int(np.isfinite(o_draws).all(axis=(0, 1)).sum())} of {C} chains finite, accepts {int(o['n_accept'].sum())} of {3 * C}")


@pytest.mark.parametrize("cut", [2, 4])
def test_nuts_continuation_equals_the_run_in_one_piece(cut):
    """0 + 6 draws with an adaptation window of 3: cut inside the window (after draw 2) and behind it (after draw 4), step sizes and the dual-averaging state handed over.
    (Behind the window the triple is dead weight for the draws and is not read back -- include/mi_mcmc.h: draw0, nuts_adapt_state; literal_kernel<2> does the same -- so
    what the second call exports of it is compared for the cut inside the window only.)"""
    d, C = 520, 33
    kind, tkw, _, init = _problem("dense", d, 0, C)
    w_draws, w = mcmc_amd.sample("nuts", kind, init, _settings(4, 3, 0, 6, seed=8), want_adapt_state=True, **tkw)
    _on_route(mcmc_amd.last_kernel(), "dense")
    assert 0 < w["n_accept"].sum() < 6 * C
    a_draws, a = mcmc_amd.sample("nuts", kind, init, _settings(4, 3, 0, cut, seed=8), want_adapt_state=True, **tkw)
    b_draws, b = mcmc_amd.sample("nuts", kind, a["theta"].T, _settings(4, 3, 0, 6 - cut, seed=8), draw0=cut, step_size_in=a["eps"], adapt_state_in=a["adapt_state"], **tkw)
    _on_route(mcmc_amd.last_kernel(), "dense")
    assert np.array_equal(np.concatenate([a_draws, b_draws]), w_draws)
    assert np.array_equal(a["n_accept"] + b["n_accept"], w["n_accept"]) and np.array_equal(a["n_leap"] + b["n_leap"], w["n_leap"])
    assert np.array_equal(b["eps"], w["eps"]) and np.array_equal(b["theta"], w["theta"])
    if cut <= 3:
        assert np.array_equal(b["adapt_state"], w["adapt_state"])
    assert np.array_equal(np.concatenate([a["depth"], b["depth"]]), w["depth"])


def test_nuts_shards_equal_the_whole():
    target, d, N, C, depth, n_adapt, burn, keep, diag, chain0 = CASES[0]
    kind, tkw, spec, init = _problem(target, d, N, C)
    o_draws, o = _oracle_case(*CASES[0])
    for lo, hi in [(0, 20), (20, 45)]:
        g_draws, g = mcmc_amd.sample("nuts", kind, init[lo:hi], _settings(depth, n_adapt, burn, keep), chain0=chain0 + lo, **tkw)
        _on_route(mcmc_amd.last_kernel(), target)
        _same(g_draws, g, o_draws[:, :, lo:hi], {k: v[lo:hi] for k, v in o.items()})
        _same_depth_as_the_oracle(g, spec, init[lo:hi], [0, hi - lo - 1], lambda cid: _oracle_settings(depth, n_adapt, burn, keep, chain_id=cid), chain0=chain0 + lo)


def test_nuts_capacity_edge_ranges_of_chains_then_the_literal_kernel():
    """the workspace is a routing condition, then chunking: under a budget of one 128-chain range 300 chains run as three ranges, same bits, same kernel; under a
    budget below one range the call stays on the literal kernel, same bits"""
    d, C, depth = 700, 300, 4
    kind, tkw, _, init = _problem("dense", d, 0, C)
    st = _settings(depth, 4, 2, 4, seed=21)
    chain_b, fixed_b = mcmc_amd.test_gemm_nuts_chain_bytes(d, 0, depth), mcmc_amd.test_gemm_nuts_fixed_bytes(d, 0)
    try:
        n0 = mcmc_amd.test_gemm_nuts_ranges()
        w_draws, w = mcmc_amd.sample("nuts", kind, init, st, chain0=1000, **tkw)
        name = mcmc_amd.last_kernel()
        _on_route(name, "dense")
        assert mcmc_amd.test_gemm_nuts_ranges() == n0 + 1
        mcmc_amd.test_set_gemm_nuts_ws_bytes(fixed_b + 128 * chain_b + chain_b // 2)
        r_draws, r = mcmc_amd.sample("nuts", kind, init, st, chain0=1000, **tkw)
        assert mcmc_amd.last_kernel() == name
        assert mcmc_amd.test_gemm_nuts_ranges() == n0 + 4
        _same(r_draws, r, w_draws, w)
        _same_depth_as_the_library(r, w)
        assert np.array_equal(r["n_exec"], w["n_exec"])
        mcmc_amd.test_set_gemm_nuts_ws_bytes(fixed_b + 127 * chain_b)
        l_draws, l = mcmc_amd.sample("nuts", kind, init, st, chain0=1000, **tkw)
        assert mcmc_amd.last_kernel().startswith("literal_kernel<2>")
        assert mcmc_amd.test_gemm_nuts_ranges() == n0 + 4
        _same(l_draws, l, w_draws, w)
        _same_depth_as_the_library(l, w)
    finally:
        mcmc_amd.test_set_gemm_nuts_ws_bytes(0)


def test_what_stays_on_the_literal_kernel():
    d, C = 520, 6
    kind, tkw, _, init = _problem("dense", d, 0, C)
    init = np.clip(init, -1.0, 1.5)
    dense_M = _diag_mass(d)
    dense_M[0, 1] = dense_M[1, 0] = 0.05
    calls = [
        (kind, dict(vals_bound=1, lower_bounds=np.full(d, -1.5), upper_bounds=np.full(d, 2.0)), {}, tkw),
        (kind, dict(precond_mat=dense_M), {}, tkw),
        (kind, dict(max_tree_depth=12), {}, tkw),
        (kind, {}, dict(kernel_hint=mcmc_amd.KERNEL_LITERAL), tkw),
        (mcmc_amd.TARGET_GAUSS_DIAG, {}, {}, dict(prec=np.linspace(0.5, 2.0, d))),
    ]
    for k, skw, ckw, t in calls:
        skw = dict(dict(max_tree_depth=3), **skw)
        st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=1, n_adapt_draws=1, step_size=STEP, **skw)
        mcmc_amd.sample("nuts", k, init, st, **ckw, **t)
        assert mcmc_amd.last_kernel().startswith("literal_kernel<2>"), (skw.keys(), ckw, mcmc_amd.last_kernel())


@pytest.mark.parametrize("depth,n_adapt", [(1, 4), (4, 0)])
def test_nuts_depth_one_and_no_adaptation_equal_the_oracle(depth, n_adapt):
    d, C = 513, 17
    kind, tkw, spec, init = _problem("dense", d, 0, C)
    g_draws, g = mcmc_amd.sample("nuts", kind, init, _settings(depth, n_adapt, 2, 4, seed=SEED_EDGE[depth]), **tkw)
    _on_route(mcmc_amd.last_kernel(), "dense")
    o_draws, o = orc.run_many(orc.ALGO_NUTS, spec, init, _oracle_settings(depth, n_adapt, 2, 4, seed=SEED_EDGE[depth]))
    print(f"nuts depth {depth} n_adapt {n_adapt}: oracle accepts {int(o['n_accept'].sum())} of {4 * C}")
    assert 0 < o["n_accept"].sum()
    _same(g_draws, g, o_draws, o)
    _same_depth_as_the_oracle(g, spec, init, [0, 8, 16], lambda cid: _oracle_settings(depth, n_adapt, 2, 4, seed=SEED_EDGE[depth], chain_id=cid))


SEED_EDGE = {1: 7, 4: 7}


def test_fuzz_slice():
    """six cases of the randomised sweep (tests/fuzz_gemm_nuts.py): every disagreement is counted, nothing is skipped"""
    import fuzz_gemm_nuts
    assert fuzz_gemm_nuts.sweep(6, seed=2024) == 0


@pytest.mark.gpu_slow
def test_fuzz_forty():
    import fuzz_gemm_nuts
    assert fuzz_gemm_nuts.sweep(40, seed=77) == 0
