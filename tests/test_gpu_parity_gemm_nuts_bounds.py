"""GPU: mcmc::nuts with settings.vals_bound beyond d = 512 on the matrix-product route (mcmc_amd/csrc/gemm_nuts.hpp, gemm_step_kernel<13, .>; ref: src/nuts.cpp:93-135,
158-162 and the final inv_transform of draws_out).  The chains live in the transformed space -- prev_draw, the point records, the edges and the U-turn tests hold
theta --, the products are taken at x = inv_transform(theta), the half-kicks take J(theta) g (the second one in the product's epilogue) and the energies add
log_jacobian(theta).  Before, such a call ran on literal_kernel<2>.  Bit for bit against the oracle (W = 4, one block), against the literal kernel of the same
library on more chains, in the non-finite regime, across a continuation, across shards and at the capacity edge."""
import functools

import numpy as np
import pytest

import mcmc_amd
import orc
from test_gpu_parity_gemm_bounds import LB, UB, _problem, _strictly_inside, bounds, diag_mass

pytestmark = pytest.mark.gpu
SEED, STEP = 7, 0.1
N_EXEC_CHAINS = 12          # chains per case whose executed leapfrogs and depths are checked against the memoised oracle (one oracle run per chain)


def _settings(d, pattern, depth, n_adapt, burn, keep, M=None, seed=SEED, step=STEP):
    lo, hi = bounds(d, pattern)
    return mcmc_amd.default_settings(rng_seed_value=seed, n_burnin_draws=burn, n_keep_draws=keep, n_adapt_draws=n_adapt, max_tree_depth=depth, step_size=step, precond_mat=M,
                                     vals_bound=1, lower_bounds=lo, upper_bounds=hi)


def _oracle_settings(d, pattern, depth, n_adapt, burn, keep, M=None, seed=SEED, step=STEP, chain_id=0):
    lo, hi = bounds(d, pattern)
    return orc.make_settings(seed=seed, n_burnin=burn, n_keep=keep, n_adapt=n_adapt, max_depth=depth, step=step, W=4, hoist=1, precond=M, chain_id=chain_id, lower=lo, upper=hi)


def _same(g_draws, g, o_draws, o, nan=False):
    """draws, accepts, the reference's leapfrog counts, step sizes and the final state (against the oracle's run_many, which returns none: its last kept row)"""
    assert np.array_equal(g["n_accept"], o["n_accept"])
    assert np.array_equal(g["n_leap"], o["n_leap"])
    assert np.array_equal(g_draws, o_draws, equal_nan=nan)
    assert np.array_equal(g["eps"], o["eps"], equal_nan=nan)
    assert np.array_equal(g["theta"], o["theta"] if "theta" in o else o_draws[-1], equal_nan=nan)
    assert np.array_equal(g["theta"], g_draws[-1], equal_nan=nan)


def _on_route(kern, target, diag=False):
    assert kern.startswith("gemm_step_kernel<") and "nuts" in kern and "memoised" in kern and "bounds" in kern, kern
    assert (", 1>" in kern) == (target == "logit"), kern
    assert ("diagonal precond_mat" in kern) == diag, kern


CASES = [  # target, d, N, C, max_tree_depth, n_adapt, burn, keep, bound pattern, diagonal precond_mat, chain0 -- and the oracle's accepts, run on the CPU beforehand
    ("dense", 513, 0, 45, 5, 3, 2, 4, "a", False, 0),        # 16 / 180
    ("dense", 640, 0, 130, 4, 4, 2, 3, "b", True, 11),       # 197 / 390
    ("dense", 1100, 0, 45, 4, 4, 2, 4, "a", False, 0),       # 53 / 180
    ("dense", 1024, 0, 45, 4, 4, 2, 4, "c", False, 11),      # 114 / 180
    ("logit", 513, 40, 130, 4, 4, 2, 3, "a", True, 11),      # 174 / 390
    ("logit", 600, 70, 45, 5, 3, 2, 4, "a", False, 0),       # 23 / 180
    ("logit", 700, 300, 45, 4, 6, 2, 4, "b", False, 5),      # 135 / 180
]


@functools.lru_cache(maxsize=None)
def _oracle_case(target, d, N, C, depth, n_adapt, burn, keep, pattern, diag, chain0):
    _, _, spec, init = _problem(target, d, N, C)
    M = diag_mass(d, d + 1) if diag else None
    return orc.run_many(orc.ALGO_NUTS, spec, init, _oracle_settings(d, pattern, depth, n_adapt, burn, keep, M), chain0=chain0)


@pytest.mark.parametrize("target,d,N,C,depth,n_adapt,burn,keep,pattern,diag,chain0", CASES)
def test_bounded_nuts_beyond_d512_equals_the_oracle(target, d, N, C, depth, n_adapt, burn, keep, pattern, diag, chain0):
    kind, tkw, spec, init = _problem(target, d, N, C)
    lo, hi = bounds(d, pattern)
    M = diag_mass(d, d + 1) if diag else None
    g_draws, g = mcmc_amd.sample("nuts", kind, init, _settings(d, pattern, depth, n_adapt, burn, keep, M), chain0=chain0, **tkw)
    _on_route(mcmc_amd.last_kernel(), target, diag)      # (on the commit before this: literal_kernel<2>)
    o_draws, o = _oracle_case(target, d, N, C, depth, n_adapt, burn, keep, pattern, diag, chain0)
    print(f"bounded nuts {target} d={d} C={C} depth {depth} pattern {pattern}: oracle accepts {int(o['n_accept'].sum())} of {keep * C}, "
          f"n_leap {int(o['n_leap'].min())}..{int(o['n_leap'].max())}")
    assert np.all(np.isfinite(o_draws))
    assert 0 < o["n_accept"].sum() < keep * C
    _same(g_draws, g, o_draws, o)
    assert _strictly_inside(g_draws, lo, hi)
    # the leapfrogs it really made and the depths: what the memoised oracle makes -- one per distinct point of a doubling + the step-size search
    for c in range(min(C, N_EXEC_CHAINS)):
        _, oc = orc.run_chain(orc.ALGO_NUTS_MEMO, spec, init[c], _oracle_settings(d, pattern, depth, n_adapt, burn, keep, M, chain_id=chain0 + c), traces=True)
        assert int(g["n_exec"][c]) == oc["n_exec"], c
        assert np.array_equal(g["depth"][:, c], oc["depth"]), c
    assert (g["n_exec"] <= g["n_leap"]).all() and g["n_exec"].sum() < g["n_leap"].sum()      # (the literal kernel executes every leaf it counts)


def test_bounded_nuts_equals_the_literal_kernel_on_more_chains():
    """three chain tiles (one ragged) x six row tiles, the logistic target: the same call on the literal kernel (one workgroup per chain)"""
    d, N, C = 700, 200, 300
    kind, tkw, _, init = _problem("logit", d, N, C)
    lo, hi = bounds(d, "a")
    st = _settings(d, "a", 4, 4, 2, 4, seed=21)
    g_draws, g = mcmc_amd.sample("nuts", kind, init, st, chain0=1000, **tkw)
    _on_route(mcmc_amd.last_kernel(), "logit")
    l_draws, l = mcmc_amd.sample("nuts", kind, init, st, chain0=1000, kernel_hint=mcmc_amd.KERNEL_LITERAL, **tkw)
    assert mcmc_amd.last_kernel().startswith("literal_kernel<2>")
    print(f"bounded nuts logit: literal kernel accepts {int(l['n_accept'].sum())} of {4 * C}")
    assert 0 < l["n_accept"].sum() < 4 * C
    _same(g_draws, g, l_draws, l)
    assert np.array_equal(g["depth"], l["depth"])
    assert _strictly_inside(g_draws, lo, hi)
    assert g["n_exec"].sum() < l["n_exec"].sum() == l["n_leap"].sum()


POISONED = (3, 7, 12, 20)


def _poison(init, lo, hi):
    """one chain ON a lower bound (type 2), one PAST an upper bound (type 3), one ON the upper bound of a two-sided dimension (type 4), one huge in an unbounded one"""
    lower, upper = np.isfinite(lo), np.isfinite(hi)
    t2, t3, t4, free = np.flatnonzero(lower & ~upper), np.flatnonzero(~lower & upper), np.flatnonzero(lower & upper), np.flatnonzero(~lower & ~upper)
    init[3, t2[1]] = LB
    init[7, t3[1]] = UB + 0.5
    init[12, t4[1]] = UB
    init[20, free[2]] = 1e200


def test_bounded_nuts_non_finite_regime_equals_the_oracle_and_the_literal_kernel():
    """chains that start on or past a bound, or far out, leave the finite regime in the step-size search: they are flagged and replayed by literal_kernel<2>, with the
    bounds, right behind the route; their neighbours in the product keep the bits of the run without them (CASES[0])"""
    target, d, N, C, depth, n_adapt, burn, keep, pattern, diag, chain0 = CASES[0]
    kind, tkw, spec, init = _problem(target, d, N, C)
    lo, hi = bounds(d, pattern)
    _poison(init, lo, hi)
    st = _settings(d, pattern, depth, n_adapt, burn, keep)
    g_draws, g = mcmc_amd.sample("nuts", kind, init, st, **tkw)
    _on_route(mcmc_amd.last_kernel(), target)
    o_draws, o = orc.run_many(orc.ALGO_NUTS, spec, init, _oracle_settings(d, pattern, depth, n_adapt, burn, keep))
    print(f"bounded nuts poisoned: n_leap of the poisoned chains {[int(o['n_leap'][c]) for c in POISONED]}, "
          f"{int(np.isfinite(o_draws).all(axis=(0, 1)).sum())} of {C} chains finite, accepts {int(o['n_accept'].sum())} of {keep * C}")
    _same(g_draws, g, o_draws, o, nan=True)
    l_draws, l = mcmc_amd.sample("nuts", kind, init, st, kernel_hint=mcmc_amd.KERNEL_LITERAL, **tkw)
    assert mcmc_amd.last_kernel().startswith("literal_kernel<2>")
    _same(g_draws, g, l_draws, l, nan=True)
    assert np.array_equal(g["depth"], l["depth"])
    for c in POISONED + (0, 44):
        _, oc = orc.run_chain(orc.ALGO_NUTS, spec, init[c], _oracle_settings(d, pattern, depth, n_adapt, burn, keep, chain_id=c), traces=True)
        assert np.array_equal(g["depth"][:, c], oc["depth"]), c
    # the healthy chains: what they are in the run without the poisoned ones
    h_draws, h = _oracle_case(*CASES[0])
    clean = np.setdiff1d(np.arange(C), POISONED)
    assert np.array_equal(g_draws[:, :, clean], h_draws[:, :, clean]) and np.array_equal(g["eps"][clean], h["eps"][clean])
    assert np.array_equal(g["n_accept"][clean], h["n_accept"][clean]) and np.array_equal(g["n_leap"][clean], h["n_leap"][clean])
    assert np.all(np.isfinite(g_draws[:, :, clean]))


def _cut_run(pattern, cut, hint):
    """0 + 6 draws with an adaptation window of 3 in one call, and cut after `cut` draws through mi_chains.draw0: the final state (x), the step sizes and the
    dual-averaging state handed over"""
    d, C = 520, 33
    kind, tkw, _, init = _problem("dense", d, 0, C)
    S = lambda keep: _settings(d, pattern, 4, 3, 0, keep, seed=8)
    w_draws, w = mcmc_amd.sample("nuts", kind, init, S(6), want_adapt_state=True, kernel_hint=hint, **tkw)
    kern = mcmc_amd.last_kernel()
    a_draws, a = mcmc_amd.sample("nuts", kind, init, S(cut), want_adapt_state=True, kernel_hint=hint, **tkw)
    b_draws, b = mcmc_amd.sample("nuts", kind, np.ascontiguousarray(a["theta"].T), S(6 - cut), draw0=cut, step_size_in=a["eps"], adapt_state_in=a["adapt_state"],
                                 want_adapt_state=True, kernel_hint=hint, **tkw)
    return kern, mcmc_amd.last_kernel(), w_draws, w, a_draws, a, b_draws, b


@pytest.mark.parametrize("cut", [2, 4])
def test_bounded_nuts_continuation(cut):
    """a run cut inside the adaptation window (after draw 2) and behind it (after draw 4).  The continuation is handed x, the final state, and puts it through
    transform as a fresh run does (nuts.cpp:158-162); transform(inv_transform(theta)) is theta only up to rounding on a bounded dimension, so the concatenation can
    equal the run in one piece bit for bit only where the hand-over is exact: that is asserted with vals_bound set and every bound infinite (pattern c: the whole
    bounded route runs, both maps are the identity).  With finite bounds (pattern a) the cut run equals the literal kernel's cut run call by call -- the reference's
    semantics of a continued call -- and its first piece the head of the run in one piece.  (Behind the window the dual-averaging triple is not read back:
    tests/test_gpu_parity_gemm_nuts.py.)"""
    kern, kern_b, w_draws, w, a_draws, a, b_draws, b = _cut_run("c", cut, mcmc_amd.KERNEL_AUTO)
    _on_route(kern, "dense")
    _on_route(kern_b, "dense")
    assert 0 < w["n_accept"].sum() < 6 * 33
    assert np.array_equal(np.concatenate([a_draws, b_draws]), w_draws)
    assert np.array_equal(a["n_accept"] + b["n_accept"], w["n_accept"]) and np.array_equal(a["n_leap"] + b["n_leap"], w["n_leap"])
    assert np.array_equal(b["eps"], w["eps"]) and np.array_equal(b["theta"], w["theta"])
    if cut <= 3:
        assert np.array_equal(b["adapt_state"], w["adapt_state"])
    assert np.array_equal(np.concatenate([a["depth"], b["depth"]]), w["depth"])
    kern, kern_b, w_draws, w, a_draws, a, b_draws, b = _cut_run("a", cut, mcmc_amd.KERNEL_AUTO)
    _on_route(kern, "dense")
    _on_route(kern_b, "dense")
    lk, lk_b, lw_draws, lw, la_draws, la, lb_draws, lb = _cut_run("a", cut, mcmc_amd.KERNEL_LITERAL)
    assert lk.startswith("literal_kernel<2>") and lk_b.startswith("literal_kernel<2>")
    assert 0 < w["n_accept"].sum() < 6 * 33
    for (x_draws, x), (y_draws, y) in [((w_draws, w), (lw_draws, lw)), ((a_draws, a), (la_draws, la)), ((b_draws, b), (lb_draws, lb))]:
        _same(x_draws, x, y_draws, y)
        assert np.array_equal(x["depth"], y["depth"])
    if cut <= 3:
        assert np.array_equal(b["adapt_state"], lb["adapt_state"])
    assert np.array_equal(a_draws, w_draws[:cut])


def test_bounded_nuts_shards_equal_the_whole():
    target, d, N, C, depth, n_adapt, burn, keep, pattern, diag, chain0 = CASES[0]
    kind, tkw, spec, init = _problem(target, d, N, C)
    o_draws, o = _oracle_case(*CASES[0])
    for lo_c, hi_c in [(0, 20), (20, 45)]:
        g_draws, g = mcmc_amd.sample("nuts", kind, init[lo_c:hi_c], _settings(d, pattern, depth, n_adapt, burn, keep), chain0=chain0 + lo_c, **tkw)
        _on_route(mcmc_amd.last_kernel(), target)
        _same(g_draws, g, o_draws[:, :, lo_c:hi_c], {k: v[lo_c:hi_c] for k, v in o.items()})


def test_bounded_nuts_capacity_edge_ranges_of_chains_then_the_literal_kernel():
    """under a budget of one 128-chain range of BOUNDED chains 300 chains run as three ranges, same bits, same kernel; under a budget below one such range (which
    would still hold 128 unbounded chains) the call stays on the literal kernel, same bits"""
    d, C, depth = 700, 300, 4
    kind, tkw, _, init = _problem("dense", d, 0, C)
    st = _settings(d, "a", depth, 4, 2, 4, seed=21)
    chain_b, fixed_b = mcmc_amd.test_gemm_nuts_bounded_chain_bytes(d, 0, depth), mcmc_amd.test_gemm_nuts_fixed_bytes(d, 0)
    assert 128 * mcmc_amd.test_gemm_nuts_chain_bytes(d, 0, depth) <= 127 * chain_b + chain_b // 2 < 128 * chain_b
    try:
        n0 = mcmc_amd.test_gemm_nuts_ranges()
        w_draws, w = mcmc_amd.sample("nuts", kind, init, st, chain0=1000, **tkw)
        name = mcmc_amd.last_kernel()
        _on_route(name, "dense")
        assert 0 < w["n_accept"].sum() < 4 * C
        assert mcmc_amd.test_gemm_nuts_ranges() == n0 + 1
        mcmc_amd.test_set_gemm_nuts_ws_bytes(fixed_b + 128 * chain_b + chain_b // 2)
        r_draws, r = mcmc_amd.sample("nuts", kind, init, st, chain0=1000, **tkw)
        assert mcmc_amd.last_kernel() == name
        assert mcmc_amd.test_gemm_nuts_ranges() == n0 + 4
        _same(r_draws, r, w_draws, w)
        assert np.array_equal(r["depth"], w["depth"]) and np.array_equal(r["n_exec"], w["n_exec"])
        mcmc_amd.test_set_gemm_nuts_ws_bytes(fixed_b + 127 * chain_b + chain_b // 2)
        l_draws, l = mcmc_amd.sample("nuts", kind, init, st, chain0=1000, **tkw)
        assert mcmc_amd.last_kernel().startswith("literal_kernel<2>")
        assert mcmc_amd.test_gemm_nuts_ranges() == n0 + 4
        _same(l_draws, l, w_draws, w)
        assert np.array_equal(l["depth"], w["depth"])
    finally:
        mcmc_amd.test_set_gemm_nuts_ws_bytes(0)


MIN_CHAINS = 16         # a bounded call of fewer chains (less than one wave of the per-chain kernel) stays on the literal kernel, as before this route took bounds


def test_what_stays_on_the_literal_kernel_with_bounds():
    """bounded nuts with a dense precond_mat, a tree deeper than 10 or MI_KERNEL_LITERAL (chains.mass_diag is hmc's alone), and a call of fewer than 16 chains -- with
    the bits of the same chains on the route; without the bound arrays the call is a bad argument"""
    d, C = 520, MIN_CHAINS
    kind, tkw, _, init = _problem("dense", d, 0, C)
    lo, hi = bounds(d, "a")
    B = dict(vals_bound=1, lower_bounds=lo, upper_bounds=hi)
    dense_M = diag_mass(d, d + 1)
    dense_M[0, 1] = dense_M[1, 0] = 0.05
    for skw, ckw in [(dict(precond_mat=dense_M), {}), (dict(max_tree_depth=12), {}), ({}, dict(kernel_hint=mcmc_amd.KERNEL_LITERAL))]:
        skw = dict(dict(max_tree_depth=3), **skw)
        st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=1, n_adapt_draws=1, step_size=STEP, **B, **skw)
        mcmc_amd.sample("nuts", kind, init, st, **ckw, **tkw)
        assert mcmc_amd.last_kernel().startswith("literal_kernel<2>"), (skw.keys(), ckw, mcmc_amd.last_kernel())
    st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=2, n_adapt_draws=1, max_tree_depth=3, step_size=STEP, **B)
    g_draws, g = mcmc_amd.sample("nuts", kind, init, st, **tkw)
    _on_route(mcmc_amd.last_kernel(), "dense")
    l_draws, l = mcmc_amd.sample("nuts", kind, init[:MIN_CHAINS - 1], st, **tkw)
    assert mcmc_amd.last_kernel().startswith("literal_kernel<2>"), mcmc_amd.last_kernel()
    _same(l_draws, l, g_draws[:, :, :MIN_CHAINS - 1], {k: g[k][:MIN_CHAINS - 1] for k in ("n_accept", "n_leap", "eps")})
    st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=1, n_adapt_draws=1, max_tree_depth=3, step_size=STEP, vals_bound=1)
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.sample("nuts", kind, init, st, **tkw)
    assert "vals_bound needs lower_bounds and upper_bounds" in str(e.value), str(e.value)


def test_fuzz_slice():
    """six cases of the randomised sweep (tests/fuzz_gemm_nuts_bounds.py): every disagreement is counted, nothing is skipped"""
    import fuzz_gemm_nuts_bounds
    assert fuzz_gemm_nuts_bounds.sweep(6, seed=2025) == 0


@pytest.mark.gpu_slow
def test_fuzz_forty():
    import fuzz_gemm_nuts_bounds
    assert fuzz_gemm_nuts_bounds.sweep(40, seed=78) == 0
