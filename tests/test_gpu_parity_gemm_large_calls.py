"""GPU: what only LARGE calls of the matrix-product route (d > 512: mcmc_amd/csrc/gemm_samplers.hip, gemm_nuts.hpp) run, at the smallest shapes that reach it.
The other suites of the route stop at 300 chains = 3 chain tiles of 128, so they never see
  (a) the second round of the step kernel's workgroup map (xcd = id & 7, nt = xcd + 8 (q / MT)): more than 8 chain tiles, i.e. C > 1024;
  (b) the second and later passes of the grid-stride kernels (packs, load, store, row terms, nuts init), which need dK x Cp > 16.7 M elements -- here under
      test_set_grid_cap, which caps exactly those grids;
  (c) draws and ticks enqueued directly instead of replayed from a captured graph (the rule is work x C < 3e10; every test is below it) -- here under
      test_set_gemm_graph(1);
  (d) the capacity condition of hmc / mala / rwmh (free device memory) -- here under test_set_gemm_ws_bytes with test_gemm_need_bytes.
d = 513 (dK = 528, dM = 640: 5 row tiles, 33 K-tiles), the logistic target with N = 40 rows; C = 1025 (9 tiles: the second round holds one tile with one live
chain), 1024 (a full first round) and 2100 (17 tiles: three rounds, ragged); 1 + 3 draws.  Bit for bit against the oracle on EVERY chain (ref: src/hmc.cpp:155-205,
src/mala.cpp:149-186, src/rwmh.cpp:123-151, src/nuts.cpp:30-332); each oracle case is computed once and shared.

Step sizes.  Every oracle run must accept AND reject -- at least 1 % of the kept draws rejected, at least half accepted (asserted) --: a case that accepts everything
does not test the accepted-state bookkeeping, and the usual 0.02 / 0.03 accept all 3075 draws at these shapes.  The values below were picked on the CPU oracle by
that condition; the counts are of the full case (kept draws accepted of 3 C)."""
import functools

import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import synth
from test_gpu_parity_gemm_bounds import bounds, diag_mass
from test_gpu_parity_gemm_dense_m import dense_mass

pytestmark = pytest.mark.gpu
ALGO = {"hmc": orc.ALGO_HMC, "mala": orc.ALGO_MALA, "rwmh": orc.ALGO_RWMH, "nuts": orc.ALGO_NUTS}
D, N_LOGIT, SEED, BURN, KEEP, CHAIN0 = 513, 40, 3, 1, 3, 11

# name: algo, target, C, L (hmc) / max_tree_depth (nuts), variant, step size        # oracle: accepted of 3 C kept draws
CASES = {
    "hmc-dense": ("hmc", "dense", 1025, 2, "plain", 0.12),                          # 2878 of 3075
    "hmc-dense-L1": ("hmc", "dense", 1025, 1, "plain", 0.2),                        # 2666
    "hmc-dense-L3": ("hmc", "dense", 1025, 3, "plain", 0.12),                       # 2756
    "mala-dense": ("mala", "dense", 1025, 0, "plain", 0.12),                        # 3001
    "rwmh-dense": ("rwmh", "dense", 1025, 0, "plain", 0.025),                       # 2141
    "rwmh-dense-1024": ("rwmh", "dense", 1024, 0, "plain", 0.025),                  # 2138 of 3072
    "hmc-dense-2100": ("hmc", "dense", 2100, 2, "plain", 0.12),                     # 5896 of 6300
    "hmc-logit": ("hmc", "logit", 1025, 2, "plain", 0.15),                          # 2751
    "mala-logit": ("mala", "logit", 1025, 0, "plain", 0.2),                         # 2785
    "rwmh-logit": ("rwmh", "logit", 1025, 0, "plain", 0.02),                        # 2764
    "hmc-dense-m": ("hmc", "dense", 1025, 2, "dense_m", 0.2),                       # 2623
    "mala-dense-m": ("mala", "dense", 1025, 0, "dense_m", 0.12),                    # 2722
    "hmc-box": ("hmc", "dense", 1025, 2, "box_diag", 0.02),                         # 2148
    "rwmh-box": ("rwmh", "dense", 1025, 0, "box", 0.02),                            # 2187
    "nuts-dense": ("nuts", "dense", 1025, 3, "plain", 0.1),                         # 2029
    "nuts-logit": ("nuts", "logit", 1025, 2, "plain", 0.1),                         # 2020
}
NUTS = dict(n_adapt=2, delta=0.55, gamma=0.1, t0=1.0)      # nuts: the adaptation window ends inside the 1 + 3 draws
DEPTH_CHAINS = (0, 1, 127, 128, 640, 895, 896, 901, 1023, 1024)      # nuts: chains whose depths per draw are compared (one oracle run each): tiles 0, 1, 5, 6, 7 and 8


def _poisoned_chains(C):
    """four chains started non-finite: in tile 0, in tile 7 (its first and its last column but one ... the last of the first round) and in the last tile -- with
    C = 1025 that is tile 8, whose only live chain it is"""
    return (3, 7 * 128 + 5, 8 * 128 - 1, C - 1)


def _poison(init, variant):
    """huge / +inf / NaN starts (tests/test_gpu_parity_gemm.py; with bounds on a bounded and on a free dimension, tests/test_gpu_parity_gemm_bounds.py)"""
    C, d = init.shape
    a, b, c, e = _poisoned_chains(C)
    i_inf, i_nan = 5, d - 1
    if variant.startswith("box"):
        lo, hi = bounds(d, "a")
        i_inf = int(np.flatnonzero(np.isfinite(lo) | np.isfinite(hi))[2])
        i_nan = int(np.flatnonzero(~(np.isfinite(lo) | np.isfinite(hi)))[-1])
    init[a] *= 1e200
    init[b, i_inf] = np.inf
    init[c, i_nan] = np.nan
    init[e] *= 1e160


@functools.lru_cache(maxsize=None)
def _problem(target, C, variant):
    """the recipes of the other suites of the route at d = 513: target keywords of mcmc_amd.sample, the oracle's TargetSpec, the initial states (read-only: shared)"""
    scale = 0.5 if target == "dense" else 0.1
    init = synth.initial_states(C, D, seed=D + 2) * scale
    if variant.startswith("box"):
        init = np.clip(init, -1.0, 1.5)                   # inside the bounds of every pattern
    init.flags.writeable = False
    if target == "dense":
        prec = synth.dense_gaussian_precision(D, seed=D % 89)
        return mcmc_amd.TARGET_GAUSS_DENSE, dict(prec=prec), orc.TargetSpec(orc.TARGET_DENSE, D, prec=prec, W=4), init
    X, y = synth.logistic_problem(D, N_LOGIT, seed=5)
    return mcmc_amd.TARGET_LOGISTIC, dict(X=X, y=y), orc.TargetSpec(orc.TARGET_LOGISTIC, D, X=X, y=y, W=4), init


def _extras(variant):
    """precond_mat and bounds of a variant: (M, lower, upper)"""
    if variant == "dense_m":
        return dense_mass(D, D + 1), None, None
    if variant.startswith("box"):
        lo, hi = bounds(D, "a")                           # about a quarter of the dimensions bounded, types 2 / 3 / 4 mixed
        return (diag_mass(D, D + 1) if variant == "box_diag" else None), lo, hi
    return None, None, None


def _settings(name, burn=BURN, keep=KEEP):
    algo, _, _, L, variant, eps = CASES[name]
    M, lo, hi = _extras(variant)
    kw = dict(rng_seed_value=SEED, n_burnin_draws=burn, n_keep_draws=keep, step_size=eps, precond_mat=M)
    if lo is not None:
        kw.update(vals_bound=1, lower_bounds=lo, upper_bounds=hi)
    if algo == "nuts":
        kw.update(n_adapt_draws=NUTS["n_adapt"], target_accept_rate=NUTS["delta"], gamma_val=NUTS["gamma"], t0_val=NUTS["t0"], max_tree_depth=L)
    else:
        kw.update(n_leap_steps=max(L, 1))
    return mcmc_amd.default_settings(**kw)


def _oracle_settings(name, chain_id=0):
    algo, _, _, L, variant, eps = CASES[name]
    M, lo, hi = _extras(variant)
    kw = dict(seed=SEED, n_burnin=BURN, n_keep=KEEP, step=eps, W=4, hoist=1, precond=M, lower=lo, upper=hi, chain_id=chain_id)
    if algo == "nuts":
        kw.update(max_depth=L, **NUTS)
    else:
        kw.update(n_leap=max(L, 1))
    return orc.make_settings(**kw)


def _freeze(o_draws, o):
    o_draws.flags.writeable = False
    for v in o.values():
        v.flags.writeable = False
    return o_draws, o


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """the oracle on every chain of a case: computed once, shared by the tests below, never written"""
    algo, target, C, _, variant, _ = CASES[name]
    _, _, spec, init = _problem(target, C, variant)
    return _freeze(*orc.run_many(ALGO[algo], spec, init, _oracle_settings(name), chain0=CHAIN0))


@functools.lru_cache(maxsize=None)
def _oracle_poisoned(name):
    """... and with the four poisoned starts: chains are independent and their random numbers counter-based on the chain index, so only those four run again"""
    algo, target, C, _, variant, _ = CASES[name]
    _, _, spec, init = _problem(target, C, variant)
    init = init.copy()
    _poison(init, variant)
    o_draws, o = _oracle(name)
    o_draws, o = o_draws.copy(), {k: v.copy() for k, v in o.items()}
    for c in _poisoned_chains(C):
        c_draws, co = orc.run_many(ALGO[algo], spec, init[c:c + 1], _oracle_settings(name), chain0=CHAIN0 + c)
        o_draws[:, :, c] = c_draws[:, :, 0]
        for k in o:
            o[k][c] = co[k][0]
    return _freeze(o_draws, o)


def _run(name, poisoned=False, **kw):
    algo, target, C, _, variant, _ = CASES[name]
    kind, tkw, _, init = _problem(target, C, variant)
    if poisoned:
        init = init.copy()
        _poison(init, variant)
    g_draws, g = mcmc_amd.sample(algo, kind, init, kw.pop("settings", None) or _settings(name), chain0=CHAIN0, **kw, **tkw)
    return g_draws, g, mcmc_amd.last_kernel()


def _on_route(name, kern, graphed=True):
    algo, target, _, _, variant, _ = CASES[name]
    assert kern.startswith("gemm_step_kernel<"), kern
    assert (", 1>" in kern) == (target == "logit"), kern
    assert ("(" + algo in kern) and ("dense precond_mat" in kern) == (variant == "dense_m") and ("bounds" in kern) == variant.startswith("box"), kern
    assert ("diagonal precond_mat" in kern) == (variant == "box_diag"), kern
    assert (", graph" in kern) == graphed, kern


def _mixed(name, o):
    """the oracle both accepts and rejects: at least 1 % of the kept draws rejected, at least half accepted"""
    C = CASES[name][2]
    n, acc = KEEP * C, int(o["n_accept"].sum())
    print(f"{name}: oracle accepts {acc} of {n}")
    assert 2 * acc >= n and 100 * (n - acc) >= n, (name, acc, n)


def _same(name, g_draws, g, o_draws, o, nan=False):
    """draws, the final state, accept counts on every chain; hmc: the leapfrog counts; nuts: the reference's leapfrog counts and the step sizes"""
    algo = CASES[name][0]
    assert np.array_equal(g["n_accept"], o["n_accept"])
    assert np.array_equal(g_draws, o_draws, equal_nan=nan)
    assert np.array_equal(g["theta"], o_draws[-1], equal_nan=nan)
    if algo in ("hmc", "nuts"):
        assert np.array_equal(g["n_leap"], o["n_leap"])
    if algo == "nuts":
        assert np.array_equal(g["eps"], o["eps"], equal_nan=nan)


@functools.lru_cache(maxsize=None)
def _oracle_depths(name, poisoned):
    algo, target, C, _, variant, _ = CASES[name]
    _, _, spec, init = _problem(target, C, variant)
    if poisoned:
        init = init.copy()
        _poison(init, variant)
    chains = sorted(set(DEPTH_CHAINS) | set(_poisoned_chains(C)))
    return {c: orc.run_chain(orc.ALGO_NUTS, spec, init[c], _oracle_settings(name, chain_id=CHAIN0 + c), traces=True)[1]["depth"] for c in chains}


def _same_depths(name, g, poisoned=False):
    for c, dep in _oracle_depths(name, poisoned).items():
        assert np.array_equal(g["depth"][:, c], dep), c


def _check(name, g_draws, g, poisoned=False):
    o_draws, o = _oracle_poisoned(name) if poisoned else _oracle(name)
    _same(name, g_draws, g, o_draws, o, nan=poisoned)
    if CASES[name][0] == "nuts":
        _same_depths(name, g, poisoned)


# ---- (a) more than eight chain tiles
@pytest.mark.parametrize("name", [n for n in CASES if n not in ("hmc-dense-L1", "hmc-dense-L3")])
def test_more_than_eight_chain_tiles_equal_the_oracle(name):
    """9 tiles (one live chain in the second round), a full first round (C = 1024), 17 ragged tiles in three rounds; every variant of the route.  A chain tile that
    is never updated, or updated by the wrong workgroup, differs from the oracle from its first draw on"""
    o_draws, o = _oracle(name)
    _mixed(name, o)
    assert np.all(np.isfinite(o_draws))
    g_draws, g, kern = _run(name)
    _on_route(name, kern)
    _check(name, g_draws, g)
    if CASES[name][0] == "nuts":
        assert (g["n_exec"] <= g["n_leap"]).all()            # (every doubling on a memoised trajectory; up to depth 3 no leaf is walked twice)


NON_FINITE = ["hmc-dense", "mala-logit", "rwmh-dense", "hmc-dense-m", "hmc-box", "nuts-dense"]


@pytest.mark.parametrize("name", NON_FINITE)
def test_non_finite_chains_across_the_tile_range(name):
    """four chains started huge / +inf / NaN, in tiles 0, 7 and 8: flagged by the accept step, skipped by gemm_store_kernel and replayed by the literal kernel behind
    the route (rwmh forms no product that can go non-finite: it carries them itself); their neighbours keep the oracle's bits and stay finite"""
    C = CASES[name][2]
    g_draws, g, kern = _run(name, poisoned=True)
    _on_route(name, kern)
    _check(name, g_draws, g, poisoned=True)
    healthy = np.setdiff1d(np.arange(C), _poisoned_chains(C))
    assert np.all(np.isfinite(g_draws[:, :, healthy]))
    o_draws, _ = _oracle_poisoned(name)
    assert not np.all(np.isfinite(o_draws[:, :, list(_poisoned_chains(C))]))


# ---- (b) the later passes of the grid-stride loops
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("name", ["hmc-dense", "hmc-logit", "hmc-box", "hmc-dense-m", "mala-dense-m", "nuts-dense", "nuts-logit"])
def test_grid_stride_passes_equal_the_oracle(name, cap):
    """under a cap of 1 and of 3 workgroups every lane of the packs (of the target's and the mass matrices), gemm_load_kernel (plain and with bounds), gemm_store_kernel,
    gemm_rowterm_kernel and nuts_init_kernel makes hundreds of passes of its loop (3 does not divide the element counts): same bits.  The poisoned starts keep the
    skip of flagged chains in gemm_store_kernel in the picture"""
    poisoned = name in NON_FINITE
    try:
        mcmc_amd.test_set_grid_cap(cap)
        g_draws, g, kern = _run(name, poisoned=poisoned)
    finally:
        mcmc_amd.test_set_grid_cap(0)
    _on_route(name, kern)
    _check(name, g_draws, g, poisoned=poisoned)


# ---- (c) draws and ticks that are not replayed from a graph
@pytest.mark.parametrize("name", ["hmc-dense-L1", "hmc-dense", "hmc-dense-L3", "hmc-logit", "mala-dense", "rwmh-dense", "hmc-dense-m", "mala-dense-m", "hmc-box", "rwmh-box",
                                  "nuts-dense", "nuts-logit"])
def test_ungraphed_draws_equal_the_oracle(name):
    """test_set_gemm_graph(1): enqueue_draw / enqueue_tick on the caller's stream, draw after draw, as a call of 65 536 chains does -- with gemm_advance_kernel between the
    draws and hmc's ping-pong of thw[cur] / thw[nxt] at both parities of L (1 and 3 end in thw[0], 2 in thw[1])"""
    if name in ("hmc-dense-L1", "hmc-dense-L3"):
        _mixed(name, _oracle(name)[1])
        g_draws, g, kern = _run(name)
        _on_route(name, kern, graphed=True)
        _check(name, g_draws, g)
    try:
        mcmc_amd.test_set_gemm_graph(1)
        g_draws, g, kern = _run(name)
    finally:
        mcmc_amd.test_set_gemm_graph(0)
    _on_route(name, kern, graphed=False)
    _check(name, g_draws, g)


def test_a_single_draw_is_not_graphed_and_equals_the_first_of_many():
    """n_total == 1 in mode 0: nothing to replay, the draw is enqueued directly"""
    name = "hmc-dense"
    w_draws, w, kern = _run(name, settings=_settings(name, burn=0, keep=3))
    _on_route(name, kern, graphed=True)
    s_draws, s, kern = _run(name, settings=_settings(name, burn=0, keep=1))
    _on_route(name, kern, graphed=False)
    assert 0 < s["n_accept"].sum() < CASES[name][2]
    assert np.array_equal(s_draws[0], w_draws[0]) and np.array_equal(s["theta"], w_draws[0])


@pytest.mark.parametrize("first_graphed", [True, False])
def test_a_run_cut_in_two_one_half_graphed_equals_the_whole(first_graphed):
    """1 + 3 draws as (1 + 1) and, through mi_chains.draw0 = 2, (0 + 2); one call replays a graph, the other enqueues its draws: the whole is the oracle's run"""
    name = "hmc-dense"
    o_draws, o = _oracle(name)
    kind, tkw, _, _ = _problem("dense", CASES[name][2], "plain")
    try:
        mcmc_amd.test_set_gemm_graph(0 if first_graphed else 1)
        a_draws, a, kern = _run(name, settings=_settings(name, burn=1, keep=1))
        _on_route(name, kern, graphed=first_graphed)
        mcmc_amd.test_set_gemm_graph(1 if first_graphed else 0)
        b_draws, b = mcmc_amd.sample("hmc", kind, np.ascontiguousarray(a["theta"].T), _settings(name, burn=0, keep=2), chain0=CHAIN0, draw0=2, **tkw)
        _on_route(name, mcmc_amd.last_kernel(), graphed=not first_graphed)
    finally:
        mcmc_amd.test_set_gemm_graph(0)
    assert np.array_equal(np.concatenate([a_draws, b_draws]), o_draws)
    assert np.array_equal(a["n_accept"] + b["n_accept"], o["n_accept"])
    assert np.array_equal(b["theta"], o_draws[-1])


# ---- (d) the capacity edge of hmc / mala / rwmh
def _capacity_case(algo, variant):
    d, C = 520, 33
    prec = synth.dense_gaussian_precision(d, seed=11)
    init = synth.initial_states(C, d, seed=4) * 0.5
    kw = dict(rng_seed_value=8, n_burnin_draws=1, n_keep_draws=3, n_leap_steps=2, step_size=0.12 if variant != mcmc_amd.GEMM_BOUNDED else 0.02)
    if variant == mcmc_amd.GEMM_DENSE_M:
        kw.update(precond_mat=dense_mass(d, d + 1))
    if variant == mcmc_amd.GEMM_BOUNDED:
        lo, hi = bounds(d, "a")
        init = np.clip(init, -1.0, 1.5)
        kw.update(vals_bound=1, lower_bounds=lo, upper_bounds=hi)
    return d, C, init, dict(prec=prec), mcmc_amd.default_settings(**kw)


@pytest.mark.parametrize("algo,variant", [("hmc", mcmc_amd.GEMM_PLAIN), ("mala", mcmc_amd.GEMM_DENSE_M), ("hmc", mcmc_amd.GEMM_BOUNDED)])
def test_capacity_edge_the_route_then_the_literal_kernel(algo, variant):
    """a budget of exactly what the call needs keeps it on the route; one byte less and it stays on the literal kernel, with the same bits.  (The hook is the only way
    here: nothing is allocated towards a real out-of-memory condition)"""
    d, C, init, tkw, st = _capacity_case(algo, variant)
    need = mcmc_amd.test_gemm_need_bytes(d, 0, C, variant, replay=True)
    try:
        mcmc_amd.test_set_gemm_ws_bytes(need)
        r_draws, r = mcmc_amd.sample(algo, mcmc_amd.TARGET_GAUSS_DENSE, init, st, **tkw)
        kern = mcmc_amd.last_kernel()
        assert kern.startswith("gemm_step_kernel<") and "(" + algo in kern, kern
        mcmc_amd.test_set_gemm_ws_bytes(need - 1)
        l_draws, l = mcmc_amd.sample(algo, mcmc_amd.TARGET_GAUSS_DENSE, init, st, **tkw)
        assert mcmc_amd.last_kernel().startswith("literal_kernel<"), mcmc_amd.last_kernel()
    finally:
        mcmc_amd.test_set_gemm_ws_bytes(0)
    print(f"{algo} variant {variant}: need {need} bytes, accepts {int(r['n_accept'].sum())} of {3 * C}")
    assert 0 < r["n_accept"].sum()
    assert np.array_equal(r_draws, l_draws) and np.array_equal(r["theta"], l["theta"]) and np.array_equal(r["n_accept"], l["n_accept"])
    if algo == "hmc":
        assert np.array_equal(r["n_leap"], l["n_leap"])
    mcmc_amd.sample(algo, mcmc_amd.TARGET_GAUSS_DENSE, init, st, **tkw)      # the hook is off again: the real figure, the route
    assert mcmc_amd.last_kernel().startswith("gemm_step_kernel<"), mcmc_amd.last_kernel()
