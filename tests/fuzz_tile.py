"""Randomised sweep of the tile-target route (include/mi_mcmc_tile_target.hpp: hmc_tile_kernel, hmc_tile_gen_kernel, mala_tile_kernel<T>, <T, true>,
nuts_tile_kernel<T, false>, <T, true>) against the oracle driven by the target library's host callback: the twisted Gaussian at NT 1 / 2 / 4 / 8, ragged d and
chain tiles, bounds of the four types and / or a diagonal precond_mat, step sizes from tiny to absurd, 0 .. 4 leapfrog steps, adaptation windows and depth caps
0 .. 6, chain0 / draw0 offsets, chains that start in the non-finite regime, runs cut in two.  Bit-exact or report.
Usage (GPU box): python tests/fuzz_tile.py [n_cases] [seed]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import tile_route as tr
from mcmc_amd import synth

FAMILIES = ("hmc_tile", "hmc_tile_gen", "mala_tile", "mala_tile_gen", "nuts_tile", "nuts_tile_gen")
DIMS = {1: [2, 3, 5, 13, 16], 2: [17, 20, 29, 32, 7], 4: [33, 37, 50, 64, 12], 8: [65, 100, 127, 128, 40]}


def draw_case(rng, index):
    """Random case number `index`: (tile_route.Case, draw0, cut or None, description).  The kernel family goes round robin (a slice of 6 n cases has n of each);
    everything else is drawn, the same random numbers whatever runs afterwards."""
    algo, general = ("hmc", "mala", "nuts")[index % 3], (index // 3) % 2 == 1
    nt = int(rng.choice([1, 2, 4, 8], p=[0.4, 0.3, 0.2, 0.1]))
    d = int(rng.choice(DIMS[nt]))
    C = int(rng.choice([1, 3, 15, 16, 17, 33, 64, 65]))
    if nt == 8: C = min(C, 33)                              # (the oracle is O(d^2) per gradient and chain)
    rseed = int(rng.integers(1, 10**6))
    chain0 = int(rng.choice([0, int(rng.integers(1, 5000)), 4099, 2**32 + 5]))
    burn, keep, L = int(rng.integers(0, 4)), int(rng.integers(1, 7)), int(rng.integers(0, 5))
    adapt, depth = int(rng.integers(0, 7)), int(rng.integers(0, 7))
    eps = float(rng.choice([0.005, 0.05, 0.2, 0.4, 0.7, 1.5, 30.0, 1e160], p=[0.08, 0.12, 0.2, 0.2, 0.15, 0.1, 0.08, 0.07]))
    init = synth.initial_states(C, d, seed=rseed % 1013) * float(rng.choice([0.1, 0.5, 1.0]))
    what = int(rng.integers(0, 3))                           # general: bounds only, a diagonal precond_mat only, both (mala with bounds: refused on this route)
    bounded = general and algo != "mala" and what != 1
    precond = general and (algo == "mala" or what != 0)
    lb = ub = M = None
    free = sorted(set(int(i) for i in rng.integers(0, d, 2)))  # two dimensions that stay unbounded: a non-finite start survives the transform there
    if bounded:
        lb, ub = tr.mixed_bounds(d, rseed % 97, free=free)
        if rng.random() < 0.5:                               # sparse bounds: most 4-dim slices have no bounded dimension (the kernels skip those)
            keep_b = rng.random(d) < 0.15
            lb, ub = np.where(keep_b, lb, -np.inf), np.where(keep_b, ub, np.inf)
        init = np.clip(init, -1.0, 1.5)                      # inside every box
    if precond:
        M = np.diag(rng.uniform(0.3, 3.0, d))
    poisoned = rng.random() < 0.25
    pc, pd_, pv = int(rng.integers(0, C)), (free[int(rng.integers(0, len(free)))] if bounded else int(rng.choice([0, 1, d // 2, d - 1]))), float(rng.choice([np.inf, -np.inf, np.nan, 1e200]))
    if poisoned:
        if pv == 1e200: init[pc] *= 1e200
        else: init[pc, pd_] = pv
    want_cut = rng.random() < 0.3
    draw0 = int(rng.choice([0, 0, 1, 3]))
    if algo == "nuts" or bounded: draw0 = 0                  # (the state at draw0 comes from the oracle: theta alone, in the natural space)
    cut = None
    if want_cut and keep >= 2 and not bounded and draw0 == 0:  # (theta is checkpointed in the natural space: bounded runs are not cut)
        cut = burn + int(rng.integers(1, keep))
    case = tr.Case(algo, nt, d, init, seed=rseed, burn=burn, keep=keep, L=L, eps=eps, adapt=adapt, depth=depth, lb=lb, ub=ub, M=M, chain0=chain0, pseed=rseed % 89 + 1)
    desc = (f"{algo} NT={nt} d={d} C={C} eps={eps} L={L} burn={burn} keep={keep} adapt={adapt} depth={depth} bounds={bounded} M={precond} chain0={chain0} draw0={draw0} "
            f"cut={cut} poisoned={(pc, pd_, pv) if poisoned else None} seed={rseed}")
    return case, draw0, cut, desc


def family(case):
    return f"{case.algo}_tile{'_gen' if case.gen else ''}"


def sweep(n_cases=24, seed=1, verbose=True, oracle_only=False):
    """Returns (mismatching cases, tally).  tally: cases per kernel family, cases with a non-finite kept draw, cases finite throughout with an accept and a reject.
    oracle_only: the generator and the oracle alone (no GPU): the mix a seed gives."""
    rng = np.random.default_rng(seed)
    say = print if verbose else (lambda *a, **k: None)
    libs = tr.Libs()
    fails = 0
    tally = dict(families={f: 0 for f in FAMILIES}, nonfinite=0, finite_mixed=0, cut=0, offset=0, n=n_cases)
    for index in range(n_cases):
        case, draw0, cut, desc = draw_case(rng, index)
        start = case.init
        whole_burn = case.burn + draw0
        if draw0:                                            # the state after draw0 draws, from the oracle: the device run starts there with mi_chains.draw0
            start = np.ascontiguousarray(tr.run_oracle(libs, case, burn=draw0 - 1, keep=1)[0][0].T)
        o_draws, o = tr.run_oracle(libs, case, burn=whole_burn)
        tally["families"][family(case)] += 1
        n_acc = int(o["n_accept"].sum())
        if not np.isfinite(o_draws).all(): tally["nonfinite"] += 1
        elif 0 < n_acc < case.keep * case.C: tally["finite_mixed"] += 1
        tally["cut"] += cut is not None; tally["offset"] += draw0 > 0 or case.chain0 > 0
        if oracle_only:
            say("oracle  ", desc, "accepts", n_acc, "of", case.keep * case.C, "finite" if np.isfinite(o_draws).all() else "NON-FINITE")
            continue
        import mcmc_amd
        g_draws, g = tr.run_gpu(libs, case, init=start, draw0=draw0)
        kernel = mcmc_amd.last_kernel()
        bad = tr.mismatches(case.algo, g_draws, g, o_draws, o)
        if kernel != case.kernel_name(): bad.append(f"kernel {kernel}")
        if cut is not None and not bad:
            c_draws, c = tr.run_gpu_cut(libs, case, cut)
            bad = ["cut " + b for b in tr.mismatches(case.algo, c_draws, c, o_draws, o)]
        if bad:
            fails += 1
            print("MISMATCH", desc, bad, flush=True)
        else:
            say("ok      ", desc, kernel, "accepts", n_acc, flush=True)
    return fails, tally


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    s = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    f, t = sweep(n, s, oracle_only="--oracle-only" in sys.argv)
    print("mismatching cases:", f, t)
    sys.exit(1 if f else 0)
