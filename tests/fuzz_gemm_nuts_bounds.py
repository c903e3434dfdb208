"""Randomised sweep of mcmc::nuts with settings.vals_bound beyond d = 512 on the matrix-product route (mcmc_amd/csrc/gemm_nuts.hpp, gemm_step_kernel<13, .>) against
the literal kernel of the same library (MI_KERNEL_LITERAL: one workgroup per chain, the reference's recursion as written), and every third case against the CPU
oracle itself: ragged d and N, 1 .. 140 chains (fewer than 16: the call stays on the literal kernel, and the comparison is that kernel against itself and the oracle), max_tree_depth 1 .. 6, the three bound patterns of tests/test_gpu_parity_gemm_bounds.py (a quarter of the dimensions
bounded with the types mixed; every dimension two-sided; vals_bound with every bound infinite) on a random draw of the bounded dimensions, adaptation windows shorter
/ longer than the run, the identity or a diagonal precond_mat, chain0 offsets, occasional chains that start ON a bound or far out.  Every case is compared -- none is
skipped -- and every disagreement is counted.
Usage (GPU box): python tests/fuzz_gemm_nuts_bounds.py [n_cases] [seed]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import mcmc_amd
import orc
from mcmc_amd import synth
from test_gpu_parity_gemm_bounds import LB, UB, bounds


def sweep(n_cases=30, seed=1, verbose=True):
    rng = np.random.default_rng(seed)
    fails = 0
    for case in range(n_cases):
        with_oracle = case % 3 == 2
        kind = str(rng.choice(["logistic", "dense"]))
        d = int(rng.integers(513, 1101))
        if kind == "logistic":
            n_rows = int(rng.choice([1, 7, 16, 17, 100, 128, 129, 300]))
            X, y = synth.logistic_problem(d, n_rows, seed=int(rng.integers(1, 99)))
            tk, tkw, scale = mcmc_amd.TARGET_LOGISTIC, dict(X=X, y=y), 0.1
            spec = orc.TargetSpec(orc.TARGET_LOGISTIC, d, X=X, y=y, W=4)
        else:
            n_rows = 0
            prec = synth.dense_gaussian_precision(d, seed=int(rng.integers(1, 99)))
            tk, tkw, scale = mcmc_amd.TARGET_GAUSS_DENSE, dict(prec=prec), 0.5
            spec = orc.TargetSpec(orc.TARGET_DENSE, d, prec=prec, W=4)
        C = int(rng.choice([1, 5, 16, 33]) if with_oracle else rng.choice([1, 5, 16, 64, 127, 128, 129, 140]))
        depth = int(rng.integers(1, 7))
        burn, keep = int(rng.integers(0, 3)), int(rng.integers(1, 4))
        n_adapt = int(rng.choice([0, 1, burn + keep, burn + keep + 3]))
        eps_bar0 = float(rng.choice([0.05, 0.1, 1.0]))
        pattern = str(rng.choice(["a", "a", "b", "c"]))
        lo, hi = bounds(d, pattern, seed=int(rng.integers(1, 10**6)))
        init = np.clip(synth.initial_states(C, d, seed=int(rng.integers(1, 1000))) * scale, -1.0, 1.5)      # inside the bounds of every pattern
        wild = rng.random() < 0.25
        if wild:      # a chain or three that start on a bound, or far out where there is none
            for c in rng.choice(C, size=min(C, 3), replace=False):
                i = int(rng.integers(0, d))
                init[c, i] = LB if np.isfinite(lo[i]) else UB if np.isfinite(hi[i]) else float(rng.choice([1e200, -1e200, np.inf, np.nan]))
        sd = int(rng.integers(1, 10**6))
        chain0 = int(rng.integers(0, 5000))
        M = np.diag(rng.uniform(0.5, 2.0, d)) if rng.random() < 0.4 else None
        st = mcmc_amd.default_settings(rng_seed_value=sd, n_burnin_draws=burn, n_keep_draws=keep, n_adapt_draws=n_adapt, max_tree_depth=depth, step_size=eps_bar0, precond_mat=M,
                                       vals_bound=1, lower_bounds=lo, upper_bounds=hi)
        a_draws, a = mcmc_amd.sample("nuts", tk, init, st, chain0=chain0, **tkw)
        kernel = mcmc_amd.last_kernel()
        b_draws, b = mcmc_amd.sample("nuts", tk, init, st, chain0=chain0, kernel_hint=mcmc_amd.KERNEL_LITERAL, **tkw)
        bits = lambda v: np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
        same = lambda u, v: np.array_equal(bits(u), bits(v)) or np.array_equal(u, v, equal_nan=True)     # (NaN payloads may differ)
        on_route = kernel.startswith("gemm_step_kernel<13") and "nuts" in kernel and "bounds" in kernel and ("diagonal precond_mat" in kernel) == (M is not None)
        ok = ((on_route if C >= 16 else kernel.startswith("literal_kernel<2>"))      # (fewer than 16 bounded chains: the literal kernel, as before)
              and mcmc_amd.last_kernel().startswith("literal_kernel<2>")
              and same(a_draws, b_draws) and np.array_equal(a["n_accept"], b["n_accept"]) and same(a["theta"], b["theta"]) and np.array_equal(a["n_leap"], b["n_leap"])
              and same(a["eps"], b["eps"]) and np.array_equal(a["depth"], b["depth"]) and bool((a["n_exec"] <= a["n_leap"]).all()))
        if ok and with_oracle:
            so = orc.make_settings(seed=sd, n_burnin=burn, n_keep=keep, n_adapt=n_adapt, max_depth=depth, step=eps_bar0, W=4, hoist=1, precond=M, lower=lo, upper=hi)
            o_draws, o = orc.run_many(orc.ALGO_NUTS, spec, init, so, chain0=chain0)
            ok = same(a_draws, o_draws) and np.array_equal(a["n_accept"], o["n_accept"]) and np.array_equal(a["n_leap"], o["n_leap"]) and same(a["eps"], o["eps"])
        if verbose or not ok:
            print(("ok  " if ok else "FAIL"), dict(kind=kind, d=d, n_rows=n_rows, C=C, depth=depth, burn=burn, keep=keep, n_adapt=n_adapt, eps_bar0=eps_bar0, pattern=pattern,
                                                   diag=M is not None, chain0=chain0, wild=wild, oracle=with_oracle, seed=sd, kernel=kernel, acc=int(a["n_accept"].sum()),
                                                   n_leap=int(a["n_leap"].sum()), n_exec=int(a["n_exec"].sum())), flush=True)
        fails += 0 if ok else 1
    return fails


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    s = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    f = sweep(n, s)
    print("mismatching cases:", f)
    sys.exit(1 if f else 0)
