"""mcmc::nuts with settings.vals_bound beyond d = 512 on the matrix-product route (gemm_nuts.hpp, gemm_step_kernel<13, .>) against literal_kernel<2>, which served such a
call before (the same call with MI_KERNEL_LITERAL: the same bits), and against the unbounded call on the same route.  The protocol of tools/gemm_nuts_time.py: HIP
events around the C-ABI call on device buffers, one warm-up call discarded, the median of N timed calls with min and max; per shape the ticks run and the fraction
of the fp64 matrix peak on the EXECUTED leapfrogs.  d = 1024, max_tree_depth 6, 10 + 10 draws, bound patterns a (a quarter of the dimensions bounded, types mixed) and
b (every dimension two-sided) of tests/test_gpu_parity_gemm_bounds.py, the dense target and the logistic target with N = 4096.
(GPU box)  python tools/gemm_nuts_bounds_time.py --part dense|logit|ab [--calls 3] [--log profiles/gemm_nuts_bounds_time.log] [--literal-max 8192] [--counts 128,1024,8192,65536]
--part ab: the UNBOUNDED call of two libraries (MI_MCMC_LIB of the children: --lib-a, --lib-b), alternating child processes A B A B ..., one warm-up and one timed
call per child, the median of --calls children per library and shape."""
import argparse, os, subprocess, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

PEAK = 78.6      # TFLOP/s, fp64 matrix
D, DEPTH, N_ADAPT, BURN, KEEP, N_ROWS = 1024, 6, 10, 10, 10, 4096
LB, UB = -1.5, 2.0
LOG = None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def bounds(d, pattern):
    """tests/test_gpu_parity_gemm_bounds.py::bounds"""
    lo, hi = np.full(d, -np.inf), np.full(d, np.inf)
    if pattern == "a":
        t = np.random.default_rng(d).choice([1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 4], size=d)
        lo[(t == 2) | (t == 4)] = LB
        hi[(t == 3) | (t == 4)] = UB
    elif pattern == "b":
        lo[:], hi[:] = LB, UB
    return lo, hi


def run(Cn, hint, calls, pattern=None, n_rows=0, warm=True, quiet=False):
    """pattern None: the unbounded call"""
    import torch, mcmc_amd
    from mcmc_amd import synth
    d = D
    init = np.clip(synth.initial_states(Cn, d, seed=3) * (0.1 if n_rows else 0.5), -1.0, 1.5)
    theta0 = torch.from_numpy(np.ascontiguousarray(init.T)).cuda()
    bkw = {}
    if pattern is not None:
        lo, hi = bounds(d, pattern)
        bkw = dict(vals_bound=1, lower_bounds=lo, upper_bounds=hi)
    st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=BURN, n_keep_draws=KEEP, n_adapt_draws=N_ADAPT, max_tree_depth=DEPTH, step_size=0.1, **bkw)
    draws = torch.empty((KEEP, d, Cn), dtype=torch.float64, device="cuda")
    i64 = lambda: torch.zeros(Cn, dtype=torch.int64, device="cuda")
    n_accept, n_leap, n_exec = i64(), i64(), i64()
    eps = torch.zeros(Cn, dtype=torch.float64, device="cuda")
    if n_rows:
        X, y = synth.logistic_problem(d, n_rows, seed=5)
        tgt = mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, d, X=torch.from_numpy(X).cuda(), y=torch.from_numpy(y).cuda(), mem=mcmc_amd.MEM_DEVICE, kernel_hint=hint)
        flop_per_leap = 4.0 * n_rows * d
    else:
        tgt = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=torch.from_numpy(synth.dense_gaussian_precision(d)).cuda(), mem=mcmc_amd.MEM_DEVICE, kernel_hint=hint)
        flop_per_leap = 2.0 * d * d
    times = []
    for it in range(calls + (1 if warm else 0)):        # (the first call is the warm-up)
        theta = theta0.clone()
        ch = mcmc_amd.make_chains(theta, Cn, draws=draws, n_accept=n_accept, step_size=eps, n_leapfrogs=n_leap, n_leapfrogs_executed=n_exec, mem=mcmc_amd.MEM_DEVICE)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        mcmc_amd.run("nuts", tgt, st, ch)
        e1.record(); torch.cuda.synchronize()
        if it or not warm: times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    kern = mcmc_amd.last_kernel()
    ex, le = int(n_exec.sum()), int(n_leap.sum())
    tf = ex * flop_per_leap / (ms * 1e-3) / 1e12
    line = (f"nuts {'logistic N=%d' % n_rows if n_rows else 'dense'} d={d} C={Cn} {'bounds pattern ' + pattern if pattern else 'unbounded'} max_tree_depth={DEPTH} n_adapt={N_ADAPT} "
            f"draws={BURN}+{KEEP}: {ms:.1f} ms (median of {len(times)}{'' if warm else ', no warm-up'}, min {min(times):.1f} max {max(times):.1f}), kernel {kern}, "
            f"leapfrogs executed {ex} of the reference's {le}, {tf:.2f} TFLOP/s on executed flops = {tf / PEAK:.4f} of the fp64 matrix peak, accepts {int(n_accept.sum())} of {KEEP * Cn}")
    if kern.startswith("gemm_step_kernel"):
        ticks, busy, slots = mcmc_amd.test_gemm_nuts_last_ticks()
        line += f"; {ticks} ticks ({ms / max(ticks, 1):.3f} ms per tick)"
    if not quiet: say(line)
    return ms


def bounded_part(n_rows, calls, literal_max, counts=(128, 1024, 8192, 65536)):
    import mcmc_amd
    plain = {Cn: run(Cn, mcmc_amd.KERNEL_AUTO, calls, None, n_rows) for Cn in counts if Cn <= 8192}
    for pattern in ("a", "b"):
        for Cn in counts:
            t = run(Cn, mcmc_amd.KERNEL_AUTO, calls, pattern, n_rows)
            if Cn in plain: say(f"    bounded (pattern {pattern}) / unbounded on the route: {t / plain[Cn]:.2f}x")
            if Cn <= literal_max:      # the parent's behaviour: the same call on literal_kernel<2> (many seconds: one call, beyond 1 024 chains without a warm-up)
                tl = run(Cn, mcmc_amd.KERNEL_LITERAL, 1, pattern, n_rows, warm=False)
                say(f"    literal_kernel<2> / route: {tl / t:.1f}x")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="dense")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--log", default="profiles/gemm_nuts_bounds_time.log")
    ap.add_argument("--literal-max", type=int, default=8192)
    ap.add_argument("--lib-a", default="")
    ap.add_argument("--lib-b", default="")
    ap.add_argument("--counts", default="128,1024,8192,65536")      # the chain counts of --part dense / logit
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0)
    a = ap.parse_args()
    LOG = a.log
    if a.part == "ab-child":                            # one library (MI_MCMC_LIB), one shape: a warm-up and one timed call; the time on the last line
        LOG = None
        print("ms", run(a.chains, 0, 1, None, a.rows, quiet=True))
        sys.exit(0)
    counts = tuple(int(c) for c in a.counts.split(","))
    if a.part == "dense": bounded_part(0, a.calls, a.literal_max, counts)
    if a.part == "logit": bounded_part(N_ROWS, a.calls, a.literal_max, counts)
    if a.part == "ab":
        for rows in ((a.rows,) if a.chains else (0, N_ROWS)):        # (--chains / --rows: that shape alone)
            for Cn in ((a.chains,) if a.chains else (1024, 65536)):
                t = {"A": [], "B": []}
                for rep in range(a.calls):
                    for name, lib in (("A", a.lib_a), ("B", a.lib_b)):
                        env = dict(os.environ, MI_MCMC_LIB=lib)
                        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "ab-child", "--chains", str(Cn), "--rows", str(rows)],
                                             env=env, capture_output=True, text=True, timeout=600)
                        if out.returncode != 0:
                            say(f"A/B child failed: rc={out.returncode} {out.stderr[-400:]}")
                            sys.exit(1)
                        t[name].append(float(out.stdout.strip().splitlines()[-1].split()[1]))
                ma, mb = float(np.median(t["A"])), float(np.median(t["B"]))
                say(f"unbounded nuts {'logistic N=%d' % rows if rows else 'dense'} d={D} C={Cn}, alternating A/B, median of {a.calls}: A ({a.lib_a}) {ma:.1f} ms "
                    f"(min {min(t['A']):.1f} max {max(t['A']):.1f}), B ({a.lib_b}) {mb:.1f} ms (min {min(t['B']):.1f} max {max(t['B']):.1f}), B / A = {mb / ma:.4f}, "
                    f"A's own spread {(max(t['A']) - min(t['A'])) / ma:.4f}")
