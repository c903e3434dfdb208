"""mcmc::nuts beyond d = 512 on the matrix-product route (gemm_nuts.hpp: per-chain memoised trees, one product per tick for all chains) against literal_kernel<2>,
which served such a call before (the same call with MI_KERNEL_LITERAL: the same bits).  HIP events around the C-ABI call on device buffers, one warm-up call, the
median of N timed calls; per shape the ticks run, the share of (tick, chain) slots in which the chain took no point, and the fraction of the fp64 matrix peak on
the EXECUTED leapfrogs.  (GPU box)  python tools/gemm_nuts_time.py [--part route|literal|logit|prof|all] [--calls 3] [--log profiles/gemm_nuts_time.log]
--part prof starts `rocprofv3 --kernel-trace --stats` on one call of the 65 536-chain shape (a child process) and copies its kernel stats next to the log."""
import argparse, glob, os, shutil, subprocess, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth

PEAK = 78.6      # TFLOP/s, fp64 matrix
D, DEPTH, N_ADAPT, BURN, KEEP = 1024, 6, 10, 10, 10
LOG = None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def run(Cn, hint, calls, warm=True, n_rows=0):
    d = D
    init = synth.initial_states(Cn, d, seed=3) * (0.1 if n_rows else 0.5)
    theta0 = torch.from_numpy(np.ascontiguousarray(init.T)).cuda()
    st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=BURN, n_keep_draws=KEEP, n_adapt_draws=N_ADAPT, max_tree_depth=DEPTH, step_size=0.1)
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
    line = (f"nuts {'logistic N=%d' % n_rows if n_rows else 'dense'} d={d} C={Cn} max_tree_depth={DEPTH} n_adapt={N_ADAPT} draws={BURN}+{KEEP}: {ms:.1f} ms (median of {len(times)}"
            f"{'' if warm else ', no warm-up'}, min {min(times):.1f} max {max(times):.1f}), kernel {kern}, leapfrogs executed {ex} of the reference's {le}, "
            f"{tf:.2f} TFLOP/s on executed flops = {tf / PEAK:.4f} of the fp64 matrix peak, accepts {int(n_accept.sum())} of {KEEP * Cn}")
    if kern.startswith("gemm_step_kernel"):
        ticks, busy, slots = mcmc_amd.test_gemm_nuts_last_ticks()
        line += f"; {ticks} ticks ({ms / max(ticks, 1):.3f} ms per tick), {1.0 - busy / max(slots, 1):.3f} of the (tick, chain) slots idle"
    say(line)
    return ms


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--log", default="profiles/gemm_nuts_time.log")
    a = ap.parse_args()
    LOG = a.log
    if a.part == "prof-child":                          # under rocprofv3: one shape, nothing else
        LOG = None
        run(65536, mcmc_amd.KERNEL_AUTO, 1, warm=False)
        sys.exit(0)
    route = {}
    if a.part in ("route", "all"):
        for Cn in (128, 1024, 8192, 65536):
            route[Cn] = run(Cn, mcmc_amd.KERNEL_AUTO, a.calls)
    if a.part in ("literal", "all"):                    # the parent's behaviour: the same call on literal_kernel<2> (8 192 chains: one call, it takes many seconds)
        for Cn in (128, 1024, 8192):
            t = route.get(Cn) or run(Cn, mcmc_amd.KERNEL_AUTO, a.calls)
            tl = run(Cn, mcmc_amd.KERNEL_LITERAL, 1 if Cn > 1024 else min(a.calls, 2), warm=Cn <= 1024)
            say(f"    literal_kernel<2> / route: {tl / t:.1f}x")
    if a.part in ("logit", "all"):
        run(8192, mcmc_amd.KERNEL_AUTO, a.calls, n_rows=4096)
        t1 = run(128, mcmc_amd.KERNEL_AUTO, a.calls, n_rows=4096)
        tl = run(128, mcmc_amd.KERNEL_LITERAL, 1, n_rows=4096)
        say(f"    logistic, 128 chains: literal_kernel<2> / route: {tl / t1:.1f}x")
    if a.part in ("prof", "all"):
        out = os.path.join(os.path.dirname(os.path.abspath(a.log)), "gemm_nuts_prof")
        env = dict(os.environ, TMPDIR="/tmp")
        rc = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--part", "prof-child"],
                            env=env, timeout=900).returncode
        stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if rc == 0 and stats:
            shutil.copy(stats[0], os.path.splitext(a.log)[0] + "_kernel_stats.csv")
            say(f"kernel stats of one call at C=65536: {os.path.splitext(a.log)[0]}_kernel_stats.csv")
        else:
            say(f"rocprofv3 run: rc={rc}, no kernel stats")
