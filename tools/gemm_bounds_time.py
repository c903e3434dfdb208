"""settings.vals_bound beyond d = 512 on the matrix-product route (gemm_samplers.hip, gemm_step_kernel<10 / 11, .>) against the plain route of the same library and
against literal_kernel<.>, which served a bounded call before (the same call with MI_KERNEL_LITERAL).  HIP events around the C-ABI call, one warm-up call, the
median of N timed calls (GPU box): python tools/gemm_bounds_time.py [--part plain|literal|rwmh|prof|all] [--calls 5]
Bound patterns: (a) about a quarter of the dimensions bounded, types 2 / 3 / 4 mixed; (b) every dimension type 4; (c) vals_bound with every bound infinite."""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth

PEAK = 78.6      # TFLOP/s, fp64 matrix


def bounds(d, pattern):
    lo, hi = np.full(d, -np.inf), np.full(d, np.inf)
    if pattern == "a":
        t = np.random.default_rng(d).choice([1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 4], size=d)
        lo[(t == 2) | (t == 4)] = -1.5; hi[(t == 3) | (t == 4)] = 2.0
    elif pattern == "b":
        lo[:], hi[:] = -1.5, 2.0
    return lo, hi


def run(algo, d, Cn, L, nd, pattern, hint, calls):
    init = np.clip(synth.initial_states(Cn, d, seed=3) * 0.3, -1.0, 1.5)
    theta0 = torch.from_numpy(np.ascontiguousarray(init.T)).cuda()
    kw = {}
    if pattern is not None:
        lo, hi = bounds(d, pattern)
        kw = dict(vals_bound=1, lower_bounds=lo, upper_bounds=hi)
    st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=nd // 2, n_keep_draws=nd - nd // 2, n_leap_steps=L, step_size=0.02, **kw)
    draws = torch.empty((nd - nd // 2, d, Cn), dtype=torch.float64, device="cuda")
    n_accept = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    tgt = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=torch.from_numpy(synth.dense_gaussian_precision(d)).cuda(), mem=mcmc_amd.MEM_DEVICE, kernel_hint=hint)
    times = []
    for it in range(calls + 1):                         # (the first call is the warm-up)
        theta = theta0.clone()
        ch = mcmc_amd.make_chains(theta, Cn, draws=draws, n_accept=n_accept, mem=mcmc_amd.MEM_DEVICE)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        mcmc_amd.run(algo, tgt, st, ch)
        e1.record(); torch.cuda.synchronize()
        if it: times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    n_prod = nd * (L if algo == "hmc" else 1) + 1       # gradients of 2 d^2 C flop each (the one at the initial values included)
    tf = n_prod * 2.0 * d * d * Cn / (ms * 1e-3) / 1e12
    acc = float(n_accept.double().mean()) / max(1, nd - nd // 2)
    name = "plain" if pattern is None else f"bounds ({pattern})"
    print(f"{algo} {name} d={d} C={Cn} L={L} draws={nd}: {ms:.1f} ms (median of {calls}, min {min(times):.1f} max {max(times):.1f}), kernel {mcmc_amd.last_kernel()}, "
          f"{tf:.2f} TFLOP/s ({n_prod} products of 2 d^2 C), {tf / PEAK:.3f} of the fp64 matrix peak, accept rate {acc:.2f}", flush=True)
    return ms


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all")
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    d, L = 1024, 16
    if a.part in ("plain", "all"):                      # against the plain route: the same shape without bounds
        base = run("hmc", d, 65536, L, 6, None, mcmc_amd.KERNEL_AUTO, a.calls)
        for p in "abc":
            t = run("hmc", d, 65536, L, 6, p, mcmc_amd.KERNEL_AUTO, a.calls)
            print(f"    {t / base:.3f}x the plain route's time")
    if a.part == "prof":                                # under rocprofv3 --kernel-trace --stats: the plain route and pattern (b), nothing else
        run("hmc", d, 65536, L, 6, None, mcmc_amd.KERNEL_AUTO, a.calls)
        run("hmc", d, 65536, L, 6, "b", mcmc_amd.KERNEL_AUTO, a.calls)
    if a.part in ("literal", "all"):                    # against literal_kernel<0>, what a bounded call ran on before
        for Cn, nd in ((128, 6), (1024, 6), (8192, 2)):
            t = run("hmc", d, Cn, L, nd, "a", mcmc_amd.KERNEL_AUTO, a.calls)
            tl = run("hmc", d, Cn, L, nd, "a", mcmc_amd.KERNEL_LITERAL, min(a.calls, 3) if Cn > 1024 else a.calls)
            print(f"    literal_kernel<0>: {tl:.1f} ms ({tl / t:.1f}x)")
    if a.part in ("rwmh", "all"):
        base = run("rwmh", d, 65536, 0, 40, None, mcmc_amd.KERNEL_AUTO, a.calls)
        t = run("rwmh", d, 65536, 0, 40, "a", mcmc_amd.KERNEL_AUTO, a.calls)
        print(f"    {t / base:.3f}x the plain route's time")
