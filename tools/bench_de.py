"""mcmc::de many-population throughput: d = 128 dense Gaussian, 16 384 populations, device-resident, HIP-event timed.

Proposals per second of de_gauss_mfma_kernel and de_literal_kernel (MI_KERNEL_LITERAL) and, in the same process on the same GPU,
rwmh on 16 384 chains of the same target.  Roofline of the tile kernel: 2 d^2 flop per proposal (the mat-vec) against its row traffic,
(3 + accept + kept) 8 d bytes (rows i, c1, c2 read; row i written on accept; row i written into draws when the generation is kept).
One JSON line per kernel."""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--pops", type=int, default=16384)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--n-pop", type=int, default=16)
ap.add_argument("--burn", type=int, default=10)
ap.add_argument("--keep", type=int, default=10)
ap.add_argument("--literal-gens", type=int, default=2, help="generations of the (slow) literal kernel's run")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
P, d, n_pop = a.pops, a.d, a.n_pop
HBM_BPS, FP64_MFMA = 8.0e12, 78.6e12          # MI355X: HBM3E 8 TB/s, fp64 matrix peak
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
prec = torch.from_numpy(synth.dense_gaussian_precision(d)).to(dev)
init = torch.from_numpy(np.ascontiguousarray(synth.initial_states(P, d, seed=3).T)).to(dev)


def timed(fn):
    best = None
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


def run_de(hint, burn, keep):
    pop = torch.empty((n_pop, d, P), dtype=torch.float64, device=dev)
    draws = torch.empty((keep, n_pop, d, P), dtype=torch.float64, device=dev)
    acc = torch.zeros(P, dtype=torch.int64, device=dev)
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=prec, mem=mcmc_amd.MEM_DEVICE, kernel_hint=hint)
    s = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=burn, n_keep_draws=keep)
    ds = mcmc_amd.de_settings(n_pop=n_pop)
    p = mcmc_amd.mi_populations()
    p.struct_size, p.mem, p.n_populations = C.sizeof(mcmc_amd.mi_populations), mcmc_amd.MEM_DEVICE, P
    p.initial_vals, p.population, p.draws, p.n_accept = init.data_ptr(), pop.data_ptr(), draws.data_ptr(), acc.data_ptr()
    fn = lambda: mcmc_amd._check(mcmc_amd.lib().mi_mcmc_de_run(C.byref(t), C.byref(s), C.byref(ds), C.byref(p), stream))
    fn(); torch.cuda.synchronize()                    # first call: workspace, code objects
    ms = timed(fn)
    gens = burn + keep
    props = P * n_pop * gens
    acc_rate = float(acc.double().sum()) / (P * n_pop * keep) if keep else 0.0
    bytes_ = props * 8.0 * d * 3 + P * n_pop * (acc_rate * gens + keep) * 8.0 * d
    flops = props * 2.0 * d * d
    r = {"algo": "de", "kernel": mcmc_amd.last_kernel(), "populations": P, "n_pop": n_pop, "d": d, "generations": gens, "ms": ms,
         "proposals_per_s": props / (ms * 1e-3), "accept": acc_rate, "flop_per_byte": flops / bytes_,
         "hbm_TBps": bytes_ / (ms * 1e-3) / 1e12, "frac_hbm_bound": bytes_ / (ms * 1e-3) / HBM_BPS,
         "TFLOPs": flops / (ms * 1e-3) / 1e12, "frac_fp64_mfma_peak": flops / (ms * 1e-3) / FP64_MFMA}
    print(json.dumps(r), flush=True)
    return r


def run_rwmh(burn, keep):
    theta = torch.empty_like(init)
    draws = torch.empty((keep, d, P), dtype=torch.float64, device=dev)
    nacc = torch.zeros(P, dtype=torch.int64, device=dev)
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=prec, mem=mcmc_amd.MEM_DEVICE)
    st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=burn, n_keep_draws=keep, step_size=0.05)
    ch = mcmc_amd.make_chains(theta, P, draws=draws, n_accept=nacc, mem=mcmc_amd.MEM_DEVICE)
    def fn():
        theta.copy_(init)
        mcmc_amd.run("rwmh", t, st, ch, stream=stream)
    fn(); torch.cuda.synchronize()
    ms = timed(fn)
    r = {"algo": "rwmh", "kernel": mcmc_amd.last_kernel(), "chains": P, "d": d, "draws": burn + keep, "ms": ms,
         "proposals_per_s": P * (burn + keep) / (ms * 1e-3)}
    print(json.dumps(r), flush=True)
    return r


tile = run_de(mcmc_amd.KERNEL_AUTO, a.burn, a.keep)
lit = run_de(mcmc_amd.KERNEL_LITERAL, 0, a.literal_gens)
rw = run_rwmh(a.n_pop * a.burn, a.n_pop * a.keep)     # as many proposals per chain as a population makes
print(json.dumps({"summary": "de vs rwmh", "tile_over_rwmh": tile["proposals_per_s"] / rw["proposals_per_s"],
                  "tile_over_literal": tile["proposals_per_s"] / lit["proposals_per_s"]}), flush=True)
