"""hmc and mala with a DENSE precond_mat beyond d = 512 on the matrix-product route (gemm_samplers.hip: the products with the mass matrices, gemm_step_kernel<4 .. 8, 0>,
the V_DENSE_M per-draw kernels).  HIP events around the C-ABI call, one warm-up call, the median of N timed calls (GPU box): python tools/gemm_dense_m_time.py [--calls 5]
MI_MCMC_LIB selects the library (A/B against another build)."""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth


def run(algo, d, Cn, L, nd, calls):
    rng = np.random.default_rng(d)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    M = A @ A.T + np.diag(rng.uniform(0.4, 2.5, d))
    theta0 = torch.from_numpy(np.ascontiguousarray((synth.initial_states(Cn, d, seed=3) * 0.3).T)).cuda()
    st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=nd // 2, n_keep_draws=nd - nd // 2, n_leap_steps=L, step_size=0.02, precond_mat=M)
    draws = torch.empty((nd - nd // 2, d, Cn), dtype=torch.float64, device="cuda")
    tgt = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=torch.from_numpy(synth.dense_gaussian_precision(d)).cuda(), mem=mcmc_amd.MEM_DEVICE)
    times = []
    for it in range(calls + 1):                         # (the first call is the warm-up: code objects, INV / CHOL_LOWER of precond_mat)
        theta = theta0.clone()
        ch = mcmc_amd.make_chains(theta, Cn, draws=draws, mem=mcmc_amd.MEM_DEVICE)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        mcmc_amd.run(algo, tgt, st, ch)
        e1.record(); torch.cuda.synchronize()
        if it: times.append(e0.elapsed_time(e1))
    print(f"dense precond_mat {algo} d={d} C={Cn} L={L} draws={nd}: {np.median(times):.1f} ms (median of {calls}, min {min(times):.1f} max {max(times):.1f}), "
          f"kernel {mcmc_amd.last_kernel()}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    run("hmc", 1024, 65536, 16, 6, a.calls)
    run("mala", 1024, 65536, 0, 20, a.calls)
