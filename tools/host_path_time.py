"""Host path of a call: tiny runs (64 chains, one draw) whose wall time is the table derivation, the uploads and the launches.  Median / min of 100 calls."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth
dev = torch.device("cuda", 0)
C = 64
def spd(d):
    A = np.random.default_rng(5).standard_normal((d, d)); return A @ A.T / d + np.eye(d)
def box(d):
    lb = np.full(d, -np.inf); ub = np.full(d, np.inf); lb[: d // 3] = -3.0; ub[d // 4: d // 2] = 3.0; return lb, ub
def case(name, algo, kind, d, **kw):
    prec = None
    if kind == mcmc_amd.TARGET_GAUSS_DENSE: prec = torch.from_numpy(synth.dense_gaussian_precision(d)).to(dev)
    init = np.clip(synth.initial_states(C, d, seed=3) * 0.3, -1.0, 1.0)
    theta0 = torch.from_numpy(np.ascontiguousarray(init.T)).to(dev)
    st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=0, n_keep_draws=1, n_adapt_draws=0, max_tree_depth=2, n_leap_steps=1, step_size=0.05, **kw)
    t = mcmc_amd.make_target(kind, d, prec=prec, mem=mcmc_amd.MEM_DEVICE)
    ts = []
    for it in range(105):
        theta = theta0.clone()
        ch = mcmc_amd.make_chains(theta, C, mem=mcmc_amd.MEM_DEVICE)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        mcmc_amd.run(algo, t, st, ch); torch.cuda.synchronize()
        if it >= 5: ts.append((time.perf_counter() - t0) * 1e6)
    print("host path %-44s median %8.1f us   min %8.1f us   (%s)" % (name, np.median(ts), min(ts), mcmc_amd.last_kernel()), flush=True)
D = mcmc_amd.TARGET_GAUSS_DENSE
lb, ub = box(128)
case("hmc d=128 diag precond + bounds", "hmc", D, 128, precond_mat=np.diag(np.linspace(0.5, 2.0, 128)), vals_bound=1, lower_bounds=lb, upper_bounds=ub)
case("hmc d=128 diag precond", "hmc", D, 128, precond_mat=np.diag(np.linspace(0.5, 2.0, 128)))
case("hmc d=128 dense precond", "hmc", D, 128, precond_mat=spd(128))
case("mala d=128 dense precond", "mala", D, 128, precond_mat=spd(128))
case("mala d=128 diag precond + bounds", "mala", D, 128, precond_mat=np.diag(np.linspace(0.5, 2.0, 128)), vals_bound=1, lower_bounds=lb, upper_bounds=ub)
case("rwmh d=128 dense cov + bounds", "rwmh", D, 128, precond_mat=spd(128), vals_bound=1, lower_bounds=lb, upper_bounds=ub)
case("nuts d=128 diag precond + bounds", "nuts", D, 128, precond_mat=np.diag(np.linspace(0.5, 2.0, 128)), vals_bound=1, lower_bounds=lb, upper_bounds=ub)
case("hmc iso d=200 diag precond (elementwise)", "hmc", mcmc_amd.TARGET_GAUSS_ISO, 200, precond_mat=np.diag(np.linspace(0.5, 2.0, 200)))
lb, ub = box(192)
case("hmc d=192 diag precond + bounds (LDS)", "hmc", D, 192, precond_mat=np.diag(np.linspace(0.5, 2.0, 192)), vals_bound=1, lower_bounds=lb, upper_bounds=ub)
case("mala d=192 diag precond (LDS)", "mala", D, 192, precond_mat=np.diag(np.linspace(0.5, 2.0, 192)))
case("mala d=192 dense precond (LDS)", "mala", D, 192, precond_mat=spd(192))
lb, ub = box(520)
case("hmc d=520 diag precond + bounds (matrix-product)", "hmc", D, 520, precond_mat=np.diag(np.linspace(0.5, 2.0, 520)), vals_bound=1, lower_bounds=lb, upper_bounds=ub)
# the plain variants of the matrix-product route: identity precond_mat, no bounds (capacity is a routing condition for them too: one hipMemGetInfo per call)
case("hmc d=520 (matrix-product, plain)", "hmc", D, 520)
case("rwmh d=520 (matrix-product, plain)", "rwmh", D, 520)
