"""mcmc::aees many-run throughput, device-resident, HIP-event timed.

Two cases:
  mixture  the example's flow (examples/aees_mixture.cpp): 2-D two-component mixture, T = (60, 9), 11 rings, ee_prob 0.05,
           cov 0.35 I, 1000 initial / 1000 burn-in / 20 000 kept draws; 4 096 runs by default.
  dense    a d = 64 dense Gaussian at the reference's aees_settings_t defaults (1000 / 1000 / 1000 draws, 5 rings, ee_prob 0.1,
           identity cov) with T = (60, 9) added (the defaults have no temper_vec: one level, no history); 1 024 runs.
Each case is timed twice: as given, and with ee_prob_par = 0 (every step an MH step: the same target evaluations per level-step
and the same history stores, but no equi-energy step and so no index upkeep).  The difference is the time the equi-energy steps
add over MH steps: their index merges and order statistics.  The model of the index traffic: every equi-energy step of a level
k >= 2 merges the whole window of m entries, 2 x 12 bytes each (read and written once).  One JSON line per timing."""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=["mixture", "dense", "both"], default="both")
ap.add_argument("--runs", type=int, default=0, help="0: 4096 (mixture) / 1024 (dense)")
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()
HBM_BPS = 8.0e12
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream


def timed(fn):
    best = None
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


def slot_bytes(d, K, S, n_total):
    """aees.hpp: aees_slot_bytes -- one run's history"""
    L = lambda j: n_total - j * S
    b = sum(L(j) * d * 8 for j in range(K - 1)) + sum(L(j) * 8 for j in range(1, K - 1)) + sum(L(k - 1) * 24 for k in range(2, K))
    return (b + 255) & ~255


def index_model_bytes(K, S, n_total, ee):
    """expected index traffic of one run: levels k >= 2, ee_prob of the draws n > k S, a merge over m = n - (k-1) S + 1 entries"""
    tot = 0.0
    for k in range(2, K):
        n = np.arange(k * S + 1, n_total, dtype=np.float64)
        tot += ee * float((n - (k - 1) * S + 1).sum()) * 24.0
    return tot


def run(case, P, ee_override=None):
    if case == "mixture":
        d, T, n_init, burn, keep, rings, ee = 2, [60.0, 9.0], 1000, 1000, 20000, 11, 0.05
        t = mcmc_amd.mixture_target(np.array([[-2.0, -2.0], [2.0, 2.0]]), np.array([0.1, 0.1]), np.array([0.5, 0.5]))
        cov = 0.35 * np.eye(2)
        init = np.tile([-2.0, -2.0], (P, 1))
    else:
        d, T, n_init, burn, keep, rings, ee = 64, [60.0, 9.0], 1000, 1000, 1000, 5, 0.10
        prec = synth.dense_gaussian_precision(d)
        t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=prec)
        cov = None
        init = synth.initial_states(P, d, seed=3)
    if ee_override is not None:
        ee = ee_override
    K, S = len(T) + 1, n_init + burn
    n_total = keep + K * S
    iv = torch.from_numpy(np.ascontiguousarray(init.T)).to(dev)
    draws = torch.empty((keep, d, P), dtype=torch.float64, device=dev)
    fin = torch.empty((K, d, P), dtype=torch.float64, device=dev)
    acc = torch.zeros((K, P), dtype=torch.int64, device=dev)
    eea = torch.zeros((K, P), dtype=torch.int64, device=dev)
    s = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=burn, n_keep_draws=keep)
    ae = mcmc_amd.aees_settings(n_initial_draws=n_init, n_rings=rings, ee_prob_par=ee, temper_vec=T, cov_mat=cov)
    r = mcmc_amd.mi_aees_runs()
    r.struct_size, r.mem, r.n_runs = C.sizeof(mcmc_amd.mi_aees_runs), mcmc_amd.MEM_DEVICE, P
    r.initial_vals, r.draws, r.final_states, r.n_accept, r.n_ee_accept = iv.data_ptr(), draws.data_ptr(), fin.data_ptr(), acc.data_ptr(), eea.data_ptr()
    fn = lambda: mcmc_amd._check(mcmc_amd.lib().mi_mcmc_aees_run(C.byref(t), C.byref(s), C.byref(ae), C.byref(r), stream))
    fn(); torch.cuda.synchronize()                     # first call: workspace, code objects
    ms = timed(fn)
    level_steps = P * sum(n_total - (k * S + 1 if k else 0) for k in range(K))     # active level-steps (level k: draws n > k S)
    slot = slot_bytes(d, K, S, n_total)
    idx = index_model_bytes(K, S, n_total, ee) * P
    far = float((draws[:, 0, :] > 0).double().mean()) if case == "mixture" else None
    res = {"algo": "aees", "case": case, "kernel": mcmc_amd.last_kernel(), "runs": P, "d": d, "K": K, "n_total": n_total, "ee_prob": ee,
           "ms": ms, "level_steps_per_s": level_steps / (ms * 1e-3), "history_bytes_per_run": slot,
           "workspace_bytes": min(P, 2048) * slot, "index_model_bytes": idx, "index_model_ms_at_hbm": idx / HBM_BPS * 1e3,
           "mh_accept_T1": float(acc[K - 1].double().sum()) / float(P * (n_total - (K - 1) * S - 1)),
           "ee_accepts": int(eea.sum()), "far_mode_share": far}
    print(json.dumps(res), flush=True)
    return res


for case in (["mixture", "dense"] if a.case == "both" else [a.case]):
    P = a.runs or (4096 if case == "mixture" else 1024)
    full = run(case, P)
    mh = run(case, P, ee_override=0.0)
    print(json.dumps({"summary": case, "ms": full["ms"], "ms_ee0": mh["ms"], "equi_energy_extra_ms": full["ms"] - mh["ms"],
                      "share_of_time_equi_energy": (full["ms"] - mh["ms"]) / full["ms"],
                      "index_model_ms_at_hbm": full["index_model_ms_at_hbm"]}), flush=True)
