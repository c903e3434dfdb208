"""mi_mcmc_draws_covariance (mcmc_amd/csrc/draws_cov.hip) on the GPU box: time per call (HIP events around the call on its stream, median of 5 after a
warm-up; the two host outputs are pinned memory) and the achieved fraction of the least time the hardware could take,
    max(8 d K bytes / HBM rate, d^2 K flop / fp64 matrix peak),
with the slab read ONCE (the call reads it twice: the means, then the products) and d^2 K the flops of the LOWER TRIANGLE of the product (2 flop per
multiply-add, half the matrix; the kernel computes the tiles with tj <= ti).  Peaks: 8.0 TB/s (HBM3E, spec), 78.6 TFLOP/s (fp64 MFMA).  Yardstick, not a
pass criterion: torch.matmul of the centred fp64 slab [d, K] with its transpose on the same device (the full product, timed alone: its centring and its
transposition of the slab are not counted).  Then one dense-mass-adapted hmc run on synth.dense_gaussian_precision(128), 65 536 chains: wall time and the
estimates' share of it.   python tools/draws_cov_time.py [--out profiles/draws_cov_time.log]"""
import argparse, ctypes as C_, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth

HBM, PEAK = 8.0e12, 78.6e12
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "draws_cov_time.log"))
ap.add_argument("--shapes", default="128x100x65536,1024x1x65536,512x1x8192")          # d x n_keep x C
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("no GPU: nothing is measured (there is no CPU path)")
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

def median_ms(fn, n=5):
    fn(); torch.cuda.synchronize()                       # warm-up
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts

say(f"device: {torch.cuda.get_device_name(0)}; peaks used: HBM {HBM / 1e12:.1f} TB/s, fp64 matrix {PEAK / 1e12:.1f} TFLOP/s; flops counted: d^2 K (lower triangle)")
stream = torch.cuda.current_stream().cuda_stream
for shp in args.shapes.split(","):
    d, n_keep, C = map(int, shp.split("x"))
    K = n_keep * C
    g = torch.Generator(device="cuda"); g.manual_seed(d + C)
    slab = torch.randn((n_keep, d, C), dtype=torch.float64, device="cuda", generator=g) + torch.linspace(-10, 10, d, dtype=torch.float64, device="cuda")[None, :, None]
    mean_t, cov_t = torch.empty(d, dtype=torch.float64).pin_memory(), torch.empty((d, d), dtype=torch.float64).pin_memory()     # the caller's host arrays: pinned
    def call():
        rc = mcmc_amd.lib().mi_mcmc_draws_covariance(slab.data_ptr(), mcmc_amd.MEM_DEVICE, n_keep, d, C,
                                                     mean_t.data_ptr(), cov_t.data_ptr(), stream)
        assert rc == 0, mcmc_amd.lib().mi_mcmc_last_error()
    ms, ts = median_ms(call)
    t_hbm, t_mfma = 8.0 * d * K / HBM, float(d) * d * K / PEAK
    bound = max(t_hbm, t_mfma)
    cov = cov_t.numpy()
    E = (slab.permute(1, 0, 2).reshape(d, K) - slab.mean(dim=(0, 2))[:, None]).contiguous()
    ref = {}
    def mm():
        ref["r"] = torch.matmul(E, E.t())
    ms_mm, ts_mm = median_ms(mm)
    rel = float((torch.from_numpy(cov).cuda() - ref["r"] / (K - 1)).abs().max() / (ref["r"] / (K - 1)).abs().max())
    say(f"d={d} n_keep={n_keep} C={C} (K={K}): draws_covariance {ms:.3f} ms (5 runs: {' '.join(f'{t:.3f}' for t in ts)}); least time {bound * 1e3:.3f} ms "
        f"({'HBM' if t_hbm >= t_mfma else 'matrix'}-bound: {t_hbm * 1e3:.3f} ms of bytes, {t_mfma * 1e3:.3f} ms of flops) -> {bound * 1e3 / ms:.3f} of it; "
        f"torch.matmul(E, E^T) alone {ms_mm:.3f} ms ({' '.join(f'{t:.3f}' for t in ts_mm)}); max |cov - torch| / max |cov| = {rel:.2e}")
    del slab, E, ref

# the adaptation end to end: hmc on the headline target, device-resident chains
d, C, burn, keep, L, n_windows = 128, 65536, 60, 20, 16, 3
prec = torch.from_numpy(synth.dense_gaussian_precision(d)).cuda()
tgt = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=prec, mem=mcmc_amd.MEM_DEVICE)
init = torch.from_numpy(np.ascontiguousarray(synth.initial_states(C, d, seed=3).T)).cuda()
st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=burn, n_keep_draws=keep, n_leap_steps=L, step_size=0.25)
draws = torch.empty((keep, d, C), dtype=torch.float64, device="cuda")
nacc = torch.zeros(C, dtype=torch.int64, device="cuda")
def adapted():
    theta = init.clone()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    M = mcmc_amd.hmc_mass_adapted_dense(tgt, st, mcmc_amd.make_chains(theta, C, draws=draws, n_accept=nacc, mem=mcmc_amd.MEM_DEVICE), n_windows=n_windows, stream=stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, M, theta
adapted()
wall, M, theta = adapted()
def estimate():                                          # what the call does between its parts (on a NEW matrix each time: nothing memoised)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    _, S = mcmc_amd.draws_covariance(theta, 1, d, C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_mean=False)
    a, b = C / (C + 5.0), 1e-3 * (5.0 / (C + 5.0))
    Sp = a * S * (1.0 + estimate.n * 2.0 ** -30); Sp[np.diag_indices(d)] += b
    M0 = mcmc_amd.mat_inverse(Sp); mcmc_amd.mat_cholesky_lower(0.5 * (M0 + M0.T))
    estimate.n += 1
    return time.perf_counter() - t0
estimate.n = 0
estimate()
est = float(np.median([estimate() for _ in range(5)]))
say(f"hmc_mass_adapted_dense on dense_gaussian_precision({d}), C={C}, {burn}+{keep} draws, L={L}, n_windows={n_windows}: wall {wall * 1e3:.1f} ms, kernel {mcmc_amd.last_kernel()}, "
    f"acceptance {float(nacc.double().mean()) / keep:.3f}; one estimate (covariance, INV, CHOL_LOWER, host clock) {est * 1e3:.2f} ms x {n_windows + 1} = "
    f"{(n_windows + 1) * est / wall:.4f} of the wall time")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
