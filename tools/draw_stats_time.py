"""Time mi_mcmc_draw_stats(want_acov=False) -- the ESS leg of the benchmark: the one-pass Gram kernel -- on a device-resident slab of the benchmark's
shape, (n_keep, d, C) = (100, 128, 65536), synthetic AR(1) draws (GPU box).  One warm-up, then 5 calls, host clock around the blocking call.  The
library under test is the in-tree one, or the one MI_MCMC_LIB names (an A/B build of another commit: run both in one session and compare the lists;
the margin is the min-max spread of the older one's five).  Appends one line per run to the log.
    python tools/draw_stats_time.py [--label parent] [--out profiles/draw_stats_variance_time.log]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch, mcmc_amd

ap = argparse.ArgumentParser()
ap.add_argument("--label", default="this tree")
ap.add_argument("--phi", type=float, default=0.7)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "draw_stats_variance_time.log"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("no GPU: nothing is measured (there is no CPU path)")
n, d, C = 100, 128, 65536
g = torch.Generator(device="cuda").manual_seed(1)
x = torch.empty((n, d, C), dtype=torch.float64, device="cuda")
x[0] = torch.randn((d, C), dtype=torch.float64, device="cuda", generator=g)
for t in range(1, n):
    x[t] = args.phi * x[t - 1] + (1 - args.phi ** 2) ** 0.5 * torch.randn((d, C), dtype=torch.float64, device="cuda", generator=g)
st = torch.cuda.current_stream().cuda_stream
def call():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    s = mcmc_amd.draw_stats(x, n, d, C, mem=mcmc_amd.MEM_DEVICE, stream=st, want_acov=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, s
call()                                                      # warm-up
runs = [call() for _ in range(5)]
ts, s = [r[0] for r in runs], runs[-1][1]
line = (f"{args.label} ({'the library MI_MCMC_LIB names' if os.environ.get('MI_MCMC_LIB') else 'in-tree library'}) on {torch.cuda.get_device_name(0)}: draw_stats(want_acov=False), (n_keep, d, C) = ({n}, {d}, {C}), "
        f"phi = {args.phi}: 5 runs after one warm-up, ms: {' '.join(f'{t:.3f}' for t in ts)}; min {min(ts):.3f} max {max(ts):.3f}; "
        f"ess_min = {s['ess'].min():.6f}, rhat_max = {s['rhat'].max():.12f}")
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write(line + "\n")
