"""Time mi_mcmc_draw_stats_lags -- every lag of long series on the fp64 matrix cores -- on a device-resident slab of the reference's default length,
(n_keep, d, C) = (1000, 128, 4096), synthetic AR(1) draws (GPU box).  One warm-up, then 5 calls, host clock around the blocking call; the median is
reported next to the five.
  1. every lag, with and without acov, at phi = 0.7 and phi = 0.99, and the fraction of the fp64 matrix peak the call reaches: the floor is
     sum_delta (NB - delta) = 2 016 MFMAs of 64 cycles per chain quad and dimension, 128 dimensions x 1 024 quads over 1 024 SIMDs at 2.4 GHz = 6.9 ms
     (a derived figure);
  2. K = 127 against mi_mcmc_draw_stats on the same slab, alternating: the same 128 lags, one on the matrix cores and one on the VALU.
Appends its lines to the log.
    python tools/draw_stats_lags_time.py [--out profiles/draw_stats_lags_time.log]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch, mcmc_amd

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "draw_stats_lags_time.log"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("no GPU: nothing is measured (there is no CPU path)")
n, d, C = 1000, 128, 4096
FLOOR_MS = 2016 * d * (C // 4) * 64 / 1024 / 2.4e9 * 1e3
st = torch.cuda.current_stream().cuda_stream
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)


def say(line):
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def slab(phi):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((n, d, C), dtype=torch.float64, device="cuda")
    x[0] = torch.randn((d, C), dtype=torch.float64, device="cuda", generator=g)
    for t in range(1, n):
        x[t] = phi * x[t - 1] + (1 - phi ** 2) ** 0.5 * torch.randn((d, C), dtype=torch.float64, device="cuda", generator=g)
    return x


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    s = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, s


def fmt(ts):
    return f"ms: {' '.join(f'{t:.2f}' for t in ts)}; median {statistics.median(ts):.2f}"


dev = torch.cuda.get_device_name(0)
for phi in (0.7, 0.99):
    x = slab(phi)
    lags = lambda K, acov: mcmc_amd.draw_stats_lags(x, K, n, d, C, mem=mcmc_amd.MEM_DEVICE, stream=st, want_acov=acov)
    for acov in (True, False):
        timed(lambda: lags(None, acov))                       # warm-up
        runs = [timed(lambda: lags(None, acov)) for _ in range(5)]
        ts, s = [r[0] for r in runs], runs[-1][1]
        p = mcmc_amd.test_draw_stats_lags_last()
        say(f"draw_stats_lags every lag, want_acov={acov}, on {dev}: (n_keep, d, C) = ({n}, {d}, {C}), phi = {phi}: 5 runs after one warm-up, {fmt(ts)}; "
            f"bands {p['bands']} subset passes {p['subset_passes']} smallest subset {p['smallest_subset']}; matrix floor {FLOOR_MS:.2f} ms = "
            f"{100 * FLOOR_MS / statistics.median(ts):.1f} % of the call; ess_min = {s['ess'].min():.6f}, ended = {int(s['ended'].sum())} of {d}")
    if phi == 0.7:
        old = lambda: mcmc_amd.draw_stats(x, n, d, C, mem=mcmc_amd.MEM_DEVICE, stream=st, want_acov=True)
        timed(lambda: lags(127, True)); timed(old)             # warm-up of both
        ta, tb = [], []
        for _ in range(5):
            ta.append(timed(lambda: lags(127, True))[0])
            tb.append(timed(old)[0])
        say(f"K = 127 with acov, alternating, phi = {phi}: draw_stats_lags {fmt(ta)} | draw_stats (streamed VALU kernel, the same 128 lags) {fmt(tb)}")
    del x
    torch.cuda.empty_cache()
