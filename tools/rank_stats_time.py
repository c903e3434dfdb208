"""mi_mcmc_draws_rank_transform and mi_mcmc_draw_stats_ranked (mcmc_amd/csrc/draws_rank.hip) on the GPU box: time per call on a device-resident slab
(HIP events around the blocking C-ABI call on its stream, one warm-up call discarded, then the median of 5 with min .. max), next to the byte model of
DESIGN.md 4.24 per sample and sort
    8 B key write + per executed pass 8 B (count) + 16 B (scatter) + 16 B lookup, plus the 8 B the key pass and the lookup each read of the slab
and the fraction of the 6.29 TB/s copy bandwidth those bytes make.  The passes a sort executes depend on the data (constant digits are skipped): the
tool reads the library's own count of executed passes (mi_mcmc_test_rank_counts).  For context, not pass criteria: mi_mcmc_draw_stats on the
same slab, and the same statistics by mcmc_amd/rank_stats.py on the host for the first --host-dims dimensions (numpy; scaled to d in the printout).
   python tools/rank_stats_time.py [--out profiles/rank_stats_time.log]"""
import argparse, ctypes as C_, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import rank_stats

COPY_BW = 6.29e12
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "rank_stats_time.log"))
ap.add_argument("--shapes", default="128x100x65536,16x60x4096")                         # d x n_keep x C; the first is the README's 6.7 GB slab
ap.add_argument("--host-dims", type=int, default=2)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("no GPU: nothing is measured (there is no CPU path)")
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

def timed(fn, n=5):
    fn(); torch.cuda.synchronize()                       # warm-up
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), min(ts), max(ts)

def counts():
    """(sorts, passes) the library has run so far: one sort per group of dimensions and kind of key, at most eight passes each"""
    so, pa = C_.c_uint64(0), C_.c_uint64(0)
    lib.mi_mcmc_test_rank_counts(C_.byref(so), C_.byref(pa))
    return so.value, pa.value

lib = mcmc_amd.lib()
say(f"device: {torch.cuda.get_device_name(0)}; copy bandwidth used for the fractions: {COPY_BW / 1e12:.2f} TB/s")
stream = torch.cuda.current_stream().cuda_stream
for shp in args.shapes.split(","):
    d, n_keep, C = map(int, shp.split("x"))
    g = torch.Generator(device="cuda"); g.manual_seed(d + C)
    slab = torch.randn((n_keep, d, C), dtype=torch.float64, device="cuda", generator=g) + torch.linspace(-10, 10, d, dtype=torch.float64, device="cuda")[None, :, None]
    h = n_keep // 2
    say(f"d={d} n_keep={n_keep} C={C} (slab {8.0 * d * n_keep * C / 1e9:.3f} GB)")
    for name, flags, sorts in (("plain", 0, 1), ("split", 1, 1), ("split | fold", 3, 2)):
        rows = 2 * h if flags & 1 else n_keep
        n = float(d) * rows * C
        out = torch.empty((h, d, 2 * C) if flags & 1 else (n_keep, d, C), dtype=torch.float64, device="cuda")
        def call():
            rc = lib.mi_mcmc_draws_rank_transform(slab.data_ptr(), mcmc_amd.MEM_DEVICE, n_keep, d, C,
                                                  1, flags, out.data_ptr(), stream)
            assert rc == 0, lib.mi_mcmc_last_error()
        ms, lo, hi = timed(call)
        s0, p0 = counts(); call(); s1, p1 = counts()
        passes = (p1 - p0) / (s1 - s0)                               # mean executed passes per sort (of a group of dimensions)
        model = n * (sorts * (8 + 8 + 24 * passes) + 8 + 16)         # per sort: slab read, key write, passes; once: slab read + lookup
        say(f"  draws_rank_transform NORMAL, {name}: {ms:.3f} ms ({lo:.3f} .. {hi:.3f}); {s1 - s0} sorts of a group, {passes:.2f} of 8 passes executed each; "
            f"model {model / 1e9:.1f} GB -> {model / (ms * 1e-3) / 1e12:.3f} TB/s = {model / (ms * 1e-3) / COPY_BW:.3f} of the copy bandwidth")
        del out
    outs = [torch.empty(d, dtype=torch.float64).pin_memory() for _ in range(5)]
    def ranked():
        rc = lib.mi_mcmc_draw_stats_ranked(slab.data_ptr(), mcmc_amd.MEM_DEVICE, n_keep, d, C,
                                           *[o.data_ptr() for o in outs], stream)
        assert rc == 0, lib.mi_mcmc_last_error()
    ms_r, lo, hi = timed(ranked)
    say(f"  draw_stats_ranked (all five outputs: two sorts, two lookups, two indicator slabs, four passes of draw_stats): {ms_r:.3f} ms ({lo:.3f} .. {hi:.3f})")
    say(f"    rhat max {outs[0].max().item():.5f}, ess_bulk per half-chain min {outs[3].min().item():.2f} of {h}, ess_tail min {outs[4].min().item():.2f}")
    mean_t, rhat_t, ess_t = (torch.empty(d, dtype=torch.float64).pin_memory() for _ in range(3))
    def stats():
        rc = lib.mi_mcmc_draw_stats(slab.data_ptr(), mcmc_amd.MEM_DEVICE, n_keep, d, C,
                                    mean_t.data_ptr(), None, rhat_t.data_ptr(), ess_t.data_ptr(), stream)
        assert rc == 0, lib.mi_mcmc_last_error()
    ms, lo, hi = timed(stats)
    say(f"  context: mi_mcmc_draw_stats (no acov) on the same slab: {ms:.3f} ms ({lo:.3f} .. {hi:.3f})")
    nd = min(d, args.host_dims)
    if nd > 0:
        part = slab[:, :nd, :].contiguous().cpu().numpy()
        t0 = time.perf_counter()
        ref = rank_stats.draw_stats_ranked_ref(part)
        dt = time.perf_counter() - t0
        same = all(np.allclose(ref[k], outs[j][:nd].numpy(), rtol=1e-8) for j, k in enumerate(("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail")))
        say(f"  context: rank_stats.draw_stats_ranked_ref on the host, {nd} of {d} dimensions: {dt:.2f} s, i.e. {dt * d / nd:.1f} s for all of them "
            f"(x {dt * d / nd / (ms_r * 1e-3):.0f} the device call); agrees with the device at rtol 1e-8: {same}")
    del slab
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
