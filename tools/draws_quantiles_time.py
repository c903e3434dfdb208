"""mi_mcmc_draws_order_stats (mcmc_amd/csrc/draws_select.hip) on the GPU box: time per call for 1, 3 (the 5 / 50 / 95 % ranks) and 32 ranks (HIP events
around the blocking call on its stream, one warm-up, then the median of 5 with min .. max; the host output is pinned memory), next to the byte model
    8 rounds x the slab = 8 x 8 d K bytes read
(the histograms and the state are small next to it), the effective rate those bytes make and its fraction of 8.0 TB/s (HBM3E, spec).  Yardsticks on the
same slab in the same session, not pass criteria: mi_mcmc_draw_stats (ESS / R-hat only: one or two reads of the slab), and torch.sort along the pooled
axis of a [d, K] copy where that copy fits (the sort alone is timed, not the copy).   python tools/draws_quantiles_time.py [--out profiles/draws_quantiles_time.log]"""
import argparse, ctypes as C_, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd

HBM = 8.0e12
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "draws_quantiles_time.log"))
ap.add_argument("--shapes", default="128x100x65536,1024x1x65536,512x1x8192")          # d x n_keep x C
ap.add_argument("--no-sort", action="store_true", help="leave the torch.sort yardstick out")
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

say(f"device: {torch.cuda.get_device_name(0)}; byte model: 8 rounds x 8 d K bytes; HBM peak used {HBM / 1e12:.1f} TB/s")
stream = torch.cuda.current_stream().cuda_stream
lib = mcmc_amd.lib()
for shp in args.shapes.split(","):
    d, n_keep, C = map(int, shp.split("x"))
    K = n_keep * C
    g = torch.Generator(device="cuda"); g.manual_seed(d + C)
    slab = torch.randn((n_keep, d, C), dtype=torch.float64, device="cuda", generator=g) + torch.linspace(-10, 10, d, dtype=torch.float64, device="cuda")[None, :, None]
    nbytes = 8.0 * 8.0 * d * K
    say(f"d={d} n_keep={n_keep} C={C} (K={K}, slab {8.0 * d * K / 1e9:.3f} GB, the rounds read {nbytes / 1e9:.3f} GB)")
    for n_ranks in (1, 3, 32):
        ranks = {1: [K // 2], 3: [int(0.05 * (K - 1)), (K - 1) // 2, int(0.95 * (K - 1))], 32: [int(r) for r in np.linspace(0, K - 1, 32)]}[n_ranks]
        ranks_a = np.array(ranks, dtype=np.uint64)
        out_t = torch.empty((n_ranks, d), dtype=torch.float64).pin_memory()
        def call():
            rc = lib.mi_mcmc_draws_order_stats(slab.data_ptr(), mcmc_amd.MEM_DEVICE, n_keep, d, C,
                                               ranks_a.ctypes.data, n_ranks, out_t.data_ptr(), stream)
            assert rc == 0, lib.mi_mcmc_last_error()
        ms, lo, hi = timed(call)
        rate = nbytes / (ms * 1e-3)
        say(f"  draws_order_stats, {n_ranks:2d} ranks: {ms:.3f} ms ({lo:.3f} .. {hi:.3f}); {rate / 1e12:.3f} TB/s effective = {rate / HBM:.3f} of peak")
    mean_t, rhat_t, ess_t = (torch.empty(d, dtype=torch.float64).pin_memory() for _ in range(3))
    def stats():
        rc = lib.mi_mcmc_draw_stats(slab.data_ptr(), mcmc_amd.MEM_DEVICE, n_keep, d, C,
                                    mean_t.data_ptr(), None, rhat_t.data_ptr(), ess_t.data_ptr(), stream)
        assert rc == 0, lib.mi_mcmc_last_error()
    try:
        ms, lo, hi = timed(stats)
        say(f"  yardstick mi_mcmc_draw_stats (no acov): {ms:.3f} ms ({lo:.3f} .. {hi:.3f}); one read of the slab in that time = {8.0 * d * K / (ms * 1e-3) / 1e12:.3f} TB/s")
    except AssertionError as e:
        say(f"  yardstick mi_mcmc_draw_stats: refused this shape ({e})")
    if not args.no_sort:
        try:
            flat = slab.permute(1, 0, 2).reshape(d, K).contiguous()
            res = {}
            def srt():
                res["v"] = torch.sort(flat, dim=1).values
            ms, lo, hi = timed(srt)
            say(f"  yardstick torch.sort of the [d, K] copy along K: {ms:.3f} ms ({lo:.3f} .. {hi:.3f})")
            chk = res["v"][:, torch.from_numpy(np.array(ranks, dtype=np.int64)).cuda()].t().contiguous().cpu().numpy()
            say(f"    the last call's {n_ranks} order statistics equal the sorted copy's: {bool(np.array_equal(chk, out_t.numpy()))}")
            del flat, res
        except torch.cuda.OutOfMemoryError:
            say("  yardstick torch.sort: the copy does not fit")
    del slab
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
