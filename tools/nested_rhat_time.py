"""mi_mcmc_draw_stats_nested (mcmc_amd/csrc/draws_nested.hip) on the GPU box: time per call on device slabs -- HIP events around the blocking call on its
stream, ONE warm-up call discarded, then the median of 7 with every run listed (the spread); the host outputs are pinned memory.  Shapes: bench.py's
configs[1] slab (100 x 128 x 65 536, M = 64) and its state (n_keep = 1).  Next to it, in the same process and on the same slab, alternating with it:
mi_mcmc_draw_stats asked for rhat alone (acov NULL), the classic diagnostic.  The time is also given as a multiple of ONE streaming read of the slab at
the achievable HBM rate (6.3 TB/s): the chain-moments kernel reads the slab twice, the sums and then the centred squares of the same tile, so close to
1 x means that the second pass came out of the caches and close to 2 x that it came from HBM.
    python tools/nested_rhat_time.py [--out profiles/nested_rhat_time.log]"""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd

HBM = 6.3e12
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "nested_rhat_time.log"))
ap.add_argument("--shapes", default="100x128x65536x64,1x128x65536x64")                   # n_keep x d x C x M
ap.add_argument("--runs", type=int, default=7)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("no GPU: nothing is measured (there is no CPU path)")
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)

say(f"device: {torch.cuda.get_device_name(0)}; library {os.path.basename(os.environ.get('MI_MCMC_LIB', mcmc_amd.LIB_PATH))}; one streaming read counted at {HBM / 1e12:.1f} TB/s; "
    f"per shape one warm-up call of each function discarded, then {args.runs} alternating runs, median and every run in ms")
stream = torch.cuda.current_stream().cuda_stream
lib = mcmc_amd.lib()
for shp in args.shapes.split(","):
    N, d, C, M = map(int, shp.split("x"))
    K = C // M
    g = torch.Generator(device="cuda"); g.manual_seed(d + C + N)
    slab = torch.randn((N, d, C), dtype=torch.float64, device="cuda", generator=g) + torch.linspace(-10, 10, d, dtype=torch.float64, device="cuda")[None, :, None]
    out = [torch.empty(d, dtype=torch.float64).pin_memory() for _ in range(5)] + [torch.empty((K, d), dtype=torch.float64).pin_memory()]
    rhat = torch.empty(d, dtype=torch.float64).pin_memory()
    def nested():
        rc = lib.mi_mcmc_draw_stats_nested(slab.data_ptr(), mcmc_amd.MEM_DEVICE, N, d, C, M, *[o.data_ptr() for o in out], stream)
        assert rc == 0, lib.mi_mcmc_last_error()
    def nested_nrhat_alone():
        rc = lib.mi_mcmc_draw_stats_nested(slab.data_ptr(), mcmc_amd.MEM_DEVICE, N, d, C, M, out[0].data_ptr(), None, None, None, None, None, stream)
        assert rc == 0, lib.mi_mcmc_last_error()
    def classic():
        rc = lib.mi_mcmc_draw_stats(slab.data_ptr(), mcmc_amd.MEM_DEVICE, N, d, C, None, None, rhat.data_ptr(), None, stream)
        assert rc == 0, lib.mi_mcmc_last_error()
    fns = [("draw_stats_nested, all six outputs", nested), ("draw_stats_nested, nrhat alone", nested_nrhat_alone)]
    if N >= 4:
        fns.append(("draw_stats, rhat alone (acov NULL)", classic))                      # the classic R-hat is not defined for the state
    for _, fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in fns}
    for _ in range(args.runs):
        for name, fn in fns:
            ts[name].append(timed(fn))
    t_read = 8.0 * N * d * C / HBM * 1e3
    say(f"n_keep={N} d={d} C={C} M={M} (K={K}), slab {8.0 * N * d * C / 2 ** 30:.3f} GiB, one streaming read {t_read:.3f} ms:")
    for name, _ in fns:
        med = float(np.median(ts[name]))
        say(f"    {name}: {med:.3f} ms = {med / t_read:.2f} x one read (min {min(ts[name]):.3f}, max {max(ts[name]):.3f}; runs: {' '.join(f'{t:.3f}' for t in ts[name])})")
    say(f"    nrhat {out[0].numpy().min():.5f} .. {out[0].numpy().max():.5f}" + (f"; classic rhat {rhat.numpy().min():.5f} .. {rhat.numpy().max():.5f}" if N >= 4 else ""))
    del slab
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
