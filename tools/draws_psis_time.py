"""mi_mcmc_draws_psis_loo (mcmc_amd/csrc/draws_psis.hip behind draws_waic.hip and draws_rank.hip) on the GPU box: time per call with the slab, the target
and the outputs in device memory and summary = NULL (HIP events around the call on its stream -- the call is blocking, the events bracket what it
enqueued and waited for --, one warm-up discarded, then the median of 5 with min .. max), next to mi_mcmc_draws_waic with loglik_out set on the same
slab in the same process: the product that both run.  The call is, per row group, the WAIC kernels with the block ll as their loglik, per sort group
the radix sort of every row of the block (keys, digit counts, scan and scatter per executed pass) and the two PSIS kernels.  A numpy evaluation of
mcmc_amd.psis on the first rows of the stored matrix is printed as a sanity figure (largest difference), not a pass criterion: the bits are the GPU
tests' business.
    python tools/draws_psis_time.py [--out profiles/draws_psis_time.log]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/draws_psis_time.py --trace      (one warm-up and one call, no log)"""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import psis, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "draws_psis_time.log"))
ap.add_argument("--shapes", default="1024x1x65536x4096")      # d x n_keep x C x n_rows
ap.add_argument("--trace", action="store_true", help="one warm-up and one call of each entry, nothing else: the run rocprofv3 wraps")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("no GPU: nothing is measured (there is no CPU path)")
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

def timed(fn, n=5):
    fn(); torch.cuda.synchronize()                       # warm-up, discarded
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), min(ts), max(ts)

say(f"device: {torch.cuda.get_device_name(0)}")
stream = torch.cuda.current_stream().cuda_stream
for spec in args.shapes.split(","):
    d, n_keep, C, n_rows = map(int, spec.split("x"))
    K = n_keep * C
    g = torch.Generator(device="cuda"); g.manual_seed(d + C)
    slab = torch.randn((n_keep, d, C), dtype=torch.float64, device="cuda", generator=g)
    Xh, yh = synth.logistic_problem(d, n_rows)
    X, y = torch.from_numpy(Xh).cuda(), torch.from_numpy(yh).cuda()
    tgt = mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, d, X=X, y=y, mem=mcmc_amd.MEM_DEVICE)
    tgt.n_rows = n_rows
    plan = mcmc_amd.test_psis_plan(tgt.kind, d, n_rows, n_keep, C, slab_host=False, target_host=False)
    say(f"logistic d={d} n_rows={n_rows} n_keep={n_keep} C={C} (K={K}, slab {8.0 * d * K / 1e9:.3f} GB, ll {8.0 * n_rows * K / 1e9:.3f} GB; M={plan['M']}, m={plan['m']}, "
        f"{plan['n_groups']} row group(s) of {plan['G']}, sorted {plan['sort_rows']} rows at a time, tail route {plan['tail_route']}, {plan['n_pieces']} body pieces per row, "
        f"workspace {plan['ws_bytes'] / 1e9:.3f} GB)")
    elpd = torch.empty(n_rows, dtype=torch.float64, device="cuda")
    pk = torch.empty(n_rows, dtype=torch.float64, device="cuda")
    lppd = torch.empty(n_rows, dtype=torch.float64, device="cuda")
    pw = torch.empty(n_rows, dtype=torch.float64, device="cuda")
    ll = torch.empty((n_rows, n_keep, C), dtype=torch.float64, device="cuda")
    def waic_call():
        mcmc_amd.draws_waic(tgt, slab, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_summary=False, lppd=lppd, p_waic=pw, loglik=ll)
    def psis_call():
        mcmc_amd.draws_psis_loo(tgt, slab, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_summary=False, elpd_loo=elpd, pareto_k=pk, lppd=lppd)
    if args.trace:
        for fn in (waic_call, psis_call):
            fn(); torch.cuda.synchronize(); fn(); torch.cuda.synchronize()
        continue
    base, blo, bhi = timed(waic_call)
    say(f"  draws_waic, loglik_out set:    {base:9.3f} ms ({blo:.3f} .. {bhi:.3f})")
    ms, lo, hi = timed(psis_call)
    say(f"  draws_psis_loo:                {ms:9.3f} ms ({lo:.3f} .. {hi:.3f}); {ms / base:.2f} x draws_waic; {8.0 * n_rows * K / (ms * 1e-3) / 1e12:.3f} TB/s of ll sorted and folded")
    kk = pk.cpu().numpy()
    say(f"    pareto_k: min {np.nanmin(kk):.3f}, median {np.nanmedian(kk):.3f}, max {np.nanmax(kk):.3f}; rows with k > 0.7, inf or NaN: {int(np.count_nonzero(~(kk <= 0.7)))} of {n_rows}")
    rows = min(n_rows, 8)                                 # the sanity figure: the first rows, numpy's own exp / log over the stored matrix
    ref_e, ref_k = psis.psis_rows(ll[:rows].reshape(rows, K).cpu().numpy())
    say(f"    largest difference to mcmc_amd.psis over numpy's libm on the first {rows} rows of the stored ll: elpd_loo {np.abs(elpd[:rows].cpu().numpy() - ref_e).max():.2e} absolute, "
        f"pareto_k {np.abs(kk[:rows] - ref_k).max():.2e} absolute")
    del slab, ll
    torch.cuda.empty_cache()
if not args.trace:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
