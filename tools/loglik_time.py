"""mi_mcmc_loglik_waic and mi_mcmc_loglik_psis_loo (mcmc_amd/csrc/draws_loglik.hip in front of draws_rank.hip and draws_psis.hip) on the GPU box: time per
call on a caller-supplied matrix of n_rows x K doubles in device memory, in both layouts, with the outputs in device memory and summary = NULL (HIP
events around the call on its stream, one warm-up discarded, then the median of 5 with min .. max).  The WAIC call is the fold kernel and the merge; the
PSIS call adds, per sort group, the radix sort of every row where it lies and the two PSIS kernels.  For comparison, in the same process:
mi_mcmc_draws_waic with loglik_out set and mi_mcmc_draws_psis_loo on the LOGISTIC slab of DESIGN.md 4.27 (d = 1 024), which form a matrix of the same
size from a built-in target.
    python tools/loglik_time.py [--out profiles/loglik_time.log]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/loglik_time.py --trace      (one warm-up and one call of each, no log)"""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "loglik_time.log"))
ap.add_argument("--shape", default="4096x1x65536x1024")       # n_rows x n_keep x C x d of the comparison slab
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
n_rows, n_keep, C, d = map(int, args.shape.split("x"))
K = n_keep * C
gb = 8.0 * n_rows * K / 1e9
new = lambda: torch.empty(n_rows, dtype=torch.float64, device="cuda")
elpd, pk, lppd, pw = new(), new(), new(), new()

# the comparison: the built-in LOGISTIC target forms the matrix (and leaves it in ll, in MI_LOGLIK_ROWS)
g = torch.Generator(device="cuda"); g.manual_seed(d + C)
slab = torch.randn((n_keep, d, C), dtype=torch.float64, device="cuda", generator=g)
Xh, yh = synth.logistic_problem(d, n_rows)
X, y = torch.from_numpy(Xh).cuda(), torch.from_numpy(yh).cuda()
tgt = mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, d, X=X, y=y, mem=mcmc_amd.MEM_DEVICE)
tgt.n_rows = n_rows
ll = torch.empty((n_rows, n_keep, C), dtype=torch.float64, device="cuda")
def draws_waic_call():
    mcmc_amd.draws_waic(tgt, slab, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_summary=False, lppd=lppd, p_waic=pw, loglik=ll)
def draws_psis_call():
    mcmc_amd.draws_psis_loo(tgt, slab, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_summary=False, elpd_loo=elpd, pareto_k=pk, lppd=lppd)
def loglik_calls(mat, layout):
    kw = dict(n_rows=n_rows, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_summary=False)
    return (lambda: mcmc_amd.loglik_waic(mat, layout, lppd=lppd, p_waic=pw, **kw),
            lambda: mcmc_amd.loglik_psis_loo(mat, layout, elpd_loo=elpd, pareto_k=pk, lppd=lppd, **kw))

say(f"matrix: n_rows={n_rows} n_keep={n_keep} C={C} (K={K}, {gb:.3f} GB); comparison: LOGISTIC d={d}, slab {8.0 * d * K / 1e9:.3f} GB")
if args.trace:
    for fn in (draws_waic_call, draws_psis_call) + loglik_calls(ll, mcmc_amd.LOGLIK_ROWS):
        fn(); torch.cuda.synchronize(); fn(); torch.cuda.synchronize()
    sys.exit(0)
base_w, lo, hi = timed(draws_waic_call)
say(f"  draws_waic, loglik_out set:      {base_w:9.3f} ms ({lo:.3f} .. {hi:.3f})")
base_p, lo, hi = timed(draws_psis_call)
say(f"  draws_psis_loo:                  {base_p:9.3f} ms ({lo:.3f} .. {hi:.3f})")
ref = dict(lppd=lppd.clone(), elpd=elpd.clone(), pk=pk.clone())
del slab
torch.cuda.empty_cache()
same = lambda a, b: bool(torch.equal(a.view(torch.int64), b.view(torch.int64)) or torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)))
for layout, name in ((mcmc_amd.LOGLIK_ROWS, "MI_LOGLIK_ROWS"), (mcmc_amd.LOGLIK_SLAB, "MI_LOGLIK_SLAB")):
    mat = ll if layout == mcmc_amd.LOGLIK_ROWS else ll.permute(1, 0, 2).contiguous()      # the same matrix, as a slab [n_keep][n_rows][C]
    plan = mcmc_amd.test_loglik_plan(layout, n_rows, n_keep, C, mat_host=False, psis=True)
    say(f"  {name}: {plan['n_chunks']} chunks, fold grid {plan['fold_grid']}, M={plan['M']}, m={plan['m']}, sorted {plan['sort_rows']} rows at a time in {plan['sort_groups']} "
        f"group(s), tail route {plan['tail_route']}, workspace {plan['ws_bytes'] / 1e9:.3f} GB")
    waic_call, psis_call = loglik_calls(mat, layout)
    ms, lo, hi = timed(waic_call)
    say(f"    loglik_waic:                   {ms:9.3f} ms ({lo:.3f} .. {hi:.3f}); {ms / base_w:.3f} x draws_waic; {gb / ms:.3f} TB/s of ll folded (fold and merge)")
    ms, lo, hi = timed(psis_call)
    say(f"    loglik_psis_loo:               {ms:9.3f} ms ({lo:.3f} .. {hi:.3f}); {ms / base_p:.3f} x draws_psis_loo; {gb / ms:.3f} TB/s of ll sorted and folded")
    say(f"    the bits of the draws_* entries on this matrix: lppd {same(lppd, ref['lppd'])}, elpd_loo {same(elpd, ref['elpd'])}, pareto_k {same(pk, ref['pk'])}")
    if mat is not ll:
        del mat
        torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
