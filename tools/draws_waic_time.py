"""mi_mcmc_draws_waic (mcmc_amd/csrc/draws_waic.hip) on the GPU box: time per call with the slab, the target and the outputs in device memory and
summary = NULL (HIP events around the call on its stream -- it only enqueues --, one warm-up discarded, then the median of 5 with min .. max), without
and with loglik_out, next to mi_mcmc_draws_log_kernel on the same slab in the same process.  The call is the pack of X, the shift kernel, the fused
product kernel and the merge.  The flop model is the product's, 2 n_rows d K (the row terms and the folds are not counted), its rate a fraction of the
fp64 matrix peak of 78.6 TFLOP/s.  A torch.float64 evaluation of lppd and p_waic is printed as a sanity figure (largest relative difference), not a
pass criterion: the bits are the GPU tests' business.
    python tools/draws_waic_time.py [--out profiles/draws_waic_time.log]"""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth

PEAK = 78.6e12
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "draws_waic_time.log"))
ap.add_argument("--shapes", default="1024x1x65536x4096,1024x16x65536x4096")      # d x n_keep x C x n_rows
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

say(f"device: {torch.cuda.get_device_name(0)}; fp64 matrix peak used {PEAK / 1e12:.1f} TFLOP/s")
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
    flops = 2.0 * n_rows * d * K
    plan = mcmc_amd.test_waic_plan(tgt.kind, d, n_rows, n_keep, C, slab_host=False, target_host=False)
    say(f"logistic d={d} n_rows={n_rows} n_keep={n_keep} C={C} (K={K}, slab {8.0 * d * K / 1e9:.3f} GB, ll {8.0 * n_rows * K / 1e9:.3f} GB, {flops / 1e12:.3f} TFLOP; "
        f"{plan['grid']} workgroups of {plan['block']}, {plan['n_chunks']} chunks, workspace {plan['ws_bytes'] / 1e6:.1f} MB)")
    lppd = torch.empty(n_rows, dtype=torch.float64, device="cuda")
    pw = torch.empty(n_rows, dtype=torch.float64, device="cuda")
    lp = torch.empty((n_keep, C), dtype=torch.float64, device="cuda")
    def logk():
        mcmc_amd.draws_log_kernel(tgt, slab, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, out=lp)
    def waic_call(ll=None):
        mcmc_amd.draws_waic(tgt, slab, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_summary=False, lppd=lppd, p_waic=pw, loglik=ll)
    base, blo, bhi = timed(logk)
    say(f"  draws_log_kernel:              {base:9.3f} ms ({blo:.3f} .. {bhi:.3f}); {flops / (base * 1e-3) / PEAK:.3f} of the matrix peak")
    ms, lo, hi = timed(waic_call)
    say(f"  draws_waic, loglik_out NULL:   {ms:9.3f} ms ({lo:.3f} .. {hi:.3f}); {flops / (ms * 1e-3) / PEAK:.3f} of the matrix peak; {ms / base:.2f} x draws_log_kernel")
    ll = torch.empty((n_rows, n_keep, C), dtype=torch.float64, device="cuda")
    ms2, lo2, hi2 = timed(lambda: waic_call(ll))
    say(f"  draws_waic, loglik_out set:    {ms2:9.3f} ms ({lo2:.3f} .. {hi2:.3f}); {flops / (ms2 * 1e-3) / PEAK:.3f} of the matrix peak; {ms2 / base:.2f} x draws_log_kernel; "
        f"the stores alone at that time = {8.0 * n_rows * K / (ms2 * 1e-3) / 1e12:.3f} TB/s")
    rows = slice(0, min(n_rows, 256))                     # the sanity figure: the first rows, from the stored matrix and from torch's own
    eta = X[rows] @ slab[0]
    ref = y[rows, None] * eta - torch.nn.functional.softplus(eta)
    rel_ll = ((ll[rows, 0] - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
    flat = ll[rows].reshape(rows.stop, K)
    ref_lppd = torch.logsumexp(flat, 1) - float(np.log(K))
    ref_pw = flat.var(1, unbiased=True)
    say(f"    largest relative difference to torch.float64 over the first {rows.stop} rows: ll {rel_ll:.2e}, lppd {((lppd[rows] - ref_lppd).abs() / ref_lppd.abs()).max().item():.2e}, "
        f"p_waic {((pw[rows] - ref_pw).abs() / ref_pw).max().item():.2e}")
    del slab, ll, lp, eta, ref, flat
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
