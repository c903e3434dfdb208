"""mi_mcmc_draws_predict (mcmc_amd/csrc/draws_predict.hip, draws_api.hip) on the GPU box: time of the call with the slab, the target and the outputs in
device memory (HIP events around the call on its stream, one warm-up discarded, then the median of 5 with min .. max), and in the same session on the
same slab the two merged reducers whose loops its two kernels are:
    mi_mcmc_draws_waic (lppd and p_waic, no matrix, no summary)  -- the template of predict_rows_kernel
    mi_mcmc_draws_log_kernel                                      -- the template of predict_cols_kernel
The call is timed with the per-row outputs alone (the row kernel), the per-draw outputs alone (the column kernel), both, both with the matrices prob and
yrep stored, and both with the summary (the counting kernel and the host's share; that call blocks).
    python tools/predict_time.py [--out profiles/predict_time.log] [--shapes 1024x1x65536x1024,128x8x65536x1024]        (d x n_keep x C x n_rows)"""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "predict_time.log"))
ap.add_argument("--shapes", default="1024x1x65536x1024,128x8x65536x1024")
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

def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"

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
    f = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
    rows = dict(p_mean=f(n_rows), p_var=f(n_rows), rep_freq=f(n_rows))
    cols = dict(t_rep=f(n_keep, C), ll_rep=f(n_keep, C), ll_obs=f(n_keep, C))
    mats = dict(prob=f(n_rows, n_keep, C), yrep=f(n_rows, n_keep, C))
    lppd, pw, lk = f(n_rows), f(n_rows), f(n_keep, C)
    common = dict(seed=1, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream)
    say(f"logistic d={d} n_rows={n_rows} n_keep={n_keep} C={C}: K = {K}, slab {8.0 * d * K / 1e9:.3f} GB, product {2.0 * n_rows * d * K / 1e12:.3f} TFLOP, "
        f"{n_rows * K / 1e6:.1f} M elements; prob + yrep {16.0 * n_rows * K / 1e9:.2f} GB")
    t_waic = timed(lambda: mcmc_amd.draws_waic(tgt, slab, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_summary=False, lppd=lppd, p_waic=pw))
    t_logk = timed(lambda: mcmc_amd.draws_log_kernel(tgt, slab, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, out=lk))
    t_rows = timed(lambda: mcmc_amd.draws_predict(tgt, slab, want_summary=False, **common, **rows))
    k_rows = mcmc_amd.last_kernel()
    t_cols = timed(lambda: mcmc_amd.draws_predict(tgt, slab, want_summary=False, **common, **cols))
    k_cols = mcmc_amd.last_kernel()
    t_both = timed(lambda: mcmc_amd.draws_predict(tgt, slab, want_summary=False, **common, **rows, **cols))
    t_mats = timed(lambda: mcmc_amd.draws_predict(tgt, slab, want_summary=False, **common, **rows, **cols, **mats))
    res = {}
    t_summ = timed(lambda: res.update(mcmc_amd.draws_predict(tgt, slab, want_summary=True, **common, **rows, **cols)))
    say(f"  templates: draws_waic {fmt(t_waic)}; draws_log_kernel {fmt(t_logk)}")
    say(f"  draws_predict, per-row outputs alone ({k_rows}): {fmt(t_rows)} = {t_rows[0] / t_waic[0]:.2f} x draws_waic")
    say(f"  draws_predict, per-draw outputs alone ({k_cols}): {fmt(t_cols)} = {t_cols[0] / t_logk[0]:.2f} x draws_log_kernel")
    say(f"  draws_predict, both: {fmt(t_both)} = {t_both[0] / (t_rows[0] + t_cols[0]):.2f} x the sum of the two ({t_rows[0] + t_cols[0]:.3f} ms)")
    say(f"  draws_predict, both and the matrices prob and yrep stored: {fmt(t_mats)} = {t_mats[0] / t_both[0]:.2f} x without them")
    say(f"  draws_predict, both and the summary (blocking): {fmt(t_summ)}; summary {res['summary']}")
    del slab, mats, rows, cols
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    fo.write("\n".join(lines) + "\n")
