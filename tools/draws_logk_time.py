"""mi_mcmc_draws_log_kernel (mcmc_amd/csrc/draws_logk.hip) on the GPU box: time per call with the slab, the target and the result in device memory (HIP
events around the call on its stream -- it only enqueues --, one warm-up discarded, then the median of 5 with min .. max).  The call is the pack of the
matrix plus the fused product kernel.  Next to it the flop model
    DENSE 2 d^2 K, LOGISTIC 2 n_rows d K          (the products; the folds and the row terms are not counted)
its rate as a fraction of the fp64 matrix peak of 78.6 TFLOP/s, and one read of the slab (8 d K bytes) at that time.  The yardstick of the d = 1024 dense
shape is the product of the same size in the samplers, gemm_step_kernel<2, 0>: 2.09 ms per launch in profiles/r6_gemm_kernel_stats.csv, 0.838 of that peak;
this reducer does the same flops and writes 1 / d of the output.  A torch.float64 evaluation of the same quantity is printed as a sanity figure (largest
relative difference), not a pass criterion: the bits are the GPU tests' business.
    python tools/draws_logk_time.py [--out profiles/draws_logk_time.log]"""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth

PEAK = 78.6e12
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "draws_logk_time.log"))
ap.add_argument("--shapes", default="dense:128x100x65536,dense:1024x1x65536,logistic:512x1x32768x1024")      # kind:d x n_keep x C [x n_rows]
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

say(f"device: {torch.cuda.get_device_name(0)}; fp64 matrix peak used {PEAK / 1e12:.1f} TFLOP/s; yardstick gemm_step_kernel<2, 0> at d = 1024 x 65 536 columns: 2.09 ms, 0.838 of peak")
stream = torch.cuda.current_stream().cuda_stream
for spec in args.shapes.split(","):
    kind, shp = spec.split(":")
    dims = list(map(int, shp.split("x")))
    d, n_keep, C = dims[:3]
    K = n_keep * C
    g = torch.Generator(device="cuda"); g.manual_seed(d + C)
    slab = torch.randn((n_keep, d, C), dtype=torch.float64, device="cuda", generator=g)
    out = torch.empty((n_keep, C), dtype=torch.float64, device="cuda")
    if kind == "dense":
        P = torch.from_numpy(synth.dense_gaussian_precision(d)).cuda()
        tgt = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=P, mem=mcmc_amd.MEM_DEVICE)
        flops, what = 2.0 * d * d * K, f"dense d={d}"
    else:
        n_rows = dims[3]
        Xh, yh = synth.logistic_problem(d, n_rows)
        X, y = torch.from_numpy(Xh).cuda(), torch.from_numpy(yh).cuda()
        tgt = mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, d, X=X, y=y, mem=mcmc_amd.MEM_DEVICE)
        flops, what = 2.0 * n_rows * d * K, f"logistic d={d} n_rows={n_rows}"
    plan = mcmc_amd.test_logk_plan(tgt.kind, d, int(tgt.n_rows), n_keep, C, slab_host=False, target_host=False)
    say(f"{what} n_keep={n_keep} C={C} (K={K}, slab {8.0 * d * K / 1e9:.3f} GB, {flops / 1e12:.3f} TFLOP; {plan['grid']} workgroups x {plan['n_row_tiles']} row tiles x {plan['Kp'] // 16} steps)")
    def call():
        mcmc_amd.draws_log_kernel(tgt, slab, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, out=out)
    ms, lo, hi = timed(call)
    rate = flops / (ms * 1e-3)
    say(f"  draws_log_kernel: {ms:.3f} ms ({lo:.3f} .. {hi:.3f}); {rate / 1e12:.2f} TFLOP/s = {rate / PEAK:.3f} of the matrix peak; one read of the slab in that time = {8.0 * d * K / (ms * 1e-3) / 1e12:.3f} TB/s")
    t0 = min(n_keep - 1, 1)
    x0 = slab[t0]                                         # [d][C]: one kept draw, the sanity figure
    if kind == "dense":
        ref = -0.5 * (x0 * (P @ x0)).sum(0)
    else:
        eta = X @ x0
        ref = (y[:, None] * eta - torch.nn.functional.softplus(eta)).sum(0) - 0.5 * (x0 * x0).sum(0)
    rel = ((out[t0] - ref).abs() / ref.abs()).max().item()
    say(f"    largest relative difference to a torch.float64 evaluation of draw {t0}: {rel:.2e}")
    del slab, out
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
