"""mi_mcmc_draws_bridge (mcmc_amd/csrc/draws_bridge.hip, draws_api.hip) on the GPU box: time of the whole call with the slab and the target in device memory
(HIP events around the call on its stream -- it always blocks --, one warm-up discarded, then the median of 5 with min .. max), and in the same session on
the same slab the call with a fit not seen before (the factorisations of d >= 64 are memoised: the plain figure is of a repeated fit) and what the call is
made of that existed before it:
    mi_mcmc_draws_covariance of the fit half;  mi_mcmc_draws_log_kernel of the iteration half, twice (the second stands for the N2 = N1 proposal columns).
What is new on top of those parts: the proposal product (2 d^2 N2 flops, d N2 doubles written), the two logg products (2 d^2 (N1 + N2) flops, the iteration
half and the proposal block read once more), the factorisations, and the iteration (two launches of N1 + N2 values and one copy of the pieces per step).
The iteration's share is timed by mi_mcmc_bridge_estimate on four device arrays of the same sizes taken from bridge_proposal and draws_log_kernel.
    python tools/bridge_time.py [--out profiles/bridge_time.log] [--shapes dense:128x100x65536,logistic:1024x2x32768x1024] [--once]
--once: one call per shape and nothing else (what a rocprofv3 --kernel-trace --stats run of its own wraps)."""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch, mcmc_amd
from mcmc_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bridge_time.log"))
ap.add_argument("--shapes", default="dense:128x100x65536,logistic:1024x2x32768x1024")      # kind:d x n_keep x C [x n_rows]
ap.add_argument("--once", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("no GPU: nothing is measured (there is no CPU path)")
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

def timed(fn, n=5, before=None):
    fn(); torch.cuda.synchronize()                       # warm-up, discarded
    ts = []
    for _ in range(n):
        if before is not None:
            before(); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), min(ts), max(ts)

say(f"device: {torch.cuda.get_device_name(0)}")
stream = torch.cuda.current_stream().cuda_stream
for spec in args.shapes.split(","):
    kind, shp = spec.split(":")
    dims = list(map(int, shp.split("x")))
    d, n_keep, C = dims[:3]
    n_fit = n_keep // 2
    n_it = n_keep - n_fit
    N1 = n_it * C
    g = torch.Generator(device="cuda"); g.manual_seed(d + C)
    slab = torch.randn((n_keep, d, C), dtype=torch.float64, device="cuda", generator=g)
    if kind == "dense":
        Ph = synth.dense_gaussian_precision(d)
        Lc = torch.from_numpy(np.linalg.cholesky(np.linalg.inv(Ph))).cuda()
        for t in range(n_keep):                           # exact draws of the target, a row at a time (no second slab)
            slab[t] = Lc @ slab[t]
        P = torch.from_numpy(Ph).cuda()
        tgt = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=P, mem=mcmc_amd.MEM_DEVICE)
        truth = 0.5 * d * 1.83787706640934548356 - 0.5 * np.linalg.slogdet(Ph)[1]
        what = f"dense d={d}"
    else:
        n_rows = dims[3]
        Xh, yh = synth.logistic_problem(d, n_rows)
        X, y = torch.from_numpy(Xh).cuda(), torch.from_numpy(yh).cuda()
        tgt = mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, d, X=X, y=y, mem=mcmc_amd.MEM_DEVICE)
        tgt.n_rows = n_rows
        # draws of the Laplace approximation at the mode (Newton steps in torch.float64): close enough to the posterior for the iteration to be typical
        th = torch.zeros(d, dtype=torch.float64, device="cuda")
        for _ in range(25):
            p = torch.sigmoid(X @ th)
            H = X.T @ (X * (p * (1 - p))[:, None]) + torch.eye(d, dtype=torch.float64, device="cuda")
            th = th - torch.linalg.solve(H, X.T @ (p - y) + th)
        Lc = torch.linalg.cholesky(torch.linalg.inv(H))
        for t in range(n_keep):
            slab[t] = th[:, None] + Lc @ slab[t]
        truth = None
        what = f"logistic d={d} n_rows={n_rows}"
    f2 = torch.empty((n_it, C), dtype=torch.float64, device="cuda")
    res = {}
    def call():
        res.update(mcmc_amd.draws_bridge(tgt, slab, seed=1, n_keep=n_keep, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_mean=False, want_cov=False, f2=f2))
    if args.once:
        call(); torch.cuda.synchronize()
        say(f"{what}: one call, summary {res['summary']}")
        continue
    say(f"{what} n_keep={n_keep} C={C}: n_fit={n_fit}, N1 = N2 = {N1}, slab {8.0 * d * n_keep * C / 1e9:.3f} GB; new products {3 * 2.0 * d * d * N1 / 1e12:.3f} TFLOP")
    ms, lo, hi = timed(call)
    s = res["summary"]
    say(f"  draws_bridge: {ms:.2f} ms ({lo:.2f} .. {hi:.2f}); logml {s['logml']:.6f}" + (f" (analytic {truth:.6f})" if truth is not None else "")
        + f", status {int(s['status'])}, {int(s['it'])} iterations, rel {s['rel']:.2e}, cv1 {s['cv1']:.3e}, cv2 {s['cv2']:.3e}; kernels: {mcmc_amd.last_kernel()}")
    c_ms, c_lo, c_hi = timed(lambda: mcmc_amd.draws_covariance(slab, n_keep=n_fit, d=d, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream))
    lp1 = torch.empty((n_it, C), dtype=torch.float64, device="cuda")
    tail = slab[n_fit:]
    def logk():
        mcmc_amd.draws_log_kernel(tgt, tail, n_keep=n_it, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, out=lp1)
        mcmc_amd.draws_log_kernel(tgt, tail, n_keep=n_it, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, out=lp1)
    k_ms, k_lo, k_hi = timed(logk)
    say(f"  parts that existed: draws_covariance of the fit half {c_ms:.2f} ms ({c_lo:.2f} .. {c_hi:.2f}); draws_log_kernel of two N1-column slabs {k_ms:.2f} ms ({k_lo:.2f} .. {k_hi:.2f});"
        f" sum {c_ms + k_ms:.2f} ms; the call is {ms / (c_ms + k_ms):.2f} x that")
    # the pieces of the call on their own: the proposal without prop_out (groups), and the estimate on device arrays
    lg1 = torch.empty((n_it, C), dtype=torch.float64, device="cuda")
    lg2 = torch.empty((N1,), dtype=torch.float64, device="cuda")
    p_ms, p_lo, p_hi = timed(lambda: mcmc_amd.bridge_proposal(slab, seed=1, n_keep=n_keep, d=d, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_mean=False,
                                                              want_cov=False, logg_post=lg1, logg_prop=lg2))
    q_ms, _, _ = timed(lambda: mcmc_amd.bridge_proposal(slab, seed=1, n_keep=n_keep, d=d, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, want_mean=True, want_cov=False))
    prop = torch.empty((1, d, N1), dtype=torch.float64, device="cuda")
    mcmc_amd.bridge_proposal(slab, seed=1, n_keep=n_keep, d=d, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, prop=prop)
    lp2 = torch.empty((1, N1), dtype=torch.float64, device="cuda")
    mcmc_amd.draws_log_kernel(tgt, prop, n_keep=1, n_chains=N1, mem=mcmc_amd.MEM_DEVICE, stream=stream, out=lp2)
    mcmc_amd.draws_log_kernel(tgt, tail, n_keep=n_it, n_chains=C, mem=mcmc_amd.MEM_DEVICE, stream=stream, out=lp1)
    torch.cuda.synchronize()
    est = {}
    e_ms, e_lo, e_hi = timed(lambda: est.update(mcmc_amd.bridge_estimate(lp1, lg1, lp2, lg2, n_it=n_it, n_chains=C, n_prop=N1, mem=mcmc_amd.MEM_DEVICE, stream=stream, f2=f2)))
    say(f"  pieces: bridge_proposal (fit, factorisations, proposal and both logg, in groups) {p_ms:.2f} ms ({p_lo:.2f} .. {p_hi:.2f}), of which the fit and the factorisations alone {q_ms:.2f} ms;"
        f" bridge_estimate {e_ms:.2f} ms ({e_lo:.2f} .. {e_hi:.2f}) for {int(est['summary']['it'])} iterations = {e_ms / ms:.2f} of the call"
        f" (same logml: {est['summary']['logml'] == s['logml']})")
    # ... and with a fit nobody has seen: INV and CHOL_LOWER of d >= 64 are memoised per thread, and the calls above fit the same S every time.  Last, because it changes the slab.  One sample of
    # the fit part is scaled before every call, so S differs in its bits and both factorisations are computed: what a caller with new draws pays
    def new_fit():
        slab[0, :, 0] *= 1.0 + 2.0 ** -20
    f_ms, f_lo, f_hi = timed(call, before=new_fit)
    say(f"  draws_bridge with a fit not seen before (both factorisations computed): {f_ms:.2f} ms ({f_lo:.2f} .. {f_hi:.2f}) = {f_ms / (c_ms + k_ms):.2f} x the parts")
    del slab, f2, lp1, lp2, lg1, lg2, prop
    torch.cuda.empty_cache()
if not args.once:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
