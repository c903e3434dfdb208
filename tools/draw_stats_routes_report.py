"""For the chains-that-disagree and the large-offset inputs of tests/test_gpu_draw_stats.py: each route's worst |got - ref| / bound against the exact reference of
tests/draw_stats_ref.py (GPU box).  No assertion and no route probe, so it also runs on the library of an older commit that MI_MCMC_LIB names -- which is how
profiles/draw_stats_bounds.log shows what the tests see on the kernels before the variance fix.    python tools/draw_stats_routes_report.py"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import draw_stats_ref as R
import mcmc_amd
print("library:", "the one MI_MCMC_LIB names" if os.environ.get("MI_MCMC_LIB") else "in-tree", flush=True)
def report(name, want_acov, label):
    ref = R.reference(name)
    s = mcmc_amd.draw_stats(R.slab(name), want_acov=want_acov)
    w = dict(mean=R.worst(s["mean"], ref["mean"], ref["mean_bound"]), rhat=R.worst(s["rhat"], ref["rhat"], ref["rhat_bound"]), ess=R.worst(s["ess"], ref["ess"], ref["ess_bound"]))
    if want_acov:
        w["acov"] = R.worst(s["acov"][:ref["nlag"]], ref["acov"], ref["acov_bound"])
    rel = np.abs((s["rhat"].astype(R.LD) / ref["rhat"] - 1).astype(np.float64)).max()
    verdict = "inside" if all(v <= 1 for v in w.values()) else "OUTSIDE"
    print(f"{name:22s} {label:28s} " + " ".join(f"{k} {v:10.4g}" for k, v in w.items()) + f"  | rel. error of R-hat {rel:.2e}  -> {verdict}", flush=True)
for delta in R.DELTAS:
    report(R.DISAGREE[(delta, 100)], True, "Gram (n=100)")
    report(R.DISAGREE[(delta, 150)], False, "window (n=150, no acov)")
    report(R.DISAGREE[(delta, 150)], True, "lag blocks (n=150, acov)")
    report(R.DISAGREE[(delta, 300)], True, "streamed (n=300)")
report(R.CENTRING[100], True, "Gram (n=100)")
report(R.CENTRING[150], False, "window (n=150, no acov)")
report(R.CENTRING[150], True, "lag blocks (n=150, acov)")
report(R.CENTRING[300], True, "streamed (n=300)")
