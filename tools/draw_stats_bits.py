"""A SHA-256 of every output of draw_stats, draw_stats_lags, draw_stats_ranked and draw_stats_ranked_lags on the inputs of tests/draw_stats_ref.py and
tests/draw_stats_lags_ref.py, one line per call (GPU box).  No assertion and no probe, so it also runs on the library of another commit that
MI_MCMC_LIB names: two runs, one per library and each in a fresh process, whose outputs are the same in every line computed the same bits.
    python tools/draw_stats_bits.py > this.txt;  MI_MCMC_LIB=/path/to/other/libmi_mcmc.so python tools/draw_stats_bits.py > other.txt"""
import hashlib, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import draw_stats_ref as R
import draw_stats_lags_ref as LR
import mcmc_amd


def say(call, res):
    digests = " ".join(f"{k} {hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16]}" for k, v in res.items() if v is not None)
    print(f"{call:64s} {digests}", flush=True)


for name in R.SPECS:
    for acov in (True, False):
        say(f"draw_stats {name} want_acov={acov}", mcmc_amd.draw_stats(R.slab(name), want_acov=acov))
lag_inputs = {name: LR.slab(name) for name in LR.INPUTS}
lag_inputs["TILING"] = LR.slab_of(*LR.TILING)
for name, x in lag_inputs.items():
    for acov in (True, False):
        for K in (None, 127, 16, 0):
            say(f"draw_stats_lags {name} want_acov={acov} max_lag={K}", mcmc_amd.draw_stats_lags(x, K, want_acov=acov))
for name in ("L1", "L2"):
    say(f"draw_stats_ranked {name}", mcmc_amd.draw_stats_ranked(lag_inputs[name]))
    for K in (None, 127):
        say(f"draw_stats_ranked_lags {name} max_lag={K}", mcmc_amd.draw_stats_ranked_lags(lag_inputs[name], K))

# a device-resident slab on a side stream, one call each
import torch
side = torch.cuda.Stream()
x = torch.from_numpy(np.array(lag_inputs["L2"])).cuda()
n, d, C = x.shape
torch.cuda.synchronize()
dev = dict(mem=mcmc_amd.MEM_DEVICE, stream=side.cuda_stream)
say("draw_stats L2 device slab, side stream", mcmc_amd.draw_stats(x, n, d, C, **dev))
say("draw_stats_lags L2 device slab, side stream", mcmc_amd.draw_stats_lags(x, None, n, d, C, **dev))
say("draw_stats_ranked L2 device slab, side stream", mcmc_amd.draw_stats_ranked(x, n, d, C, **dev))
say("draw_stats_ranked_lags L2 device slab, side stream", mcmc_amd.draw_stats_ranked_lags(x, None, n, d, C, **dev))
