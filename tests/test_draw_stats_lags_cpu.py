"""No GPU: the host side of mi_mcmc_draw_stats_lags / mi_mcmc_draw_stats_ranked_lags -- the numpy statement mcmc_amd/acov.py against the exact reference
tests/draw_stats_lags_ref.py inside its bounds, against ess_per_chain (FFT against direct sums), the margin of every input the GPU tests use, the band
schedule, the argument checks of the C ABI (returned before any HIP call) and the symbols."""

import numpy as np
import pytest

import draw_stats_lags_ref as LR
import draw_stats_ref as R
import mcmc_amd
from mcmc_amd import acov as A
from mcmc_amd.ess import ess_per_chain

WINDOWS = (None, 127, 255)


@pytest.mark.parametrize("name", sorted(LR.INPUTS))
def test_numpy_statement_is_inside_the_bounds_of_the_exact_reference(name):
    x = LR.slab(name)
    for K in WINDOWS:
        ref = LR.reference_lags(x, K)
        s = A.draw_stats_lags_ref(x, K)
        s["acov"] = np.ascontiguousarray(s["acov"])
        LR.inside(f"{name} (numpy)", s, ref)
        e, en = A.ess_lags_ref(x, K)
        assert np.array_equal(e, s["ess"]) and np.array_equal(en, s["ended"]) and np.array_equal(A.acov_ref(x, K), s["acov"])


@pytest.mark.parametrize("name", sorted(LR.INPUTS))
def test_every_lag_is_ess_per_chain(name):
    x = LR.slab(name)
    e, en = A.ess_lags_ref(x, None)
    assert np.allclose(e, ess_per_chain(x), rtol=1e-8, atol=0.0) and en.all()


def test_the_issue_table():
    """all-lag ESS and the first lag of the stopping pair, as the issue lists them; the cut of mi_mcmc_draw_stats on L3"""
    want = {"L1": ((100.5, 3.318), (16, None)), "L2": ((132.4, 4.828, 2.324), (10, 262, 316)), "L3": ((177.5, 2.219), (24, 714)),
            "L4": ((18.94, 1.460), (34, None)), "L5": ((35.62, 3.791), (6, 76)), "L6": ((79.41, 2.027), (6, None))}
    for name, (ess, stop) in want.items():
        ref = LR.reference_lags(LR.slab(name), None)
        assert np.allclose(ref["ess"].astype(np.float64), ess, rtol=5e-4) and tuple(ref["stop"]) == stop, (name, ref["ess"], ref["stop"])
    x = LR.slab("L3")
    assert np.allclose([float(LR.reference_lags(x, K)["ess"][1]) for K in (None, 127, 255)], (2.219, 5.280, 3.377), rtol=5e-4)


def _gpu_cases():
    """(tag, slab, K) of every call of tests/test_gpu_draw_stats_lags.py that is compared with the reference"""
    for name in LR.INPUTS:
        yield name, LR.slab(name), None
    for name in ("L2", "L3"):
        yield name, LR.slab(name), 127
    yield "L2", LR.slab("L2"), 255
    for K in (0, 1, 2, 15, 16, 17, 159, 160, 161):
        yield "L1", LR.slab("L1"), K
    for n in (1, 2, 3, 4, 16, 17, 128, 129, 160):
        yield f"prefix-{n}", LR.slab_of(160, 2, 130, 0.5, 9160)[:n], None
    yield "tiling", LR.slab_of(*LR.TILING), None
    for Cn in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65):
        yield f"chains-{Cn}", LR.slab_of(170, 2, Cn, 0.5, 9170 + Cn), 40
    yield "dims-130", LR.slab_of(170, 130, 20, 0.5, 9171), 40
    yield "groups", LR.slab_of(200, 1, 1100, 0.6, 9200), None
    yield "offsets", LR.slab_of(300, 4, 130, 0.5, 9300, R.OFFSETS), None


def test_margins_of_every_gpu_input():
    worst = np.inf
    for tag, x, K in _gpu_cases():
        m = LR.reference_lags(x, K)["margin"]
        assert (m >= 100.0).all(), (tag, K, m)
        worst = min(worst, float(m.min()))
    print(f"smallest margin over the GPU inputs: {worst:.3g}")


@pytest.mark.parametrize("n", [1, 2, 17, 129, 161, 1000, 2500])
def test_band_plan_covers_every_offset_once(n):
    for K in sorted({k for k in (0, 1, 15, 16, 17, 127, 128, n - 1) if k <= n - 1}):
        ND = (K + 15) // 16 + 1
        assert A.n_offsets(K) == ND
        plan = A.band_plan(n, K)
        covered = [dl for lo, hi in plan for dl in range(lo, hi)]
        assert covered == list(range(ND)), (n, K, plan)
        assert all(0 < hi - lo <= 16 for lo, hi in plan)
        assert A.lags_complete(plan[-1], K) == K + 1                 # the last band completes the window
        q, r = divmod(K, 16)
        assert q + (1 if r else 0) < ND                              # both offsets the last lag straddles
    assert A.band_plan(n, 10 ** 9) == A.band_plan(n, n - 1)
    assert A.band_plan(1000, 999) == [(0, 8), (8, 16), (16, 32), (32, 48), (48, 64)]


def _lags(slab, n_keep, d, n_chains, outs=(1, 1, 1, 1, 1), max_lag=0xFFFFFFFF):
    buf = np.zeros(8)
    ptr = lambda on: buf.ctypes.data if on else None
    return mcmc_amd.lib().mi_mcmc_draw_stats_lags(slab, mcmc_amd.MEM_HOST, n_keep, d, n_chains, max_lag, *[ptr(o) for o in outs], None)


def _ranked(slab, n_keep, d, n_chains, outs=(1,) * 6):
    buf = np.zeros(8)
    ptr = lambda on: buf.ctypes.data if on else None
    return mcmc_amd.lib().mi_mcmc_draw_stats_ranked_lags(slab, mcmc_amd.MEM_HOST, n_keep, d, n_chains, 0xFFFFFFFF, *[ptr(o) for o in outs], None)


X = np.zeros(64)
BAD = [
    ("null slab", lambda: _lags(0, 4, 1, 4)),
    ("n_keep = 0", lambda: _lags(X.ctypes.data, 0, 1, 4)),
    ("d = 0", lambda: _lags(X.ctypes.data, 4, 0, 4)),
    ("n_chains = 0", lambda: _lags(X.ctypes.data, 4, 1, 0)),
    ("n_keep beyond 32 bits", lambda: _lags(X.ctypes.data, 1 << 32, 1, 4)),
    ("n_chains beyond 32 bits", lambda: _lags(X.ctypes.data, 4, 1, 1 << 32)),
    ("d beyond 65 536", lambda: _lags(X.ctypes.data, 4, 65537, 4)),
    ("all outputs NULL", lambda: _lags(X.ctypes.data, 4, 1, 4, outs=(0, 0, 0, 0, 0))),
    ("ranked: null slab", lambda: _ranked(0, 4, 1, 4)),
    ("ranked: d = 0", lambda: _ranked(X.ctypes.data, 4, 0, 4)),
    ("ranked: d beyond 65 536", lambda: _ranked(X.ctypes.data, 4, 65537, 4)),
    ("ranked: n_keep < 4", lambda: _ranked(X.ctypes.data, 3, 1, 4)),
    ("ranked: n_chains beyond 32 bits", lambda: _ranked(X.ctypes.data, 4, 1, 1 << 32)),
    ("ranked: all outputs NULL", lambda: _ranked(X.ctypes.data, 4, 1, 4, outs=(0,) * 6)),
]


@pytest.mark.parametrize("case", range(len(BAD)), ids=[b[0] for b in BAD])
def test_bad_arguments_are_rejected_without_a_gpu(case):
    tag, call = BAD[case]
    assert call() == mcmc_amd.MI_ERR_BAD_ARG, tag
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draw_stats_ranked_lags:" if tag.startswith("ranked") else "draw_stats_lags:"), msg


def test_the_symbols_are_there():
    for name in ("mi_mcmc_draw_stats_lags", "mi_mcmc_draw_stats_ranked_lags"):
        assert name in mcmc_amd.EXPORTS and hasattr(mcmc_amd.lib(), name)
    assert hasattr(mcmc_amd.lib(), "mi_mcmc_test_draw_stats_lags_last")
    assert mcmc_amd.STATS_ALL_LAGS == A.ALL_LAGS == 0xFFFFFFFF
    for f in ("draw_stats_lags", "draw_stats_ranked_lags", "test_draw_stats_lags_last"):
        assert callable(getattr(mcmc_amd, f))
    for f in ("acov_ref", "ess_lags_ref", "band_plan", "draw_stats_ranked_lags_ref"):
        assert callable(getattr(A, f))
