"""GPU: mi_mcmc_draw_stats_lags / mi_mcmc_draw_stats_ranked_lags -- every lag of long series on the fp64 matrix cores (stats_band_kernel,
mcmc_amd/csrc/draw_stats_lags.hpp) against the exact reference tests/draw_stats_lags_ref.py, inside the bounds tests/draw_stats_ref.py derives.

Every case compares each element of mean / acov / rhat / ess with the reference, prints its worst |got - ref| / bound, compares `ended`, and asserts
through the probe (mi_mcmc_test_draw_stats_lags_last) that its shape reached the path it names: ND block offsets, the bands of the schedule
(mcmc_amd.acov.band_plan), the band passes over a subset of the dimensions, the time tiles of 128 rows per series, the chain groups G of
max(1, min(64, ceil(C / 16), 2^18 / d)) and the chains per tile.  tests/test_draw_stats_lags_cpu.py asserts the margin of every input used here."""
import functools

import numpy as np
import pytest

import draw_stats_lags_ref as LR
import draw_stats_ref as R
import mcmc_amd
from mcmc_amd import acov as A
from mcmc_amd import rank_stats
from mcmc_amd.ess import ess_per_chain

pytestmark = pytest.mark.gpu


def _frozen(s):
    for a in s.values():
        if a is not None:
            a.setflags(write=False)
    return s


def _run(x, K=None, want_acov=True):
    """one engine call, what the probe says of it, and the probe held to the host rules"""
    s = _frozen(mcmc_amd.draw_stats_lags(x, max_lag=K, want_acov=want_acov))
    p = mcmc_amd.test_draw_stats_lags_last()
    n, d, C = x.shape
    Kw = LR.window(n, K)
    G = max(1, min(64, (C + 15) // 16, 2 ** 18 // d))
    assert (p["K"], p["ND"], p["bands"], p["time_tiles"], p["G"]) == (Kw, A.n_offsets(Kw), len(A.band_plan(n, Kw)), (n + 127) // 128, G), p
    assert p["tile_chains"] == min(16, (C + G - 1) // G)
    assert (s["acov"] is None) == (not want_acov)
    return s, p


@functools.lru_cache(maxsize=None)
def _call(name, K=None, want_acov=True):
    return _run(LR.slab(name), K, want_acov)


def _inside(tag, x, K=None, want_acov=True):
    s, p = _run(x, K, want_acov)
    ref = LR.reference_lags(x, K)
    LR.inside(tag, s, ref, f" ND {p['ND']} bands {p['bands']} subset-passes {p['subset_passes']} smallest {p['smallest_subset']} time-tiles {p['time_tiles']} "
                           f"G {p['G']} tile-chains {p['tile_chains']};")
    return s, p, ref


def _bits(a, b, keys=("mean", "rhat", "ess", "ended")):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in keys)


# ---- 1. every lag
@pytest.mark.parametrize("name", sorted(LR.INPUTS))
def test_every_lag(name):
    x = LR.slab(name)
    s, p = _call(name)
    ref = LR.reference_lags(x, None)
    LR.inside(name, s, ref, f" ND {p['ND']} bands {p['bands']} time-tiles {p['time_tiles']} G {p['G']};")
    assert s["acov"].shape == (x.shape[0], x.shape[1]) and np.isfinite(s["acov"]).all()
    assert s["ended"].all() and ref["ended"].all()
    assert np.allclose(s["ess"], ess_per_chain(x), rtol=1e-8, atol=0.0)          # no relaxation for phi >= 0.9
    assert p["subset_passes"] == 0                                               # with acov every band runs over every dimension


# ---- 2. the cut is gone
def test_the_cut_is_gone():
    x = LR.slab("L3")
    s, _ = _call("L3")
    old = mcmc_amd.draw_stats(x)
    assert mcmc_amd.test_draw_stats_last()["route"] == 2
    print(f"L3 dimension 1: every lag {s['ess'][1]:.4g}, 128 lags {old['ess'][1]:.4g}")
    assert s["ess"][1] < 0.5 * old["ess"][1]
    full, cut = LR.reference_lags(x, None), R.reference_of(x)
    assert abs(s["ess"][0] - old["ess"][0]) <= full["ess_bound"][0] + cut["ess_bound"][0]


# ---- 3. windows
@pytest.mark.parametrize("name,ended", [("L2", (1, 0, 0)), ("L3", (1, 0))])
def test_window_of_128_lags(name, ended):
    x = LR.slab(name)
    s, p = _call(name, 127)
    ref = LR.reference_lags(x, 127)
    LR.inside(f"{name} K = 127", s, ref)
    assert s["acov"].shape == (128, x.shape[1]) and (p["ND"], p["bands"]) == (9, 2)
    old, cut = mcmc_amd.draw_stats(x), R.reference_of(x)
    assert np.all(np.abs(s["acov"] - old["acov"][:128]) <= ref["acov_bound"] + cut["acov_bound"])
    assert tuple(s["ended"]) == ended
    assert R.worst(s["ess"], ref["ess"], ref["ess_bound"]) <= 1.0                # the reference truncated at K


def test_window_of_256_lags():
    s, p, ref = _inside("L2 K = 255", LR.slab("L2"), 255)
    assert tuple(s["ended"]) == (1, 0, 0) and ref["stop"][1:] == [None, None]    # the stops are at 262 and 316
    assert s["acov"].shape == (256, 3)


@pytest.mark.parametrize("K", [0, 1, 2, 15, 16, 17, 159, 160, 161, mcmc_amd.STATS_ALL_LAGS])
def test_window_edges(K):
    x = LR.slab("L1")
    n = x.shape[0]
    s, p, ref = _inside(f"L1 K = {K}", x, K)
    Kw = min(K, n - 1)
    assert s["acov"].shape == (Kw + 1, 2) and p["ND"] == (Kw + 15) // 16 + 1
    if K == 0:
        assert np.array_equal(s["ess"], [n, n]) and not s["ended"].any()
    if K >= n - 1:
        assert _bits(s, _call("L1")[0], ("mean", "rhat", "ess", "ended", "acov"))  # the clamp


# ---- 4. short series against the existing routes
def _against_draw_stats(tag, x):
    s, p, ref = _inside(tag, x)
    old, cut = mcmc_amd.draw_stats(x), R.reference_of(x)
    assert cut["nlag"] == x.shape[0]
    for k in ("mean", "acov", "rhat", "ess"):
        assert np.all(np.abs(s[k] - old[k]) <= ref[f"{k}_bound"] + cut[f"{k}_bound"]), k
    assert s["ended"].all()


@pytest.mark.parametrize("name", ["L5", "L6"])
def test_short_series_agree_with_draw_stats(name):
    _against_draw_stats(name, LR.slab(name))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 16, 17, 128, 129, 160])
def test_prefixes_agree_with_draw_stats(n):
    _against_draw_stats(f"prefix-{n}", np.ascontiguousarray(LR.slab_of(160, 2, 130, 0.5, 9160)[:n]))


# ---- 5. ladder
def test_ladder_runs_further_bands_over_the_open_dimensions_only():
    full, pf = _call("L2")
    s, p = _call("L2", None, False)
    assert _bits(s, full)
    assert pf["subset_passes"] == 0
    # dimension 0 stops at lag 10, inside the first band (lags 0..112); dimensions 1 and 2 stop at 262 and 316: bands [8,16) and [16,32) run over the two of
    # them (lags 0..240 and 0..496 complete), nothing after
    assert (p["subset_passes"], p["smallest_subset"]) == (2, 2) and p["bands"] == 3
    LR.inside("L2 (no acov)", s, LR.reference_lags(LR.slab("L2"), None))


# ---- 6. time tiling
def test_time_tiles():
    x = LR.slab_of(*LR.TILING)
    s, p, ref = _inside("tiling", x)
    assert p["time_tiles"] == 20 and p["bands"] == 11 and s["acov"].shape == (2500, 1)


# ---- 7. chain and dimension edges
@pytest.mark.parametrize("Cn", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65])
def test_chain_edges(Cn):
    x = LR.slab_of(170, 2, Cn, 0.5, 9170 + Cn)
    s, p, ref = _inside(f"chains-{Cn}", x, 40)
    assert s["acov"].shape == (41, 2) and p["ND"] == 4
    if Cn == 1:
        n = 170
        W = x.var(axis=0, ddof=1)[:, 0]
        assert np.allclose(s["rhat"], np.sqrt((n - 1) / n * W / W), rtol=1e-14)     # B/n = 0 with one chain: the reference's rule


def test_many_dimensions():
    s, p, ref = _inside("dims-130", LR.slab_of(170, 130, 20, 0.5, 9171), 40)
    assert p["G"] == 2 and p["tile_chains"] == 10


def test_many_chain_groups():
    s, p, ref = _inside("groups", LR.slab_of(200, 1, 1100, 0.6, 9200))
    assert p["G"] == 64 and p["tile_chains"] == 16                               # 18 chains per group: a full tile and one of two chains


# ---- 8. centring
def test_offsets_per_dimension():
    _inside("offsets", LR.slab_of(300, 4, 130, 0.5, 9300, R.OFFSETS))


def test_chains_that_disagree():
    x = LR.slab_of(300, 2, 200, 0.3, 9301, None, 1e6)
    s, p = _run(x)
    ref = LR.reference_lags(x, None)
    w = R.worst(s["rhat"], ref["rhat"], ref["rhat_bound"])
    print(f"draw_stats_lags delta 1e6: R-hat {s['rhat']}, worst |got - ref| / bound {w:.3g}")
    assert w <= 1.0


# ---- 9. non-finite
@pytest.mark.parametrize("want_acov", [True, False])
def test_non_finite_samples_stay_in_their_dimension(want_acov):
    clean = LR.slab_of(300, 3, 130, 0.5, 9302)
    x = clean.copy()
    x[17, 1, 5] = np.nan
    x[201, 1, 77] = np.inf
    c, _ = _run(clean, None, want_acov)
    s, _ = _run(x, None, want_acov)
    keys = ("mean", "rhat", "ess", "ended") + (("acov",) if want_acov else ())
    for k in keys:
        for j in (0, 2):
            assert np.array_equal(s[k][..., j], c[k][..., j]) and np.array_equal(np.ascontiguousarray(s[k][..., j]).view(np.uint8), np.ascontiguousarray(c[k][..., j]).view(np.uint8)), (k, j)
    want = A.draw_stats_lags_ref(x, None)
    for k in keys:
        assert np.array_equal(s[k][..., 1], want[k][..., 1], equal_nan=True), (k, s[k][..., 1], want[k][..., 1])


# ---- 10. device slab
def test_device_slab():
    import torch
    x = LR.slab("L2")
    host, _ = _call("L2")
    t = torch.from_numpy(x.copy()).cuda()
    s = mcmc_amd.draw_stats_lags(t, n_keep=x.shape[0], d=x.shape[1], n_chains=x.shape[2], mem=mcmc_amd.MEM_DEVICE)
    torch.cuda.synchronize()
    assert _bits(s, host, ("mean", "rhat", "ess", "ended", "acov"))


# ---- 11. ranked
RANKED = {"mixing": (1000, 3, 200, 0.7, 1000), "slow": (600, 2, 130, (0.5, 0.99), 9600)}


@functools.lru_cache(maxsize=None)
def _ranked_case(name):
    x = LR.slab_of(*RANKED[name])
    return x, rank_stats.draw_stats_ranked_ref(x)


@pytest.mark.parametrize("name", sorted(RANKED))
def test_ranked_with_every_lag(name):
    x, want = _ranked_case(name)
    got = mcmc_amd.draw_stats_ranked_lags(x)
    for k in ("rhat", "rhat_bulk", "rhat_tail"):
        assert np.allclose(got[k], want[k], rtol=1e-10, atol=0.0), (k, got[k], want[k])
    for k in ("ess_bulk", "ess_tail"):
        assert np.allclose(got[k], want[k], rtol=1e-8, atol=0.0), (k, got[k], want[k])       # no relaxation for phi >= 0.9
    assert got["ended"].all()
    mine = A.draw_stats_ranked_lags_ref(x)
    assert np.array_equal(got["ended"], mine["ended"]) and np.allclose(got["ess_tail"], mine["ess_tail"], rtol=1e-8, atol=0.0)


def test_ranked_window_cuts_the_slow_dimension():
    x, _ = _ranked_case("slow")
    got = mcmc_amd.draw_stats_ranked_lags(x, max_lag=127)
    mine = A.draw_stats_ranked_lags_ref(x, 127)
    assert got["ended"][1] == 0 and np.array_equal(got["ended"], mine["ended"])
    for k in ("ess_bulk", "ess_tail"):
        assert np.allclose(got[k], mine[k], rtol=1e-8, atol=0.0), (k, got[k], mine[k])
