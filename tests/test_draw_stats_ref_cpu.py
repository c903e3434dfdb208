"""CPU: the exact reference of the draw_stats GPU tests (tests/draw_stats_ref.py) is itself right, and its bounds are bounds.

 - On the benign shapes the suite has always had, the reference equals mcmc_amd.ess.ess_per_chain and plain float64 numpy to 1e-12.
 - On EVERY input of tests/test_gpu_draw_stats.py, careful float64 numpy -- the slab shifted by a representable constant per dimension, then the plain
   definitions: mean, autocovariance about the pooled mean, two-pass R-hat -- stays inside the bounds: a correct float64 computation passes the check the
   kernels are held to.  Worst |numpy - ref| / bound over all inputs and elements, as measured when this file was written:  mean 0.012,  acov 0.0054,
   R-hat 0.61 (chain means spread over +-1e6 sd: the shift itself rounds at 1e-10 sd there; 0.0081 on every other input).  Without the shift numpy is
   3.9e4 (acov) and 2.5e3 (R-hat) times outside at mean = -1e8, sd = 1 -- one double cannot hold that mean to better than 1e-8 sd --, and so is the
   exact reference's own longdouble sum, which is why the reference shifts too.
 - The Geyer margin holds for every input and dimension: at the reference's stopping pair and at every earlier pair |acov_t + acov_{t+1}| exceeds 100 times
   the pair's bound (smallest ratio over all inputs: 1.0e6), so an implementation inside the acov bounds stops at the reference's lag.
 - The launches of the ladder case (n = 150, five dimensions with different phi, no autocovariance asked for) are derived here from the reference
   autocovariances; the GPU test asserts the same numbers against the route probe."""
import numpy as np
import pytest

import draw_stats_ref as R
from mcmc_amd.ess import ess_per_chain

ALL = sorted(R.SPECS)


def _numpy64(x):
    """Careful float64 numpy: the slab is first shifted by a REPRESENTABLE constant per dimension (the mean of the first row), as any float64
    implementation must at |mean| / sd = 1e8 -- the pooled mean itself is a double 1e-8 sd wide there, and so are the chain means --; everything
    after that is the plain definition: mean, autocovariance about the pooled mean, two-pass R-hat."""
    n, d, C = x.shape
    a = x[0].mean(axis=1)
    xs = x - a[None, :, None]
    e = xs.mean(axis=(0, 2))
    xc = xs - e[None, :, None]
    nlag = n if n <= R.STATS_MAX_N else R.STATS_TILED_LAGS
    acov = np.stack([(xc[: n - k] * xc[k:]).sum(axis=(0, 2)) / C / (n - k) for k in range(nlag)])
    m = xs.mean(axis=0)
    W = xs.var(axis=0, ddof=1).mean(axis=1) if n > 1 else np.zeros(d)
    B_n = m.var(axis=1, ddof=1) if C > 1 else np.zeros(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        rhat = np.where(W > 0, np.sqrt(((n - 1) / n * W + B_n) / np.where(W > 0, W, 1.0)), 1.0)
    return a + e, acov, rhat


@pytest.mark.parametrize("name", R.OLD_FULL + R.OLD_LONG + R.OLD_NOACOV)
def test_reference_equals_the_library_definitions_on_benign_shapes(name):
    x, ref = R.slab(name), R.reference(name)
    n = ref["n"]
    mean, acov, rhat = _numpy64(x)
    assert np.allclose(ref["mean"].astype(np.float64), mean, rtol=1e-12, atol=1e-12)
    assert np.allclose(ref["acov"].astype(np.float64), acov, rtol=1e-12, atol=1e-12)
    assert np.allclose(ref["rhat"].astype(np.float64), rhat, rtol=1e-12, atol=0.0)
    if n <= R.STATS_MAX_N or all(s is not None for s in ref["stop"]):       # (beyond 160 draws the reference sums 128 lags: equal where the sum ended inside them)
        assert np.allclose(ref["ess"].astype(np.float64), ess_per_chain(x), rtol=1e-12, atol=0.0)
    else:
        assert np.all(ref["ess"].astype(np.float64) >= ess_per_chain(x) * (1 - 1e-12))


@pytest.mark.parametrize("name", ALL)
def test_float64_numpy_is_inside_the_bounds_and_geyer_has_its_margin(name):
    x, ref = R.slab(name), R.reference(name)
    mean, acov, rhat = _numpy64(x)
    wm, wa, wr = R.worst(mean, ref["mean"], ref["mean_bound"]), R.worst(acov, ref["acov"], ref["acov_bound"]), R.worst(rhat, ref["rhat"], ref["rhat_bound"])
    print(f"{name}: numpy float64 / bound: mean {wm:.4f} acov {wa:.4f} rhat {wr:.4f}; Geyer margin {ref['margin'].min():.3g}; stop {ref['stop'][:8]}")
    assert wm <= 1.0 and wa <= 1.0 and wr <= 1.0
    assert np.isfinite(ref["acov"].astype(np.float64)).all()
    assert ref["n"] == 1 or np.all(ref["W"] > 0)                                  # no constant chain among the inputs
    assert np.all(ref["margin"] > 100.0), (name, ref["margin"])


def test_slabs_of_one_seed_are_prefixes_of_each_other():
    assert np.array_equal(R.slab("nb-129")[:128], R.slab("nb-128")) and np.array_equal(R.slab("nb-128")[:17], R.slab("nb-17"))
    for n in (100, 150):
        assert np.array_equal(R.slab(R.DISAGREE[(1e4, 300)])[:n], R.slab(R.DISAGREE[(1e4, n)]))


def test_routes_and_groups_of_the_named_shapes():
    """host arithmetic of stats_collate.hip, restated: which shape reaches which path"""
    for name, (G, tiles, NB) in R.TILE_LOOP_EXPECT.items():
        n, d, C = R.SPECS[name][:3]
        assert R.route_of(n) == 0 and R.gram_groups(n, d, C) == (G, tiles) and (n + 15) // 16 == NB
    assert sorted({(n + 15) // 16 for n in R.GRAM_NS}) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert R.route_of(128) == 0 and R.route_of(129) == 1 and R.route_of(160) == 1 and R.route_of(161) == 2
    assert R.gram_groups(10, 1, 4097) == (64, 2) and 4097 - 63 * 65 == 2                     # the last group holds two chains
    assert R.gram_groups(100, 1, 8200) == (64, 3) and 8200 - 63 * 129 == 73                  # ... and here two tiles, the first groups three (64, 64, 1)


def test_ladder_case_closes_its_dimensions_at_different_passes():
    """(150, 5, 130), phi = (0.97, 0, 0.9, 0.3, 0.99): after the 16 streamed lags the open set is {0, 2, 4} -- not contiguous --, and the
    dimensions close at different passes: what the GPU test asserts against the probe."""
    plan = R.ladder_plan(R.reference(R.LADDER_SUBSETS))
    print(plan)
    assert plan["open_after_window"] == [0, 2, 4]
    assert plan["lag_passes"] >= 2 and plan["subset_passes"] == plan["lag_passes"] and 1 <= plan["smallest_subset"] < 3
    assert len({tuple(p[2]) for p in plan["passes"]}) >= 2
    # the phi = 0.97 case of the suite does fall through at n = 150: its sum is still open after lags 0..47
    plan = R.ladder_plan(R.reference(R.FALLS_THROUGH))
    assert plan["lag_passes"] >= 2 and plan["passes"][1][2]
