"""GPU: device reducers over draws_out slabs (mi_mcmc_draw_stats) against an exact reference, on every route of the host ladder.

The reference (np.longdouble), the per-element bounds and every input live in tests/draw_stats_ref.py, whose docstring derives the bounds;
tests/test_draw_stats_ref_cpu.py checks reference and bounds on the CPU.  Every case here compares mean, autocovariance (where asked for), R-hat and
ESS with the reference in every element, prints its worst |got - ref| / bound, and asserts through the route probe (mi_mcmc_test_draw_stats_last) that
its shape reached the path it names:

  n <= 128         route 0: stats_gram_kernel<NB>, NB = ceil(n / 16), G = min(64, ceil(2048 / d), ceil(C / 64)) chain groups, tiles of 64 chains
  129 <= n <= 160  route 1: the ladder -- stats_window_kernel<16> (only without acov), then lag passes of stats_acov_kernel over the open dimensions
  n > 160          route 2: stats_acov_tiled_kernel, lags 0..127, NaN beyond

The assertions the file had before the bounds (np.allclose against float64 numpy) are kept next to them on the shapes it had."""
import functools
import warnings

import numpy as np
import pytest

import draw_stats_ref as R
import mcmc_amd
from mcmc_amd.ess import ess_per_chain

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _call(name, want_acov=True):
    """ONE engine call per (input, want_acov) and what the probe says of it -- shared by the tests, never modified"""
    s = mcmc_amd.draw_stats(R.slab(name), want_acov=want_acov)
    probe = mcmc_amd.test_draw_stats_last()
    for a in s.values():
        if a is not None:
            a.setflags(write=False)
    return s, probe


def _inside(tag, s, ref, probe=None):
    """every element of s inside the bounds of ref; prints the worst ratios; returns them"""
    n, nlag = ref["n"], ref["nlag"]
    w = dict(mean=R.worst(s["mean"], ref["mean"], ref["mean_bound"]), rhat=R.worst(s["rhat"], ref["rhat"], ref["rhat_bound"]),
             ess=R.worst(s["ess"], ref["ess"], ref["ess_bound"]))
    if s["acov"] is not None:
        assert s["acov"].shape == (n, ref["d"])
        w["acov"] = R.worst(s["acov"][:nlag], ref["acov"], ref["acov_bound"])
        assert np.isnan(s["acov"][nlag:]).all()                              # the streamed route: rows from lag 128 on are NaN
    p = "" if probe is None else f" route {probe['route']} NB {probe['NB']} G {probe['G']} tiles {probe['tiles']} window {probe['window_launches']} " \
                                 f"passes {probe['lag_passes']} subset-passes {probe['subset_passes']} smallest {probe['smallest_subset']};"
    print(f"draw_stats {tag} (n, d, C) = ({n}, {ref['d']}, {ref['C']}):{p} worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in w.items()))
    for k in ("mean", "rhat", "ess") + (("acov",) if s["acov"] is not None else ()):
        assert np.isfinite(s[k][:nlag] if k == "acov" else s[k]).all(), k
        assert w[k] <= 1.0, (k, w[k])
    return w


def _check(name, want_acov=True, route=None):
    s, probe = _call(name, want_acov)
    ref = R.reference(name)
    assert probe["route"] == (R.route_of(ref["n"]) if route is None else route)
    assert (probe["G"], probe["tiles"]) == R.gram_groups(ref["n"], ref["d"], ref["C"])
    assert (s["acov"] is None) == (not want_acov)
    _inside(f"{name}{'' if want_acov else ' (no acov)'}", s, ref, probe)
    return s, probe, ref


def _numpy_rhat(x):
    n = x.shape[0]
    m = x.mean(axis=0); W = x.var(axis=0, ddof=1).mean(axis=1); B_n = m.var(axis=1, ddof=1)
    return np.sqrt(((n - 1) / n * W + B_n) / W)


# ---- the shapes the suite has always had: the earlier assertions, and the bounds
@pytest.mark.parametrize("n,d,C,phi", [(100, 5, 700, 0.6), (40, 3, 64, 0.0), (160, 2, 1000, 0.9), (7, 4, 130, 0.3)])
def test_draw_stats_match_the_numpy_definitions(n, d, C, phi):
    name = f"old-{n}-{d}-{C}"
    x = R.slab(name)
    assert np.array_equal(x, R.ar1(n, d, C, phi, seed=n))
    s, probe, ref = _check(name)
    assert np.allclose(s["mean"], x.mean(axis=(0, 2)), rtol=1e-12, atol=1e-12)
    xc = x - x.mean(axis=(0, 2), keepdims=True)
    acov = np.stack([(xc[: n - k] * xc[k:]).sum(axis=0).mean(axis=1) / (n - k) for k in range(n)])
    assert np.allclose(s["acov"], acov, rtol=1e-10, atol=1e-12)
    assert np.allclose(s["ess"], ess_per_chain(x), rtol=1e-8)
    assert np.allclose(s["rhat"], _numpy_rhat(x), rtol=1e-10)
    assert np.all(np.abs(s["rhat"] - 1.0) < 0.2)


def test_draw_stats_of_a_real_run():
    from mcmc_amd import synth
    d, C, keep = 16, 4096, 60
    prec = synth.dense_gaussian_precision(d)
    st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=50, n_keep_draws=keep, n_leap_steps=8, step_size=0.15)
    draws, _ = mcmc_amd.hmc(mcmc_amd.TARGET_GAUSS_DENSE, synth.initial_states(C, d, seed=3), st, prec=prec)
    s = mcmc_amd.draw_stats(draws)
    assert np.allclose(s["ess"], ess_per_chain(draws), rtol=1e-8)
    assert np.all(s["rhat"] < 1.05) and np.all(np.abs(s["mean"]) < 0.1)


@pytest.mark.parametrize("n,d,C,phi", [(1000, 3, 200, 0.7), (161, 2, 130, 0.2), (517, 2, 64, 0.95)])
def test_long_series_are_streamed_and_truncated_at_128_lags(n, d, C, phi):
    """n_keep beyond 160 (the reference's default is 1 000 kept draws): lags 0..127 from the time-tiled kernel, NaN beyond;
    mean, R-hat and Geyer's ESS (which stops at the first non-positive pair, long before lag 127 here) as defined in ess.py."""
    name = f"old-{n}-{d}-{C}"
    x = R.slab(name)
    assert np.array_equal(x, R.ar1(n, d, C, phi, seed=n))
    s, probe, ref = _check(name, route=2)
    assert np.allclose(s["mean"], x.mean(axis=(0, 2)), rtol=1e-12, atol=1e-12)
    xc = x - x.mean(axis=(0, 2), keepdims=True)
    acov = np.stack([(xc[: n - k] * xc[k:]).sum(axis=0).mean(axis=1) / (n - k) for k in range(128)])
    assert np.allclose(s["acov"][:128], acov, rtol=1e-10, atol=1e-12) and np.isnan(s["acov"][128:]).all()
    assert np.allclose(s["rhat"], _numpy_rhat(x), rtol=1e-10)
    if phi < 0.9:
        assert np.allclose(s["ess"], ess_per_chain(x), rtol=1e-8)
    else:                                   # the sum may still be positive at lag 127: the device reports the truncated sum
        assert np.all(s["ess"] >= ess_per_chain(x) * (1 - 1e-8)) and np.all(s["ess"] < n)


@pytest.mark.parametrize("n,d,C,phi", [(100, 5, 700, 0.6), (40, 3, 64, 0.0), (160, 2, 1000, 0.9), (7, 4, 130, 0.3), (1000, 3, 200, 0.7),
                                       (100, 2, 300, 0.97), (20, 130, 70, 0.5), (150, 2, 300, 0.97)])
def test_ess_and_rhat_without_the_full_autocovariance(n, d, C, phi):
    """acov == NULL.  n <= 128: the one-pass Gram kernel all the same (every lag; also phi = 0.97 at n = 100).  129 <= n <= 160: the first 16 lags
    straight from HBM (stats_window_kernel<16>), then lag passes of 32, then 48 lags for the dimensions whose Geyer sum has not ended: phi = 0.97 at
    n = 150 does not end within 48 lags and falls through to the passes after them.  Beyond 160: the streamed kernel.  Same numbers as ess.py."""
    name = f"oldq-{n}-{d}-{C}"
    x = R.slab(name)
    assert np.array_equal(x, R.ar1(n, d, C, phi, seed=n + C))
    s, probe, ref = _check(name, want_acov=False)
    assert s["acov"] is None
    assert np.allclose(s["mean"], x.mean(axis=(0, 2)), rtol=1e-12, atol=1e-12)
    if n <= 160:
        assert np.allclose(s["ess"], ess_per_chain(x), rtol=1e-8)
    else:
        full = mcmc_amd.draw_stats(x)["ess"]
        assert np.allclose(s["ess"], full, rtol=1e-8)
    assert np.allclose(s["rhat"], _numpy_rhat(x), rtol=1e-10)
    if R.route_of(n) == 1:
        assert probe["window_launches"] == 1
        plan = R.ladder_plan(ref)
        assert (probe["lag_passes"], probe["subset_passes"], probe["smallest_subset"]) == (plan["lag_passes"], plan["subset_passes"], plan["smallest_subset"])
        if phi == 0.97:
            assert probe["lag_passes"] >= 2                      # it does fall through
    else:
        assert probe["window_launches"] == 0 and probe["lag_passes"] == 0


# ---- Gram route: the tile loop (deposit(tile + 1), request(tile + 2), both LDS buffers, the rotation of the moment adder past tile 7)
@pytest.mark.parametrize("want_acov", [True, False], ids=["acov", "noacov"])
@pytest.mark.parametrize("name", R.TILE_LOOP)
def test_gram_tile_loop(name, want_acov):
    """(33, 1, 40000): G = 64, 625 chains per group = 10 tiles, the last of 49 chains; (100, 1, 8200): 129 chains per group = three tiles, the third of
    one chain, the last group two tiles; (5, 2049, 200): d past 2048 forces G = 1 -- four tiles (64, 64, 64, 8), rows 0, 2, 4 for the centre."""
    s, probe, ref = _check(name, want_acov)
    G, tiles, NB = R.TILE_LOOP_EXPECT[name]
    assert (probe["route"], probe["G"], probe["tiles"], probe["NB"]) == (0, G, tiles, NB)


def test_gram_tile_loop_device_resident_on_a_side_stream():
    import torch
    name = "tiles-33-1-40000"
    x = R.slab(name)
    n, d, C = x.shape
    host, _ = _call(name)
    xd = torch.from_numpy(x.copy()).cuda()                       # (the shared slab is read-only)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = mcmc_amd.draw_stats(xd, n, d, C, mem=mcmc_amd.MEM_DEVICE, stream=side.cuda_stream)
    probe = mcmc_amd.test_draw_stats_last()
    side.synchronize()
    assert (probe["route"], probe["tiles"]) == (0, 10)
    for k in ("mean", "acov", "rhat", "ess"):
        assert np.array_equal(s[k], host[k]), k                  # the same bits as the host call
    assert np.array_equal(xd.cpu().numpy(), x)                   # the slab is unchanged


# ---- Gram route: every instantiation NB = 1..8 and the edges of each (n = 16 NB - 1, 16 NB, 16 NB + 1)
@pytest.mark.parametrize("n", R.GRAM_NS)
def test_gram_every_nb_and_its_edges(n):
    s, probe, ref = _check(f"nb-{n}")
    assert (probe["route"], probe["NB"]) == (0, (n + 15) // 16)
    assert s["acov"].shape == (n, 2)
    if n < 4:
        assert np.array_equal(s["ess"], np.full(2, float(n)))
    if n == 1:
        assert np.array_equal(s["rhat"], np.ones(2))             # W = 0 under today's rule


def test_n_128_and_129_land_on_different_routes():
    """the same series, one draw longer: the Gram kernel's last shape and the ladder's first"""
    s128, p128, _ = _check("nb-128")
    s129, p129, _ = _check(R.BOUNDARY_129)
    assert np.array_equal(R.slab(R.BOUNDARY_129)[:128], R.slab("nb-128"))
    assert (p128["route"], p128["NB"]) == (0, 8) and (p129["route"], p129["NB"]) == (1, 0) and p129["lag_passes"] == 3 and p129["window_launches"] == 0


# ---- the ladder, 129 <= n <= 160
@pytest.mark.parametrize("name", R.LADDER_ACOV)
def test_ladder_with_the_autocovariance(name):
    """every lag in passes of three blocks of 16; n = 129: the last block holds ONE lag; 145, 159: ragged last blocks; 160: none"""
    s, probe, ref = _check(name)
    n = ref["n"]
    assert (probe["route"], probe["window_launches"], probe["lag_passes"], probe["subset_passes"]) == (1, 0, ((n + 15) // 16 + 2) // 3, 0)


def test_ladder_closes_dimensions_at_different_passes():
    """(150, 5, 130), phi = (0.97, 0, 0.9, 0.3, 0.99), no acov: the open set after the window pass is {0, 2, 4} -- a `dims` subset that is not
    contiguous --, and it shrinks from pass to pass.  The launch counts are derived on the CPU from the reference autocovariances
    (test_draw_stats_ref_cpu.py); ESS and R-hat are compared with the reference, not with another device call."""
    s, probe, ref = _check(R.LADDER_SUBSETS, want_acov=False)
    plan = R.ladder_plan(ref)
    assert plan["open_after_window"] == [0, 2, 4]
    assert probe["window_launches"] == 1
    assert (probe["lag_passes"], probe["subset_passes"], probe["smallest_subset"]) == (plan["lag_passes"], plan["subset_passes"], plan["smallest_subset"])
    assert probe["subset_passes"] >= 1


# ---- the streamed route: tile + halo exactly (192 = 64 + 128), one past it, a multiple of the tile; C = 65: the second lane tile has one chain
@pytest.mark.parametrize("name", R.TILED_EDGES)
def test_tiled_edges(name):
    s, probe, ref = _check(name)
    assert probe["route"] == 2 and np.isnan(s["acov"][128:]).all() and np.isfinite(s["acov"][:128]).all()
    _check(name, want_acov=False)


# ---- chains and groups: C = 1, a tile less one / exactly / plus one; C = 4097: G = 64, the last group holds two chains
@pytest.mark.parametrize("name", R.CHAIN_EDGES)
def test_chain_counts_at_the_tile_edges(name):
    s, probe, ref = _check(name)
    if ref["C"] == 4097:
        assert (probe["G"], probe["tiles"]) == (64, 2)
    _check(name, want_acov=False)


# ---- centring
@pytest.mark.parametrize("n,want_acov", [(100, True), (150, True), (150, False), (300, True)])
def test_large_offsets_per_dimension(n, want_acov):
    """means (0, 1e3, 1e6, -1e8) with unit sd, on a Gram, a ladder (both ways) and a streamed shape: the bounds do not know the offset"""
    _check(R.CENTRING[n], want_acov)


@pytest.mark.parametrize("n", sorted(R.DRIFT))
def test_a_drifting_start(n):
    """x_t = 50 * 0.9^t + AR(1): the first draw sits 50 sd from the mode -- the case the provisional centre (first, middle, last row) was made for"""
    _check(R.DRIFT[n])
    _check(R.DRIFT[n], want_acov=False)


# ---- chains that disagree: offsets per chain uniform in +-delta, unit within-chain sd -- the case R-hat exists to report
@pytest.mark.parametrize("delta", R.DELTAS, ids=lambda v: f"{v:g}")
def test_rhat_of_chains_that_disagree_is_inside_its_bound_on_every_route(delta):
    """n = 100: the Gram kernel; n = 150 without acov: the window kernel; n = 150 with acov: the lag-block kernel; n = 300: the streamed kernel.
    The three lengths are prefixes of one series, so the R-hat values differ; what must agree is each route's deviation from its own exact value:
    got / ref - 1 of any two routes within twice the bound, and on the one slab two routes share (n = 150) the values themselves."""
    runs = [(R.DISAGREE[(delta, 100)], True, 0), (R.DISAGREE[(delta, 150)], False, 1), (R.DISAGREE[(delta, 150)], True, 1), (R.DISAGREE[(delta, 300)], True, 2)]
    dev, rel = [], []
    for name, want_acov, route in runs:
        s, probe, ref = _check(name, want_acov, route=route)
        assert probe["window_launches"] == (1 if (route == 1 and not want_acov) else 0)
        assert np.all(ref["rhat"] > 10.0)                        # chains that share nothing
        dev.append((s["rhat"].astype(R.LD) / ref["rhat"] - 1).astype(np.float64))
        rel.append((ref["n"] + ref["C"] + 64) * 2.0 ** -52)
        print(f"    R-hat {s['rhat']}, relative deviation {dev[-1]}, bound {rel[-1]:.3g}")
    for a in range(4):
        for b in range(a + 1, 4):
            assert np.all(np.abs(dev[a] - dev[b]) <= 2 * max(rel[a], rel[b])), (a, b, dev[a], dev[b])
    same = np.abs(_call(runs[1][0], False)[0]["rhat"] - _call(runs[2][0], True)[0]["rhat"])
    assert np.all(same <= 2 * R.reference(runs[1][0])["rhat_bound"])


# ---- non-finite samples stay in their own dimension
@pytest.mark.parametrize("name", R.NONFINITE)
def test_non_finite_samples_stay_in_their_dimension(name):
    """one NaN and one +inf in dimension 1: dimensions 0 and 2 return the bits of the clean call; dimension 1 is what the definitions give"""
    clean, _ = _call(name)
    x = R.slab(name).copy()
    n = x.shape[0]
    x[5, 1, 7] = np.nan
    x[n - 3, 1, 100] = np.inf
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        ref = R.reference_of(x)
    for want_acov in (True, False):
        s = mcmc_amd.draw_stats(x, want_acov=want_acov)
        base = clean if want_acov else _call(name, False)[0]
        for k in ("mean", "rhat", "ess") + (("acov",) if want_acov else ()):
            assert np.array_equal(s[k][..., [0, 2]], base[k][..., [0, 2]]), k
            assert np.array_equal(s[k][..., 1], ref[k][..., 1].astype(np.float64), equal_nan=True), (k, s[k][..., 1])
    assert np.isnan(ref["mean"][1]) and np.isnan(ref["acov"][:, 1].astype(np.float64)).all()


def test_device_transpose_to_chain_major():
    import torch
    n, d, C = 37, 5, 1000
    x = np.random.default_rng(0).standard_normal((n, d, C))
    xd = torch.from_numpy(x).cuda()
    out = torch.empty((C, d, n), dtype=torch.float64, device="cuda")
    mcmc_amd.draws_to_chain_major_device(xd, n, d, C, out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.ascontiguousarray(x.transpose(2, 1, 0)))
    n, d, C = 300, 2, 130                                   # more draws than one LDS tile holds
    x = np.random.default_rng(1).standard_normal((n, d, C))
    out = torch.empty((C, d, n), dtype=torch.float64, device="cuda")
    mcmc_amd.draws_to_chain_major_device(torch.from_numpy(x).cuda(), n, d, C, out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.ascontiguousarray(x.transpose(2, 1, 0)))
