"""CPU: the tile-route tests' own target library (tests/tile_targets.hip) cross-compiles for gfx950 with -Wall -Werror and its host callback is the example's
for every d the example takes; the random sweep of the route (tests/fuzz_tile.py), run on the oracle alone, draws the mix of cases its GPU slice is meant to have."""
import ctypes as C

import numpy as np
import pytest

import tile_route as tr


@pytest.fixture(scope="module")
def libs():
    if not tr.have_toolchain():
        pytest.skip("no hipcc / libmi_mcmc")
    return tr.Libs()


def test_tile_targets_library_builds_and_its_host_callback_is_the_examples(libs):
    for name in ("twisted1_run", "twisted2_run", "twisted8_run", "twisted_host_kernel_n"):
        assert hasattr(libs.get("tests"), name)
    dp = C.POINTER(C.c_double)
    rng = np.random.default_rng(0)
    for d in (2, 3, 13, 37, 64):
        P = tr.precision(d)
        tgt = tr.TwistedTile(P.ctypes.data, d, tr.B, tr.S2)
        for v in (rng.standard_normal(d), rng.standard_normal(d) * 1e80, np.where(np.arange(d) == d - 1, np.inf, 0.3)):
            v = np.ascontiguousarray(v)
            g1, g2 = np.zeros(d), np.zeros(d)
            a = libs.get("example").twisted_host_kernel(v.ctypes.data_as(dp), g1.ctypes.data_as(dp), C.byref(tgt))
            b = libs.host_kernel(v.ctypes.data_as(dp), g2.ctypes.data_as(dp), C.byref(tgt))
            assert np.array_equal(a, b, equal_nan=True) and np.array_equal(g1, g2, equal_nan=True)
    d = 128                                              # ... and beyond the example's buffers: the analytic gradient is the gradient
    P = tr.precision(d)
    tgt = tr.TwistedTile(P.ctypes.data, d, tr.B, tr.S2)
    v, g, num, h = rng.standard_normal(d) * 0.3, np.zeros(d), np.zeros(d), 1e-6
    val = libs.host_kernel(v.ctypes.data_as(dp), g.ctypes.data_as(dp), C.byref(tgt))
    for i in range(d):
        vp, vm = v.copy(), v.copy(); vp[i] += h; vm[i] -= h
        num[i] = (libs.host_kernel(vp.ctypes.data_as(dp), None, C.byref(tgt)) - libs.host_kernel(vm.ctypes.data_as(dp), None, C.byref(tgt))) / (2 * h)
    assert np.isfinite(val) and np.allclose(g, num, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("n_cases,seed", [(24, 4), (80, 107)])       # the slices of tests/test_gpu_fuzz.py::test_tile_route_random_cases_are_bit_exact
def test_the_tile_sweep_draws_the_mix_it_is_meant_to(libs, n_cases, seed):
    """Conditions on the generator and the oracle alone (no GPU): every kernel family at least twice, at least a quarter of the cases with a non-finite kept draw,
    at least a third finite throughout with both an accept and a reject."""
    import fuzz_tile
    fails, tally = fuzz_tile.sweep(n_cases, seed, verbose=False, oracle_only=True)
    assert fails == 0
    assert set(tally["families"]) == set(fuzz_tile.FAMILIES) and min(tally["families"].values()) >= 2
    assert 4 * tally["nonfinite"] >= n_cases
    assert 3 * tally["finite_mixed"] >= n_cases
    assert tally["cut"] >= 2 and tally["offset"] >= n_cases // 2
