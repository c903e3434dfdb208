"""GPU: the device's deterministic math, Philox + Box-Muller generator and fp64 MFMA tile on the edge tables of tests/math_edges.py, held to the CPU
oracle (the tile: to the exact fma chain) bit for bit.  Outputs are compared as uint64; any NaN matches any NaN.  No tolerance anywhere.  Every math
table runs through both builds of det_math.hpp: MI_KC_MODE 1 (probes.hip) and MI_KC_MODE 2 with MI_RNG_NOINLINE (probes_kc2.hip, the logistic units)."""
import numpy as np
import pytest

import math_edges as me
import mcmc_amd
import orc

pytestmark = pytest.mark.gpu

KC2 = pytest.mark.parametrize("kc2", [False, True], ids=["kc1", "kc2"])


def _assert_same(a, b, what):
    """bitwise; any NaN matches any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    assert a.shape == b.shape, what
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.uint64) != b.view(np.uint64)))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {a.size} differ; first at {i}: device {a[i]!r} ({a[i].hex()}), reference {b[i]!r} ({b[i].hex()})")


TABLES = [(0, "exp", me.exp_table), (1, "log", me.log_table), (2, "sincos2pi", me.sincos_table), (3, "softplus", me.logistic_table),
          (4, "sigmoid", me.logistic_table), (5, "norm_ppf", me.norm_ppf_table)]


@KC2
@pytest.mark.parametrize("fn,name,table", TABLES, ids=[t[1] for t in TABLES])
def test_math_table_matches_oracle_bitwise(fn, name, table, kc2):
    x = table()
    g1, g2 = mcmc_amd.probe_math(fn, x, kc2=kc2)
    o1, o2 = orc.math_eval(fn, x)
    _assert_same(g1, o1, name)
    if fn == 2:
        _assert_same(g2, o2, name + " (cos)")


@KC2
def test_pow_table_matches_oracle_bitwise(kc2):
    x, y = me.pow_table()
    _assert_same(mcmc_amd.probe_math2(0, x, y, kc2=kc2), orc.math_eval(6, x, y)[0], "pow")


def test_unknown_function_codes_give_nan_not_garbage():
    x = np.array([0.5, 1.0])
    assert np.isnan(mcmc_amd.probe_math(6, x)[0]).all() and np.isnan(mcmc_amd.probe_math(6, x, kc2=True)[0]).all()
    assert np.isnan(mcmc_amd.probe_math2(1, x, x)).all() and np.isnan(mcmc_amd.probe_math2(1, x, x, kc2=True)).all()


VARIANTS = ["pair", "pair_at", "two_pairs", "four_pairs"]


@pytest.mark.parametrize("case", me.rng_cases(), ids=lambda c: "-".join(hex(v) for v in c))
def test_normals_every_variant_matches_oracle_bitwise(case):
    seed, chain, draw, stream, d = case
    ref = orc.normal_vec(seed, chain, draw, stream, d)
    _assert_same(mcmc_amd.probe_normals(seed, chain, draw, stream, d), ref, "mi_probe_normals")
    for kc2 in (False, True):
        for v, name in enumerate(VARIANTS):
            _assert_same(mcmc_amd.probe_normals_variant(v, seed, chain, draw, stream, d, kc2=kc2), ref, f"rng_normal_{name}, kc2={kc2}")


def test_normals_probe_refuses_bad_arguments():
    for kc2 in (False, True):
        for variant, d in ((4, 8), (-1, 8), (0, 0)):
            with pytest.raises(mcmc_amd.MiMcmcError):
                mcmc_amd.probe_normals_variant(variant, 1, 0, 0, 0, d, kc2=kc2)


def test_uniform_extremes_match_oracle_bitwise():
    for args in me.uniform_cases():
        g, o = mcmc_amd.probe_uniform(*args), orc.uniform(*args)
        assert g == o and 0.0 < g < 1.0, args


_TILES = me.mfma_tiles()


@pytest.mark.parametrize("name", list(_TILES))
def test_mfma_tile_is_the_exact_fma_chain(name):
    A, B, C = _TILES[name]
    _assert_same(mcmc_amd.probe_mfma(A, B, C), me.mfma_reference(A, B, C), name)
