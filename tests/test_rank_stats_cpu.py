"""No GPU: the host side of mi_mcmc_draws_rank_transform / mi_mcmc_draw_stats_ranked -- the normal quantile (mi_mcmc_norm_ppf: one function for the
host and the device), mcmc_amd/rank_stats.py (the numpy statement the device result is held to bit for bit), the argument checks (MI_ERR_BAD_ARG even
where no device is visible) and the arithmetic of the group rule.

norm_ppf is AS 241 PPND16 with CPython's coefficients and nesting, so statistics.NormalDist().inv_cdf is the same algorithm in CPython's arithmetic:
 * |p - 0.5| <= 0.425 involves no logarithm: BITWISE;
 * in the tails the only difference is the engine's det_log against libm's log.  MEASURED on the CPU over the grid p = 10^-k 10^(j/32), k = 1..300,
   j = 0..31 (9 566 points beyond the centre) and the mirrored 1 - p where that is below 1 (486 points): the largest relative difference is
   2.61e-16 (1.17 eps; 5 in 10 000 points differ at all).  The test asserts 8 x that: the grid is a sample, the margin covers the points between.
 * independently of CPython, 0.5 erfc(-z / sqrt 2) returns to p within 4 ulp(p) + 1e-16 for p >= 1e-300 (measured worst: 0.71 of that bound, and
   the same 0.71 for CPython's own function)."""
import math
import statistics

import numpy as np
import pytest

import mcmc_amd
from mcmc_amd import quantiles as Q
from mcmc_amd import rank_stats as R

_INV = statistics.NormalDist().inv_cdf
TAIL_MEASURED = 2.61e-16                    # see the docstring
EPS = np.finfo(float).eps


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _centre_points():
    rng = np.random.default_rng(241)
    lo, hi = 0.075, 0.925
    while abs(lo - 0.5) > 0.425:            # the branch edges: the outermost doubles the central branch takes
        lo = np.nextafter(lo, 1.0)
    while abs(hi - 0.5) > 0.425:
        hi = np.nextafter(hi, 0.0)
    assert abs(np.nextafter(lo, 0.0) - 0.5) > 0.425 or lo == 0.075
    p = rng.uniform(lo, hi, 10 ** 4 - 3)
    p = np.concatenate([p, [0.5, lo, hi]])
    assert (np.abs(p - 0.5) <= 0.425).all() and p.size == 10 ** 4
    return p


def _tail_points():
    k = np.arange(1, 301, dtype=np.float64)[:, None]
    u = 10.0 ** (np.arange(32) / 32.0)[None, :]
    pt = (10.0 ** -k * u).ravel()
    pt = pt[(pt > 0.0) & (np.abs(pt - 0.5) > 0.425)]
    pm = 1.0 - pt
    pm = pm[(pm < 1.0) & (np.abs(pm - 0.5) > 0.425)]
    return np.concatenate([pt, pm])


def test_norm_ppf_is_cpythons_inv_cdf_bit_for_bit_in_the_centre():
    p = _centre_points()
    z = mcmc_amd.norm_ppf(p)
    assert np.array_equal(_bits(z), _bits([_INV(float(v)) for v in p]))
    assert _bits(mcmc_amd.norm_ppf([0.5]))[0] == 0                                       # +0.0


def test_norm_ppf_tails_differ_from_cpython_by_the_logarithm_only():
    p = _tail_points()
    z = mcmc_amd.norm_ppf(p)
    ref = np.array([_INV(float(v)) for v in p])
    rel = np.abs(z - ref) / np.abs(ref)
    print(f"tails: {p.size} points, worst relative difference {rel.max():.3e} = {rel.max() / EPS:.2f} eps, {np.count_nonzero(rel)} differ")
    assert rel.max() <= 8.0 * TAIL_MEASURED
    assert np.array_equal(np.sign(z), np.sign(ref)) and np.isfinite(z).all()


def test_norm_ppf_inverts_the_normal_cdf():
    p = np.concatenate([_centre_points()[::5], _tail_points()])
    p = p[p >= 1e-300]
    z = mcmc_amd.norm_ppf(p)
    worst = 0.0
    for pv, zv in zip(p.tolist(), z.tolist()):
        worst = max(worst, abs(0.5 * math.erfc(-zv / math.sqrt(2.0)) - pv) / (4.0 * math.ulp(pv) + 1e-16))
    print(f"worst |Phi(z) - p| = {worst:.3f} of 4 ulp(p) + 1e-16")
    assert worst <= 1.0


def test_norm_ppf_has_one_rule_outside_the_open_interval():
    z = mcmc_amd.norm_ppf([0.0, -0.0, -1.0, -np.inf, 1.0, 2.0, np.inf, np.nan, 5e-324, 1.0 - 2.0 ** -53])
    assert np.array_equal(z[:4], [-np.inf] * 4) and np.array_equal(z[4:7], [np.inf] * 3) and np.isnan(z[7])
    assert np.isfinite(z[8:]).all() and z[8] < -38.0 and z[9] > 8.0
    assert mcmc_amd.norm_ppf(np.zeros((0,))).size == 0


# ---- rank_stats.py

def test_ranks_of_a_permutation_are_1_to_S():
    rng = np.random.default_rng(0)
    v = rng.permutation(7 * 11).astype(np.float64).reshape(7, 1, 11) - 30.0
    r = R.average_ranks(v)
    assert np.array_equal(np.sort(r.ravel()), np.arange(1, 78))
    assert np.array_equal(r, v + 31.0)                                                   # the value k - 30 has rank k + 1


def test_ties_share_the_mean_rank_and_the_sum_is_fixed():
    v = np.array([3.0, 1.0, 3.0, 2.0, 3.0, 1.0]).reshape(2, 1, 3)
    assert np.array_equal(R.average_ranks(v).ravel(), [5.0, 1.5, 5.0, 3.0, 5.0, 1.5])
    rng = np.random.default_rng(1)
    for shape in [(5, 3, 7), (1, 2, 1), (4, 1, 50)]:
        w = rng.integers(-2, 3, size=shape).astype(np.float64)
        S = shape[0] * shape[2]
        assert (R.average_ranks2(w).sum(axis=(0, 2)) == S * (S + 1)).all()              # sum of R2 = S (S + 1) whatever the ties
    c = np.full((3, 2, 5), 7.25)
    assert (R.average_ranks(c) == 8.0).all()                                             # (S + 1) / 2
    assert (_bits(R.normal_scores(c)) == 0).all()                                        # p = 0.5 exactly, z = +0.0


def test_minus_zero_ranks_below_plus_zero():
    v = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]).reshape(1, 1, 6)
    assert np.array_equal(R.average_ranks(v).ravel(), [4.5, 2.5, 4.5, 2.5, 6.0, 1.0])


def test_nans_rank_on_top_and_come_out_nan():
    neg_payload = np.array([0xFFF0000000000123], dtype=np.uint64).view(np.float64)[0]
    v = np.array([1.0, np.nan, np.inf, neg_payload, -np.inf, 2.0]).reshape(1, 1, 6)
    assert np.array_equal(R.average_ranks2(v).ravel(), [4, 11, 8, 11, 2, 6])             # the two NaNs share the ranks 5 and 6
    for f in (R.average_ranks, R.normal_scores):
        out = f(v).ravel()
        assert (_bits(out)[[1, 3]] == Q.CANONICAL_NAN_BITS).all() and np.isfinite(out[[0, 2, 4, 5]]).all()
    assert np.array_equal(R.average_ranks(v).ravel()[[0, 2, 4, 5]], [2.0, 4.0, 1.0, 3.0])


def test_retained_drops_the_middle_row_and_puts_the_second_halves_behind():
    x = np.arange(7 * 2 * 3, dtype=np.float64).reshape(7, 2, 3)
    assert R.retained(x, False) is x or np.array_equal(R.retained(x, False), x)
    s = R.retained(x, True)
    assert s.shape == (3, 2, 6)
    assert np.array_equal(s[:, :, :3], x[:3]) and np.array_equal(s[:, :, 3:], x[4:])      # row 3, the middle one, is not there
    e = R.retained(x[:6], True)
    assert np.array_equal(e[:, :, :3], x[:3]) and np.array_equal(e[:, :, 3:], x[3:6])


def test_normal_scores_are_the_blom_scores_and_fold_is_about_the_median():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((6, 2, 9))
    z = R.normal_scores(x)
    S = 54
    want = mcmc_amd.norm_ppf((R.average_ranks(x) - 0.375) / (S + 0.25))
    assert np.array_equal(_bits(z), _bits(want))
    assert abs(z.sum()) < 1e-12 and np.array_equal(np.argsort(z[:, 0].ravel()), np.argsort(x[:, 0].ravel()))
    o = x[:5]                                                                            # S = 45, odd: the median is a sample, no arithmetic
    assert np.array_equal(R.folded(o), np.abs(o - np.median(o.transpose(1, 0, 2).reshape(2, -1), axis=1)[None, :, None]))
    assert np.array_equal(_bits(R.rank_transform_ref(x, "average", split=True, fold=True)), _bits(R.average_ranks(R.folded(R.retained(x, True)))))


def test_the_reference_diagnostics_see_what_the_classic_ones_miss():
    """The issue's table, on the numpy reference alone (the device comparison: tests/test_gpu_draw_stats_ranked.py)."""
    x = np.random.default_rng(0).standard_normal((41, 2, 130))
    a = x.copy()
    a[:, 1, :65] *= 3
    assert R.rhat_classic(a)[1] < 1.01 and R.draw_stats_ranked_ref(a)["rhat_tail"][1] > 1.05
    w = x.copy()
    w[:20, 0, :] += 1
    assert R.rhat_classic(w)[0] < 1.01 and R.draw_stats_ranked_ref(w)["rhat_bulk"][0] > 1.05
    n = x.copy()
    n[3, 0, 7] = np.nan
    got, clean = R.draw_stats_ranked_ref(n), R.draw_stats_ranked_ref(x)
    for k in got:
        assert np.isnan(got[k][0]) and got[k][1] == clean[k][1]


# ---- argument checks: MI_ERR_BAD_ARG before any device call

_X = np.zeros((4, 3, 5))
_OUT = np.zeros((4, 3, 5))
_D5 = [np.zeros(3) for _ in range(5)]


def _rc_transform(slab=_X.ctypes.data, n_keep=4, d=3, n_chains=5, what=1, flags=0, out=_OUT.ctypes.data):
    return mcmc_amd.lib().mi_mcmc_draws_rank_transform(slab, mcmc_amd.MEM_HOST, n_keep, d, n_chains,
                                                       what, flags, out, None)


def _rc_stats(slab=_X.ctypes.data, n_keep=4, d=3, n_chains=5, outs=None):
    outs = [o.ctypes.data for o in _D5] if outs is None else outs
    return mcmc_amd.lib().mi_mcmc_draw_stats_ranked(slab, mcmc_amd.MEM_HOST, n_keep, d, n_chains,
                                                    *[o for o in outs], None)


_SHARED = {"null_slab": (dict(slab=None), "slab"), "d_is_0": (dict(d=0), "d "), "d_past_65536": (dict(d=65537), "d = 65537"),
           "n_keep_past_32_bits": (dict(n_keep=1 << 32), "n_keep"), "n_chains_past_32_bits": (dict(n_chains=1 << 32), "n_chains"),
           "S_is_0_chains": (dict(n_chains=0), "S = 0"), "S_is_2_to_32": (dict(n_keep=1 << 16, n_chains=1 << 16), "2^32")}
_TRANSFORM = dict(_SHARED, null_out=(dict(out=None), "out"), S_is_0_keep=(dict(n_keep=0), "S = 0"), what_is_2=(dict(what=2), "what"),
                  what_is_minus_1=(dict(what=-1), "what"), flag_bit_4=(dict(flags=4), "flag"), flag_bit_31=(dict(flags=(1 << 31) | 1), "flag"),
                  split_of_one_draw=(dict(n_keep=1, flags=1), "MI_RANK_SPLIT"), split_of_no_draw=(dict(n_keep=0, flags=3), "MI_RANK_SPLIT"))
_STATS = dict(_SHARED, all_outputs_null=(dict(outs=[None] * 5), "NULL"), n_keep_is_3=(dict(n_keep=3), "n_keep = 3"), n_keep_is_2=(dict(n_keep=2), "n_keep = 2"),
              n_keep_is_0=(dict(n_keep=0), "n_keep"))


@pytest.mark.parametrize("case", sorted(_TRANSFORM))
def test_rank_transform_rejects_bad_arguments_without_a_gpu(case):
    kw, names = _TRANSFORM[case]
    assert _rc_transform(**kw) == mcmc_amd.MI_ERR_BAD_ARG
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_rank_transform:") and names in msg, msg


@pytest.mark.parametrize("case", sorted(_STATS))
def test_draw_stats_ranked_rejects_bad_arguments_without_a_gpu(case):
    kw, names = _STATS[case]
    assert _rc_stats(**kw) == mcmc_amd.MI_ERR_BAD_ARG
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draw_stats_ranked:") and names in msg, msg


def test_front_ends_raise_and_the_entries_are_exported():
    for name in ("mi_mcmc_draws_rank_transform", "mi_mcmc_draw_stats_ranked", "mi_mcmc_norm_ppf"):
        assert name in mcmc_amd.EXPORTS and hasattr(mcmc_amd.lib(), name)
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_rank_transform(np.zeros((1, 2, 3)), split=True)
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draw_stats_ranked(np.zeros((3, 2, 3)))
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(ValueError):
        mcmc_amd.draws_rank_transform(_X, what="median")
    hdr = open(mcmc_amd.LIB_PATH.replace("libmi_mcmc.so", "csrc/mi_mcmc_probes.h")).read()
    for name in ("mi_mcmc_test_set_rank_ws_bytes", "mi_mcmc_test_rank_dim_bytes", "mi_mcmc_test_rank_dims_per_group", "mi_mcmc_test_rank_counts"):
        assert name in hdr and hasattr(mcmc_amd.lib(), name)


# ---- the group rule (draws_rank.hpp), as host arithmetic

def _dim_bytes(n_keep, C_, flags, stats):
    return mcmc_amd.lib().mi_mcmc_test_rank_dim_bytes(n_keep, C_, flags, stats)


def _dims_per_group(n_keep, d, C_, flags, stats):
    return mcmc_amd.lib().mi_mcmc_test_rank_dims_per_group(n_keep, d, C_, flags, stats)


def _set_budget(b):
    mcmc_amd.lib().mi_mcmc_test_set_rank_ws_bytes(b)


def test_the_group_rule():
    TILE = 16384
    for n_keep, C_, flags, stats in [(7, 45, 0, 0), (7, 45, 1, 0), (7, 45, 1, 1), (9, 40003, 0, 0), (9, 40003, 3, 0), (100, 65536, 1, 1)]:
        rows = 2 * (n_keep // 2) if flags & 1 else n_keep
        S = rows * C_
        tiles = -(-S // TILE)
        want = 16 * S + 1024 * tiles + 8192 + (8 * S if stats else 0)
        assert _dim_bytes(n_keep, C_, flags, stats) == want
    try:
        _set_budget(0)
        assert _dims_per_group(7, 5, 45, 0, 0) == 5                                      # the real budget holds all five
        assert _dims_per_group(100, 128, 65536, 1, 1) == (2 << 30) // _dim_bytes(100, 65536, 1, 1)
        assert _dims_per_group(2, 65536, 1, 0, 0) == 65536
        b = _dim_bytes(7, 45, 0, 0)
        _set_budget(2 * b)
        dpg = _dims_per_group(7, 5, 45, 0, 0)
        assert dpg == 2 and [min(dpg, 5 - s) for s in range(0, 5, dpg)] == [2, 2, 1]
        _set_budget(3 * b - 1)
        assert _dims_per_group(7, 5, 45, 0, 0) == 2
        _set_budget(b - 1)
        assert _dims_per_group(7, 5, 45, 0, 0) == 1                                      # never fewer than one dimension
        _set_budget(1 << 62)
        assert _dims_per_group(7, 5, 45, 0, 0) == 5                                      # more than the real budget: the real budget
    finally:
        _set_budget(0)
