"""No GPU: mi_mcmc_draws_order_stats / mi_mcmc_draws_quantiles reject bad arguments before any device call (MI_ERR_BAD_ARG even where no device is
visible -- a call that reached the device probe would answer MI_ERR_NO_DEVICE there), and mcmc_amd/quantiles.py, the numpy statement the device result
is held to bit for bit, is itself checked against np.sort and np.quantile.

The bound of the np.quantile comparison is derived, not fitted: numpy computes the same type-7 quantile by another formula of at most three
roundings, ours has three (the difference, the product, the sum), each on a magnitude of at most 2 max(|x_lo|, |x_hi|): 6 eps max(|x_lo|, |x_hi|).  It
is asked only where 0 < g < 1 on finite data; at g = 0 the rule `x_lo` is the definition (numpy's lerp gives NaN next to an infinity there)."""

import numpy as np
import pytest

import mcmc_amd
from mcmc_amd import quantiles as Q

_X = np.zeros((2, 3, 4))                  # K = 8
_RANKS = np.array([0, 7], dtype=np.uint64)
_PROBS = np.array([0.0, 0.5])
_OUT = np.zeros((2, 3))


def _rc(fn, slab=_X.ctypes.data, n_keep=2, d=3, n_chains=4, sel=None, n_sel=2, out=_OUT.ctypes.data):
    if sel is None:
        sel = (_RANKS if fn == "order_stats" else _PROBS).ctypes.data
    f = getattr(mcmc_amd.lib(), "mi_mcmc_draws_" + ("order_stats" if fn == "order_stats" else "quantiles"))
    return f(slab, mcmc_amd.MEM_HOST, n_keep, d, n_chains, sel, n_sel, out, None)


_SHARED = {"null_slab": (dict(slab=None), "slab"), "null_out": (dict(out=None), "out"), "d_is_0": (dict(d=0), "d "),
           "K_is_0_keep": (dict(n_keep=0), "K "), "K_is_0_chains": (dict(n_chains=0), "K "), "n_keep_past_32_bits": (dict(n_keep=1 << 32), "n_keep"),
           "n_chains_past_32_bits": (dict(n_chains=1 << 32), "n_chains"), "d_past_65536": (dict(d=65537), "d = 65537")}
_BIG_RANKS = np.zeros(33, dtype=np.uint64)
_BAD_RANK = np.array([0, 8], dtype=np.uint64)
_BIG_PROBS = np.full(17, 0.5)
_ORDER = dict(_SHARED, null_ranks=(dict(sel=0), "ranks"), n_ranks_is_0=(dict(n_sel=0), "n_ranks"),
              n_ranks_is_33=(dict(sel=_BIG_RANKS.ctypes.data, n_sel=33), "n_ranks"), rank_is_K=(dict(sel=_BAD_RANK.ctypes.data), "ranks[1]"))
_BAD_PROBS = {"prob_below_0": np.array([0.5, -1e-300]), "prob_above_1": np.array([0.5, np.nextafter(1.0, 2.0)]), "prob_nan": np.array([0.5, np.nan])}
_QUANT = dict(_SHARED, null_probs=(dict(sel=0), "probs"), n_probs_is_0=(dict(n_sel=0), "n_probs"),
              n_probs_is_17=(dict(sel=_BIG_PROBS.ctypes.data, n_sel=17), "n_probs"),
              **{k: (dict(sel=v.ctypes.data), "probs[1]") for k, v in _BAD_PROBS.items()})


@pytest.mark.parametrize("case", sorted(_ORDER))
def test_order_stats_rejects_bad_arguments_without_a_gpu(case):
    kw, names = _ORDER[case]
    assert _rc("order_stats", **kw) == mcmc_amd.MI_ERR_BAD_ARG
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_order_stats:") and names in msg, msg


@pytest.mark.parametrize("case", sorted(_QUANT))
def test_quantiles_rejects_bad_arguments_without_a_gpu(case):
    kw, names = _QUANT[case]
    assert _rc("quantiles", **kw) == mcmc_amd.MI_ERR_BAD_ARG
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_quantiles:") and names in msg, msg


def test_front_ends_raise_and_the_entries_are_exported():
    for name in ("mi_mcmc_draws_order_stats", "mi_mcmc_draws_quantiles"):
        assert name in mcmc_amd.EXPORTS and hasattr(mcmc_amd.lib(), name)
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_order_stats(_X, [8])
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_quantiles(_X, [1.5])
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_quantiles(_X, [])
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG


SHAPES = [(1, 1, 1), (7, 3, 45), (5, 130, 130), (3, 17, 257), (100, 4, 1000)]


def _slab(shape, with_inf=False):
    n, d, C = shape
    rng = np.random.default_rng(n * 1000003 + d * 1009 + C)
    slab = rng.standard_normal(shape) * np.exp(rng.uniform(-20.0, 20.0, (1, d, 1)))
    if with_inf:
        flat = slab.reshape(-1)
        idx = rng.permutation(flat.size)[: max(2, flat.size // 10)]
        flat[idx[::2]] = np.inf
        flat[idx[1::2]] = -np.inf
    return slab


def _ranks(K):
    return sorted({0, K - 1, K // 2, K // 3})


@pytest.mark.parametrize("with_inf", [False, True], ids=["finite", "with_inf"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_order_stats_ref_is_np_sort_on_the_value_level(shape, with_inf):
    n, d, C = shape
    slab = _slab(shape, with_inf)
    ranks = _ranks(n * C)
    x = slab.transpose(1, 0, 2).reshape(d, n * C)
    assert np.array_equal(Q.order_stats_ref(slab, ranks), np.sort(x, axis=1)[:, ranks].T)
    assert np.array_equal(Q.order_stats_ref(slab, ranks[::-1] + ranks[:1]), np.sort(x, axis=1)[:, ranks[::-1] + ranks[:1]].T)     # unsorted, repeated


def test_key_orders_the_specials_and_inverts_exactly():
    nan_neg_payload = np.array([0xFFF0000000000123], dtype=np.uint64).view(np.float64)[0]
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, nan_neg_payload, 5e-324, -5e-324, 1.0, 1.0 + 2.0 ** -52, 1.0, -1.0, 1.7976931348623157e308])
    o = Q.order_stats_ref(x.reshape(1, 1, -1), np.arange(x.size))[:, 0]
    want = np.array([-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.0, 1.0 + 2.0 ** -52, 1.7976931348623157e308, np.inf, np.nan, np.nan])
    assert np.array_equal(o.view(np.uint64), want.view(np.uint64)[:-2].tolist() + [0x7FF8000000000000] * 2)
    assert np.signbit(o[3]) and not np.signbit(o[4])                                     # -0.0 before +0.0
    k = Q.key(x)
    assert (k[4] == Q.KEY_NAN) and (k[5] == Q.KEY_NAN) and (np.sort(k)[-3] == Q.key(np.array([np.inf]))[0])
    finite = x[~np.isnan(x)]
    assert np.array_equal(Q.unkey(Q.key(finite)).view(np.uint64), finite.view(np.uint64))          # key is a bijection off the NaNs


def test_order_stats_ref_returns_the_canonical_nan_bits():
    rng = np.random.default_rng(5)
    slab = rng.standard_normal((3, 2, 50))
    bits = slab.view(np.uint64)
    bits[0, 0, :10] = 0x7FF0000000000001 + np.arange(10, dtype=np.uint64)               # signalling, positive
    bits[1, 0, :5] = 0xFFF8000000000000 + np.arange(5, dtype=np.uint64)                 # quiet, negative
    o = Q.order_stats_ref(slab, [134, 135, 149])
    assert np.array_equal(o[:, 0].view(np.uint64), [np.sort(slab[:, 0][~np.isnan(slab[:, 0])])[-1:].view(np.uint64)[0], 0x7FF8000000000000, 0x7FF8000000000000])
    assert np.isfinite(o[:, 1]).all()


PROBS = [0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.95, 0.999, 1.0]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quantiles_ref_agrees_with_np_quantile_within_the_derived_bound(shape):
    n, d, C = shape
    K = n * C
    slab = _slab(shape)
    x = slab.transpose(1, 0, 2).reshape(d, K)
    q = Q.quantiles_ref(slab, PROBS)
    ref = np.quantile(x, PROBS, axis=1, method="linear")
    s = np.sort(x, axis=1)
    worst = 0.0
    for a, p in enumerate(PROBS):
        lo, hi, g = Q.quantile_ranks(K, p)
        if g == 0.0:
            assert np.array_equal(q[a], s[:, lo])                                        # the pinned rule
            continue
        mag = np.maximum(np.abs(s[:, lo]), np.abs(s[:, hi]))
        worst = max(worst, float((np.abs(q[a] - ref[a]) / (np.finfo(float).eps * mag)).max()))
        assert (np.abs(q[a] - ref[a]) <= 6.0 * np.finfo(float).eps * mag).all()
    print(f"{shape}: worst |quantiles_ref - np.quantile| = {worst:.3f} eps max(|x_lo|, |x_hi|)")


def test_quantiles_ref_propagates_non_finite_samples_through_the_one_expression():
    slab = np.array([-np.inf, 1.0, 2.0, np.inf, np.nan]).reshape(1, 1, 5)              # K - 1 = 4
    q = Q.quantiles_ref(slab, [0.0, 0.25, 0.5, 0.75, 1.0, 0.125, 0.6, 0.8])[:, 0]
    assert np.array_equal(q[:5].view(np.uint64), np.array([-np.inf, 1.0, 2.0, np.inf, np.nan]).view(np.uint64))
    assert np.isnan(q[5]) and q[6] == np.inf and np.isnan(q[7])                          # -inf + g (1 + inf) ; 2 + g inf ; inf + g (nan - inf)
