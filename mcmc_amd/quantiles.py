"""Pooled order statistics and quantiles of a draws slab: the numpy statement of what mi_mcmc_draws_order_stats and mi_mcmc_draws_quantiles
compute (include/mi_mcmc.h states the same), as ess.py is for mi_mcmc_draw_stats.

The samples of dimension i of a slab [n_keep, d, C] are its K = n_keep * C values, pooled over draws and chains.  They are ordered by a 64-bit
key: -inf < negatives < -0.0 < +0.0 < positives < +inf < NaN, numpy's sort order with the sign of zero made definite; every NaN has one key and
comes back as the canonical quiet NaN.  The device result is held to these functions bit for bit."""
import numpy as np

KEY_NAN = np.uint64(0xFFFFFFFFFFFFFFFF)
CANONICAL_NAN_BITS = np.uint64(0x7FF8000000000000)
_TOP = np.uint64(1 << 63)


def key(x):
    """float64 array -> uint64 keys of the same shape."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    u = x.view(np.uint64)
    k = np.where((u >> np.uint64(63)) == 1, ~u, u | _TOP)
    k[np.isnan(x)] = KEY_NAN
    return k


def unkey(k):
    """The inverse of key(): uint64 keys -> float64 values (the NaN key: the canonical quiet NaN)."""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    u = np.where((k >> np.uint64(63)) == 1, k & ~_TOP, ~k)
    u[k == KEY_NAN] = CANONICAL_NAN_BITS
    return u.view(np.float64)


def sorted_keys(draws):
    """[n_keep, d, C] -> the ascending keys [d, K] of every dimension."""
    x = np.ascontiguousarray(draws, dtype=np.float64)
    n, d, C = x.shape
    return np.sort(key(np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(d, n * C)), axis=1)


def order_stats_ref(draws, ranks, keys_sorted=None):
    """out[a, i]: the value whose key is the ranks[a]-th smallest (0-based) of dimension i's K keys.  ranks may be unsorted and may repeat.
    keys_sorted: sorted_keys(draws), where a caller has it already."""
    ks = sorted_keys(draws) if keys_sorted is None else keys_sorted
    ranks = np.asarray(ranks, dtype=np.int64)
    return unkey(np.ascontiguousarray(ks[:, ranks].T))


def quantile_ranks(K, p):
    """(lo, hi, g) of the type-7 rule for one probability: h = p (K - 1), lo = floor(h), g = h - lo, hi = min(lo + 1, K - 1)."""
    h = float(p) * float(K - 1)
    lo = min(int(np.floor(h)), K - 1)
    g = h - float(lo)
    return lo, min(lo + 1, K - 1), g


def quantiles_ref(draws, probs, keys_sorted=None):
    """out[a, i]: the Hyndman-Fan type-7 quantile (numpy's method="linear") of dimension i at probs[a], from two order statistics:
    q = x_lo if g == 0 else x_lo + g * (x_hi - x_lo), every operation rounded once."""
    x = np.asarray(draws)
    n, d, C = x.shape
    K = n * C
    ks = sorted_keys(draws) if keys_sorted is None else keys_sorted
    out = np.empty((len(probs), d))
    for a, p in enumerate(probs):
        lo, hi, g = quantile_ranks(K, p)
        x_lo, x_hi = order_stats_ref(draws, [lo, hi], ks)
        if g == 0.0:
            out[a] = x_lo
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                out[a] = x_lo + np.float64(g) * (x_hi - x_lo)
    return out
