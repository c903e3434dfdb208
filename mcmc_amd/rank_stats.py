"""Ranks, normal scores and the rank-normalised diagnostics of a draws slab: the numpy statement of what mi_mcmc_draws_rank_transform and
mi_mcmc_draw_stats_ranked compute (include/mi_mcmc.h states the same), as quantiles.py is for the order statistics.

Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021), "Rank-normalization, folding, and localization: an improved R-hat": every retained sample of
a dimension is replaced by the normal score of its average rank among the S retained samples of that dimension; the chains are split into halves;
bulk quantities come from the scores of x, the tail R-hat from the scores of |x - median|, the tail ESS from the indicators of the 5 % and 95 %
quantiles.  The order is that of quantiles.key; the normal quantile is the library's own host function (mcmc_amd.norm_ppf), so a slab made here is
the device's bit for bit."""
import numpy as np

from . import quantiles as Q
from .ess import ess_per_chain


def retained(draws, split):
    """[n_keep, d, C] -> the retained samples in the output layout: the slab itself, or with split [h, d, 2 C], h = n_keep // 2, the rows t < h in the
    columns [0, C) and the rows t >= n_keep - h in the columns [C, 2 C) (the middle row of an odd n_keep is dropped)."""
    x = np.ascontiguousarray(draws, dtype=np.float64)
    if not split:
        return x
    n = x.shape[0]
    h = n // 2
    return np.ascontiguousarray(np.concatenate([x[:h], x[n - h:]], axis=2))


def _pooled(v):
    """[rows, d, W] -> [d, rows * W]"""
    rows, d, W = v.shape
    return np.ascontiguousarray(v.transpose(1, 0, 2)).reshape(d, rows * W)


def average_ranks2(v):
    """[rows, d, W] -> R2 (uint64, same shape): twice the average 1-based rank of every sample among the S = rows * W samples of its dimension,
    R2 = lo + hi + 1 with lo the number of keys below the sample's and hi the number not above it."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    rows, d, W = v.shape
    k = Q.key(_pooled(v))
    R2 = np.empty(k.shape, dtype=np.uint64)
    for i in range(d):
        ks = np.sort(k[i])
        lo = np.searchsorted(ks, k[i], side="left")
        hi = np.searchsorted(ks, k[i], side="right")
        R2[i] = (lo + hi + 1).astype(np.uint64)
    return np.ascontiguousarray(R2.reshape(d, rows, W).transpose(1, 0, 2))


def average_ranks(v):
    """The average 1-based ranks as doubles (exact multiples of 0.5); a NaN sample comes out as the canonical quiet NaN."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = 0.5 * average_ranks2(v).astype(np.float64)
    return _nan_out(out, v)


def _nan_out(out, v):
    bits = out.view(np.uint64)
    bits[np.isnan(v)] = Q.CANONICAL_NAN_BITS
    return out


def normal_scores(v):
    """z = norm_ppf((0.5 R2 - 0.375) / (S + 0.25)) of every sample, every operation rounded once; a NaN sample: the canonical quiet NaN."""
    from . import norm_ppf
    v = np.ascontiguousarray(v, dtype=np.float64)
    S = v.shape[0] * v.shape[2]
    p = (0.5 * average_ranks2(v).astype(np.float64) - 0.375) / (np.float64(S) + 0.25)
    return _nan_out(norm_ppf(p), v)


def medians(v):
    """[rows, d, W] -> [d]: the type-7 quantile at 0.5 of every dimension's samples (quantiles.quantiles_ref's arithmetic)."""
    return Q.quantiles_ref(v, [0.5])[0]


def folded(v):
    """|v - med_i|: one subtraction, the sign cleared."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(v - medians(v)[None, :, None])


def rank_transform_ref(draws, what="normal", split=False, fold=False):
    """What mi_mcmc_draws_rank_transform writes."""
    v = retained(draws, split)
    if fold:
        v = folded(v)
    return normal_scores(v) if what in ("normal", 1) else average_ranks(v)


def indicator(v, q):
    """1{v <= q_i} as 0.0 / 1.0, a NaN sample: the canonical quiet NaN."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        out = (v <= np.asarray(q)[None, :, None]).astype(np.float64)
    return _nan_out(out, v)


def rhat_classic(x):
    """The Gelman-Rubin expression of mi_mcmc_draw_stats over the columns of [n, d, C]."""
    n = x.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x.mean(axis=0)
        W = x.var(axis=0, ddof=1).mean(axis=1)
        B_n = m.var(axis=1, ddof=1)
        return np.sqrt(((n - 1) / n * W + B_n) / W)


def draw_stats_ranked_ref(draws):
    """What mi_mcmc_draw_stats_ranked returns, as a dict of [d] arrays; the ESS values are per half-chain.  A dimension with a NaN among its retained
    samples is NaN throughout."""
    x = retained(draws, True)
    z_bulk = normal_scores(x)
    z_fold = normal_scores(folded(x))
    q05, q95 = Q.quantiles_ref(x, [0.05, 0.95])
    rb, rt = rhat_classic(z_bulk), rhat_classic(z_fold)
    res = dict(rhat_bulk=rb, rhat_tail=rt, rhat=np.where(np.isnan(rb) | np.isnan(rt), np.nan, np.maximum(rb, rt)),
               ess_bulk=ess_per_chain(z_bulk), ess_tail=np.minimum(ess_per_chain(indicator(x, q05)), ess_per_chain(indicator(x, q95))))
    bad = np.isnan(x).any(axis=(0, 2))
    for k in res:
        res[k] = np.where(bad, np.nan, res[k])
    return res
