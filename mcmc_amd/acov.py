"""Every autocovariance lag of a draws slab and Geyer's sum over a window of them: the numpy statement of what mi_mcmc_draw_stats_lags and
mi_mcmc_draw_stats_ranked_lags compute (include/mi_mcmc.h states the same), as ess.py is for the untruncated ESS.

Direct sums in float64, no FFT.  Per dimension j of a slab x[t][j][c], n x d x C, with K = min(max_lag, n - 1) (max_lag=None: every lag):
  mean    = sum_{t,c} x / (n C)
  acov_k  = sum_c sum_{t < n-k} v_t v_{t+k} / (C (n - k)),  v = x - mean,  k = 0 .. K
  R-hat   = sqrt(((n - 1) / n W + B/n) / W) when W > 0, else 1.0  (W the mean within-chain variance, B/n the variance of the chain means)
  ess     = ess_per_chain's loop over the lags [0, K]
  ended   = 1: the sum met its non-positive pair inside the window, or K = n - 1, or n < 4;  0: the window cut it.
The device centres in two parts (x - a_j) - e_j and sums in another order: it agrees with this file to roundoff (tests/draw_stats_lags_ref.py has the
bounds), and exactly in what is discrete: the shape of acov, `ended`, and where non-finite samples go."""
import numpy as np

from . import quantiles as Q
from . import rank_stats as RS

ALL_LAGS = 0xFFFFFFFF


def window(n_keep, max_lag=None):
    """K = min(max_lag, n_keep - 1)"""
    return n_keep - 1 if max_lag is None else min(int(max_lag), n_keep - 1)


def n_offsets(K):
    """ND: the block offsets delta = sb - tb whose 16 x 16 accumulators hold the lags 0 .. K (offset delta holds the lags 16 delta - 15 .. 16 delta + 15)"""
    return (K + 15) // 16 + 1


def band_plan(n_keep, K):
    """The band schedule of the host ladder, [(delta_lo, delta_hi), ..]: a function of (n_keep, K) alone.  Offsets [0, 8), [8, 16), then bands of 16, the
    last one cut at ND.  After the band [a, b) the lags 0 .. 16 (b - 1) are complete."""
    K = min(K, n_keep - 1)
    ND, lo, out = n_offsets(K), 0, []
    while lo < ND:
        hi = min(ND, lo + (8 if lo < 16 else 16))
        out.append((lo, hi))
        lo = hi
    return out


def lags_complete(band, K):
    """the number of complete lags after `band` = (lo, hi) has run (and every band before it)"""
    return min(K + 1, 16 * (band[1] - 1) + 1)


def acov_ref(draws, max_lag=None):
    """[n, d, C] -> acov [K + 1, d]"""
    x = np.asarray(draws, dtype=np.float64)
    n, d, C = x.shape
    K = window(n, max_lag)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x - x.mean(axis=(0, 2), keepdims=True)
        return np.stack([(v[: n - k] * v[k:]).sum(axis=(0, 2)) / C / (n - k) for k in range(K + 1)])


def geyer_window(acov_j, n, K):
    """ess_per_chain's loop on one dimension over the lags [0, K]: (ess, ended)"""
    if n < 4:
        return float(n), 1
    a0 = acov_j[0]
    den = a0 if a0 > 0 else 1.0
    tau, t, met = -1.0, 0, False
    while t + 1 <= K:
        pair = acov_j[t] / den + acov_j[t + 1] / den
        if pair <= 0:
            met = True
            break
        tau += 2.0 * pair
        t += 2
    ess = n / max(tau, 1.0 / n) if tau > 0 else float(n)
    return min(ess, 10.0 * n), int(met or K == n - 1)


def ess_lags_ref(draws, max_lag=None):
    """[n, d, C] -> (ess [d], ended [d] uint8)"""
    x = np.asarray(draws, dtype=np.float64)
    n, d, C = x.shape
    K = window(n, max_lag)
    ac = acov_ref(x, K)
    with np.errstate(invalid="ignore"):
        res = [geyer_window(ac[:, j], n, K) for j in range(d)]
    return np.array([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.uint8)


def draw_stats_lags_ref(draws, max_lag=None):
    """What mi_mcmc_draw_stats_lags returns, as a dict mean / acov / rhat / ess / ended"""
    x = np.asarray(draws, dtype=np.float64)
    n, d, C = x.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.mean(axis=0)
        W = x.var(axis=0, ddof=1).mean(axis=1) if n > 1 else np.zeros(d)
        B_n = m.var(axis=1, ddof=1) if C > 1 else np.zeros(d)
        rhat = np.where(W > 0, np.sqrt(((n - 1) / n * W + B_n) / np.where(W > 0, W, 1.0)), 1.0)
        mean = x.mean(axis=(0, 2))
    ess, ended = ess_lags_ref(x, max_lag)
    return dict(mean=mean, acov=acov_ref(x, max_lag), rhat=rhat, ess=ess, ended=ended)


def draw_stats_ranked_lags_ref(draws, max_lag=None):
    """What mi_mcmc_draw_stats_ranked_lags returns: rank_stats.draw_stats_ranked_ref with the ESS sums over the lags [0, K] of the half-chains,
    K = min(max_lag, h - 1), and ended = 1 only where the bulk sum and both indicator sums ended.  A dimension with a NaN among its retained samples
    is NaN throughout (ended is what the sums give)."""
    x = RS.retained(draws, True)
    z_bulk = RS.normal_scores(x)
    z_fold = RS.normal_scores(RS.folded(x))
    q05, q95 = Q.quantiles_ref(x, [0.05, 0.95])
    rb, rt = RS.rhat_classic(z_bulk), RS.rhat_classic(z_fold)
    eb, en_b = ess_lags_ref(z_bulk, max_lag)
    e05, en_05 = ess_lags_ref(RS.indicator(x, q05), max_lag)
    e95, en_95 = ess_lags_ref(RS.indicator(x, q95), max_lag)
    res = dict(rhat_bulk=rb, rhat_tail=rt, rhat=np.where(np.isnan(rb) | np.isnan(rt), np.nan, np.maximum(rb, rt)), ess_bulk=eb, ess_tail=np.minimum(e05, e95))
    bad = np.isnan(x).any(axis=(0, 2))
    for k in res:
        res[k] = np.where(bad, np.nan, res[k])
    res["ended"] = (en_b & en_05 & en_95).astype(np.uint8)
    return res
