"""Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO) and the Pareto k diagnostic of a draws slab: the numpy statement of what
mi_mcmc_draws_psis_loo computes (include/mi_mcmc.h states the same, orders and constants included), as waic.py is for mi_mcmc_draws_waic.

ll[r, k] is the pointwise log-likelihood of observation r at sample k (waic.waic_ref(...)["loglik"]).  Per row the K values are sorted ascending by the
64-bit key of quantiles.py, s_0 <= ... <= s_{K-1}; the importance ratios of leaving r out are exp(-ll), so the LARGEST ratios are the FIRST sorted
values and lw_i = s_0 - s_i <= 0 are the log-ratios relative to the largest.  The M = tail_length(K) largest ratios are replaced by the order
statistics of a generalised Pareto distribution fitted to them (Zhang and Stephens 2009; Vehtari, Simpson, Gelman, Yao and Gabry 2024), truncated at
the largest raw ratio; elpd_loo_r is the log of the self-normalised estimate and pareto_k_r the fitted shape.  Everything is a function of the sorted
row, hence of the multiset of its values.

This module never looks at the library.  Every elementary operation is one IEEE fp64 operation of numpy, rounded once; exp and log come in through
`math` as in waic.py.  The device result is held to these functions bit for bit where `math` is the library's arithmetic (tests: the CPU oracle's).

THE SUMS.  SUM(v_0 .. v_{n-1}) below is ONE order, that of a workgroup of 256 threads: slot t (t < 256) takes v_t, v_{t+256}, ... ascending from +0;
the 256 slots meet as u[i] = u[i] + u[i + 128] (i < 128), then + u[i + 64] (i < 64), ... + u[i + 1].  The body fold cuts its K - M values into pieces
of BODY_PIECE, takes SUM of each and adds the pieces ascending from +0.  The sums over the m fit points (l and j) are plain, ascending from +0."""
import math as _pymath

import numpy as np

from . import quantiles, waic

SLOTS = 256                         # running sums of SUM
BODY_PIECE = 16384                  # values of one piece of the body fold
LOG_MIN_NORMAL = -708.3964185322641  # log of the smallest normal double
W_MIN = 10.0 * 2.0 ** -52           # fit weights below this are dropped
K_MIN = 25                          # below it the tail has fewer than five values
K_BAD = 0.7


def tail_length(K):
    """M = min(K div 5, m3), m3 the smallest integer with m3 * m3 >= 9 K  (= ceil(3 sqrt(K)), in integers)."""
    K = int(K)
    m3 = _pymath.isqrt(9 * K - 1) + 1
    return min(K // 5, m3)


def fit_points(M):
    """m = 30 + floor(sqrt(M)), in integers."""
    return 30 + _pymath.isqrt(int(M))


def _f(math, name, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.asarray(waic._m(math, name)(a.ravel()), dtype=np.float64).reshape(a.shape)


def tree_sum(v):
    """SUM over the last axis: [..., n] -> [...]."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[-1]
    q = (n + SLOTS - 1) // SLOTS
    pad = np.zeros(v.shape[:-1] + (q * SLOTS,))       # + 0.0 leaves a running sum that started from +0 as it is
    pad[..., :n] = v
    pad = pad.reshape(v.shape[:-1] + (q, SLOTS))
    u = np.zeros(v.shape[:-1] + (SLOTS,))
    for i in range(q):
        u = u + pad[..., i, :]
    h = SLOTS // 2
    while h >= 1:
        u = u[..., :h] + u[..., h:2 * h]
        h //= 2
    return u[..., 0]


def psis_rows(ll, math=waic.NUMPY_MATH):
    """(elpd_loo [R], pareto_k [R]) of ll [R, K], K >= 25."""
    ll = np.ascontiguousarray(ll, dtype=np.float64)
    R = ll.shape[0]
    ll = ll.reshape(R, -1)
    K = ll.shape[1]
    if K < K_MIN:
        raise ValueError("at least 25 samples are needed")
    M = tail_length(K)
    m = fit_points(M)
    n = np.float64(M)
    s = quantiles.unkey(np.sort(quantiles.key(ll), axis=1))
    with np.errstate(all="ignore"):
        s0 = s[:, 0]
        bad = ~(np.isfinite(s0) & np.isfinite(s[:, K - 1]))
        dcut = s0 - s[:, M]
        cut = np.where(dcut > LOG_MIN_NORMAL, dcut, LOG_MIN_NORMAL)
        ec = _f(math, "exp", cut)
        st = np.ascontiguousarray(s[:, :M][:, ::-1])                      # st[:, j - 1] = s_{M - j}, j = 1 .. M
        raw = s0[:, None] - st                                             # the raw log-ratios of the tail, ascending
        x = _f(math, "exp", raw) - ec[:, None]                            # the exceedances, ascending
        q = x[:, (M + 2) // 4 - 1]                                         # x_{floor(M / 4 + 0.5)}
        xM = x[:, M - 1]
        # the fit
        jj = np.arange(1, m + 1, dtype=np.float64)
        root = 1.0 - np.sqrt(np.float64(m) / (jj - 0.5))
        b = root[None, :] / (3.0 * q)[:, None] + (1.0 / xM)[:, None]      # [R, m]
        kj = tree_sum(_f(math, "log", 1.0 - b[:, :, None] * x[:, None, :])) / n
        L = n * ((_f(math, "log", -(b / kj)) - kj) - 1.0)
        acc = np.zeros((R, m))
        for l in range(m):
            acc = acc + _f(math, "exp", L[:, l:l + 1] - L)
        w = 1.0 / acc
        wz = np.where(w >= W_MIN, w, 0.0)
        sw = np.zeros(R)
        for j in range(m):
            sw = sw + wz[:, j]
        wn = wz / sw[:, None]
        bh = np.zeros(R)
        for j in range(m):
            bh = bh + b[:, j] * wn[:, j]
        k0 = tree_sum(_f(math, "log", 1.0 - bh[:, None] * x)) / n
        sigma = -(k0 / bh)
        kh = (n * k0 + 5.0) / (n + 10.0)
        deg = ~(q > 0.0) | ~np.isfinite(kh) | ~(sigma > 0.0)
        # the smoothed tail
        p = (np.arange(1, M + 1, dtype=np.float64) - 0.5) / n
        lg = _f(math, "log", 1.0 - p)                                      # [M]
        e = _f(math, "exp", (-kh)[:, None] * lg[None, :])
        g = np.where((kh == 0.0)[:, None], -(sigma[:, None] * lg[None, :]), (sigma[:, None] * (e - 1.0)) / kh[:, None])
        lt = _f(math, "log", g + ec[:, None])
        t = np.where(lt < 0.0, lt, 0.0)
        t = np.where(deg[:, None], raw, t)
        # the folds
        Wt = tree_sum(_f(math, "exp", t))
        Nt = tree_sum(_f(math, "exp", t + (st - s0[:, None])))
        B = np.zeros(R)
        for e0 in range(0, K - M, BODY_PIECE):
            e1 = min(K - M, e0 + BODY_PIECE)
            B = B + tree_sum(_f(math, "exp", s0[:, None] - s[:, M + e0:M + e1]))
        W = B + Wt
        N = np.float64(K - M) + Nt
        elpd = (s0 + _f(math, "log", N)) - _f(math, "log", W)
        pk = np.where(deg, np.inf, kh)
        elpd = np.where(bad, np.nan, elpd)
        pk = np.where(bad, np.nan, pk)
    return elpd, pk


def summary(elpd_loo, pareto_k, lppd):
    """(elpd_loo, p_loo, lppd, se_elpd_loo, n_bad): plain sums over r ascending from +0; p_loo = lppd - elpd_loo; se as waic.summary's on elpd_loo_r;
    n_bad = the number of rows with not (k <= 0.7)."""
    elpd_loo = np.asarray(elpd_loo, dtype=np.float64)
    lppd = np.asarray(lppd, dtype=np.float64)
    R = elpd_loo.shape[0]
    with np.errstate(all="ignore"):
        e = l = np.float64(0.0)
        for r in range(R):
            e = e + elpd_loo[r]
            l = l + lppd[r]
        mean = e / np.float64(R)
        v = np.float64(0.0)
        for r in range(R):
            dv = elpd_loo[r] - mean
            v = v + dv * dv
        se = np.sqrt(np.float64(R) * (v / np.float64(R - 1)))
    n_bad = np.float64(np.count_nonzero(~(np.asarray(pareto_k) <= K_BAD)))
    return np.array([e, l - e, l, se, n_bad])


def psis_ref(ll, math=waic.NUMPY_MATH):
    """dict of elpd_loo, pareto_k, lppd [n_rows] and summary [5] of ll [n_rows, n_keep, C] (or [n_rows, K]); lppd is waic.row_stats'."""
    ll = np.ascontiguousarray(ll, dtype=np.float64)
    elpd, pk = psis_rows(ll, math)
    lppd, _ = waic.row_stats(ll, math)
    return dict(elpd_loo=elpd, pareto_k=pk, lppd=lppd, summary=summary(elpd, pk, lppd))
