"""Pointwise log-likelihood, lppd and WAIC of a draws slab: the numpy statement of what mi_mcmc_draws_waic computes (include/mi_mcmc.h states the same,
order and constants included), as quantiles.py is for mi_mcmc_draws_quantiles and rank_stats.py for the rank diagnostics.

The samples are the K = n_keep * C columns k = t * C + c of a slab [n_keep, d, C].  ll[r, k] is the log-likelihood of observation r at sample k;
lppd[r] = log(mean_k exp(ll[r, k])); p_waic[r] is the sample variance of ll[r, :] (divisor K - 1); elpd_waic = sum_r (lppd[r] - p_waic[r]).

This module never looks at the library.  Every elementary operation below is one IEEE fp64 operation of numpy, rounded once; what numpy does not have
-- a fused multiply-add chain, and the library's own exp / log / softplus (det_math.hpp) -- comes in through `math`, a caller-supplied object or dict of
    dot(a, b)      the fma chain over i ascending of a[i] * b[i], from +0, as a float
    exp(x), log(x), softplus(x)     arrays -> arrays, elementwise
The device result is held to these functions bit for bit where `math` is the library's arithmetic (tests: the CPU oracle's); with math=NUMPY_MATH the
same orders run over numpy's own functions (an fma-free dot), which states the order but not the last bits."""
import numpy as np

CHUNK = 2048            # columns of a chunk
TILE = 128              # columns of a column tile
WAVE_COLS = 32          # columns of a tile that belong to one of its four groups w
SLOTS = 64              # running sums per (chunk, row)
LOG_2PI = 1.83787706640934548356
LOGISTIC, NORMAL_MODEL = 4, 5       # mi_target_kind


def _softplus_np(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(x > 0.0, x + np.log(1.0 + np.exp(-np.abs(x))), np.log(1.0 + np.exp(-np.abs(x))))


NUMPY_MATH = dict(dot=lambda a, b: float(np.sum(np.asarray(a) * np.asarray(b))), exp=np.exp, log=np.log, softplus=_softplus_np)


def _m(math, name):
    return math[name] if isinstance(math, dict) else getattr(math, name)


def slot(o):
    """The slot 0 .. 63 of the column at offset o inside its chunk."""
    o = np.asarray(o)
    return 16 * ((o % TILE) // WAVE_COLS) + o % 16


def loglik(kind, draws, y, X=None, math=NUMPY_MATH):
    """ll [n_rows, n_keep, C] of a slab [n_keep, d, C]: LOGISTIC (X [n_rows, d], y [n_rows]) or NORMAL_MODEL (d = 2: mu, sigma; y the observations)."""
    x = np.ascontiguousarray(draws, dtype=np.float64)
    n, d, C = x.shape
    y = np.ascontiguousarray(y, dtype=np.float64)
    R = y.shape[0]
    cols = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(n * C, d)         # column k = t * C + c
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if kind == LOGISTIC:
            X = np.ascontiguousarray(X, dtype=np.float64)
            dot = _m(math, "dot")
            eta = np.empty((R, n * C))
            for r in range(R):
                for k in range(n * C):
                    eta[r, k] = dot(X[r], cols[k])
            ll = y[:, None] * eta - np.asarray(_m(math, "softplus")(eta.ravel())).reshape(eta.shape)
        elif kind == NORMAL_MODEL:
            mu, sigma = cols[:, 0], cols[:, 1]
            base = -(0.5 * LOG_2PI + np.asarray(_m(math, "log")(sigma)))
            den = 2.0 * (sigma * sigma)
            e = y[:, None] - mu[None, :]
            ll = base[None, :] - (e * e) / den[None, :]
        else:
            raise ValueError(f"target kind {kind} has no observations")
    return ll.reshape(R, n, C)


def _tree64(u):
    """[..., 64] slots -> [...]: the 16 slots of each w halved four times, then (w0 + w1) + (w2 + w3)."""
    u = u.reshape(u.shape[:-1] + (4, 16))
    for h in (8, 4, 2, 1):
        u = u[..., :h] + u[..., h:2 * h]
    u = u[..., 0]
    return (u[..., 0] + u[..., 1]) + (u[..., 2] + u[..., 3])


def chunk_partials(ll_chunk, math=NUMPY_MATH, third=None):
    """(shift, A, S1, S2), each [n_rows], of one chunk ll_chunk [n_rows, n_b] (n_b <= CHUNK).  third: None, or the [n_rows, n_b] values that A sums
    in place of exp(ll) (mcmc_amd.predict: the replicates), in the same slots, order and tree."""
    R, nb = ll_chunk.shape
    sh = ll_chunk[:, 0].copy()
    o = np.arange(nb)
    s = slot(o)
    # the q-th column of a slot: two per column tile (offsets + 0 and + 16 inside the group's 32), ascending
    q = 2 * (o // TILE) + (o % WAVE_COLS) // 16
    nq = int(q.max()) + 1
    grid = np.zeros((R, nq, SLOTS))
    have = np.zeros((nq, SLOTS), dtype=bool)
    grid[:, q, s] = ll_chunk
    have[q, s] = True
    with np.errstate(over="ignore", invalid="ignore"):
        if third is None:
            ex = np.asarray(_m(math, "exp")(np.ascontiguousarray(grid).ravel())).reshape(grid.shape)
        else:
            ex = np.zeros((R, nq, SLOTS))
            ex[:, q, s] = third
        S1 = np.zeros((R, SLOTS))
        S2 = np.zeros((R, SLOTS))
        A = np.zeros((R, SLOTS))
        for i in range(nq):
            v = grid[:, i, :] - sh[:, None]
            m = have[i][None, :]
            S1 = np.where(m, S1 + v, S1)
            S2 = np.where(m, S2 + v * v, S2)
            A = np.where(m, A + ex[:, i, :], A)
        return sh, _tree64(A), _tree64(S1), _tree64(S2)


def row_stats(ll, math=NUMPY_MATH):
    """(lppd [n_rows], p_waic [n_rows]) of ll [n_rows, n_keep, C] (or [n_rows, K]), in the header's order."""
    ll = np.ascontiguousarray(ll, dtype=np.float64)
    R = ll.shape[0]
    ll = ll.reshape(R, -1)
    K = ll.shape[1]
    if K < 2:
        raise ValueError("at least 2 samples are needed")
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        n = mean = M2 = A = None
        for b, c0 in enumerate(range(0, K, CHUNK)):
            part = ll[:, c0:min(K, c0 + CHUNK)]
            nb = np.float64(part.shape[1])
            sh, Ab, S1, S2 = chunk_partials(part, math)
            mb = sh + S1 / nb
            M2b = S2 - (S1 * S1) / nb
            if b == 0:
                n, mean, M2, A = nb, mb, M2b, Ab
            else:
                delta = mb - mean
                nn = n + nb
                mean = mean + delta * (nb / nn)
                M2 = (M2 + M2b) + (delta * delta) * ((n * nb) / nn)
                n = nn
                A = A + Ab
        lppd = np.asarray(_m(math, "log")(A / np.float64(K)))
        p_waic = M2 / np.float64(K - 1)
    return lppd, p_waic


def summary(lppd, p_waic):
    """(elpd_waic, p_waic, lppd, se_elpd): plain sums over r ascending; se_elpd = sqrt(n_rows * var(elpd_r)), divisor n_rows - 1 (NaN for one row)."""
    lppd = np.asarray(lppd, dtype=np.float64)
    p_waic = np.asarray(p_waic, dtype=np.float64)
    R = lppd.shape[0]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        elpd_r = lppd - p_waic
        elpd = p = l = np.float64(0.0)
        for r in range(R):
            elpd = elpd + elpd_r[r]
            p = p + p_waic[r]
            l = l + lppd[r]
        m = elpd / np.float64(R)
        v = np.float64(0.0)
        for r in range(R):
            dv = elpd_r[r] - m
            v = v + dv * dv
        se = np.sqrt(np.float64(R) * (v / np.float64(R - 1)))
    return np.array([elpd, p, l, se])


def waic_ref(kind, draws, y, X=None, math=NUMPY_MATH):
    """dict of loglik [n_rows, n_keep, C], lppd, p_waic [n_rows] and summary [4] of a slab under a LOGISTIC or NORMAL_MODEL target."""
    ll = loglik(kind, draws, y, X, math)
    lppd, p_waic = row_stats(ll, math)
    return dict(loglik=ll, lppd=lppd, p_waic=p_waic, summary=summary(lppd, p_waic))
