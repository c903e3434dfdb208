"""Posterior predictive checks of a draws slab under the logistic target: the numpy statement of what mi_mcmc_draws_predict computes (include/mi_mcmc.h
states the same, order and constants included), as waic.py is for mi_mcmc_draws_waic.

The samples are the K = n_keep * C columns k = t * C + c of a slab [n_keep, d, C]; X [n_rows, d] are the rows to predict at.  eta[r, k] = X_r . x_k,
p = sigmoid(eta), u[r, k] the uniform of the Philox block of (seed, k, 0, r, STREAM_PREDICT), yrep = (u < p).  Per row over the draws: p_mean, p_var
(divisor K - 1), rep_freq; per draw over the rows: t_rep (the replicated successes), ll_rep, ll_obs; summary = (t_obs, ppp_t, ppp_dev, t_rep_mean).

This module never looks at the library.  Every elementary operation below is one IEEE fp64 (or integer) operation of numpy; what numpy does not have
comes in through `math`, a caller-supplied object or dict of
    dot(a, b)                     the fma chain over i ascending of a[i] * b[i], from +0, as a float
    exp(x), log(x), softplus(x), sigmoid(x)     arrays -> arrays, elementwise
    philox(ctr, key)              Philox4x32-10: counters [n, 4] and a key [2] of uint32 -> [n, 4] uint32
The device result is held to these functions bit for bit where `math` is the library's arithmetic (tests: the CPU oracle's); NUMPY_MATH runs the same
orders over numpy's own functions, which states the order but not the last bits (its Philox is exact)."""
import numpy as np

from . import waic
from .waic import _m

STREAM_PREDICT = 8      # det_math.hpp


def _sigmoid_np(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def _philox_np(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011) of counters [n, 4], key [2]"""
    c = np.array(ctr, dtype=np.uint64).reshape(-1, 4)
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = (np.uint64(int(v)) for v in key)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


NUMPY_MATH = dict(waic.NUMPY_MATH, sigmoid=_sigmoid_np, philox=_philox_np)


def linear(draws, X, math=NUMPY_MATH):
    """eta [n_rows, K] of a slab [n_keep, d, C] and X [n_rows, d]: one fma chain per element."""
    x = np.ascontiguousarray(draws, dtype=np.float64)
    n, d, C = x.shape
    X = np.ascontiguousarray(X, dtype=np.float64)
    R = X.shape[0]
    cols = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(n * C, d)         # column k = t * C + c
    dot = _m(math, "dot")
    eta = np.empty((R, n * C))
    for r in range(R):
        for k in range(n * C):
            eta[r, k] = dot(X[r], cols[k])
    return eta


def prob(draws, X, math=NUMPY_MATH, eta=None):
    """p [n_rows, n_keep, C] = sigmoid(eta)"""
    n, _, C = np.shape(draws)
    eta = linear(draws, X, math) if eta is None else eta
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.asarray(_m(math, "sigmoid")(np.ascontiguousarray(eta).ravel()))
    return p.reshape(eta.shape[0], n, C)


def uniforms(seed, n_rows, K, math=NUMPY_MATH, stream=STREAM_PREDICT):
    """u [n_rows, K]: u01 of the first two words of rng_block(seed, chain = k, draw = 0, slot = r, stream) (det_math.hpp), written out:
    counter = (k mod 2^32, 0, r, stream | (k div 2^32) * 2^8), key = (seed mod 2^32, seed div 2^32); u = (2 m + 1) 2^-53, m = the 52 high bits of (w1 : w0)."""
    r, k = np.meshgrid(np.arange(n_rows, dtype=np.uint64), np.arange(K, dtype=np.uint64), indexing="ij")
    r, k = r.ravel(), k.ravel()
    ctr = np.stack([k & np.uint64(0xFFFFFFFF), np.zeros_like(k), r, np.uint64(stream) | ((k >> np.uint64(32)) << np.uint64(8))], axis=1).astype(np.uint32)
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    w = np.asarray(_m(math, "philox")(ctr, key), dtype=np.uint64).reshape(-1, 4)
    m = ((w[:, 1] << np.uint64(32)) | w[:, 0]) >> np.uint64(12)
    u = (np.uint64(2) * m + np.uint64(1)).astype(np.float64) * 2.0 ** -53           # 2 m + 1 < 2^53: the conversion is exact
    return u.reshape(n_rows, K)


def yrep(p, u):
    """(u < p) as 1.0 / 0.0, in p's shape; a NaN p gives 0"""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (np.asarray(u).reshape(p.shape) < p).astype(np.float64)


def row_stats(p, yr, math=NUMPY_MATH):
    """(p_mean, p_var, rep_freq), each [n_rows], of p and yrep [n_rows, n_keep, C] (or [n_rows, K]): THE ORDER of mi_mcmc_draws_waic with p where ll stood
    and A = A + yrep where A + exp(ll) stood."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    R = p.shape[0]
    p = p.reshape(R, -1)
    yr = np.ascontiguousarray(yr, dtype=np.float64).reshape(R, -1)
    K = p.shape[1]
    if K < 2:
        raise ValueError("at least 2 samples are needed")
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        n = mean = M2 = A = None
        for b, c0 in enumerate(range(0, K, waic.CHUNK)):
            c1 = min(K, c0 + waic.CHUNK)
            nb = np.float64(c1 - c0)
            sh, Ab, S1, S2 = waic.chunk_partials(p[:, c0:c1], math, third=yr[:, c0:c1])
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
        return mean, M2 / np.float64(K - 1), A / np.float64(K)


def sum4(a):
    """[n_rows, K] -> [K]: four chains q[r % 4], r ascending, each from +0; (q0 + q2) + (q1 + q3)"""
    a = np.asarray(a, dtype=np.float64)
    q = np.zeros((4, a.shape[1]))
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(a.shape[0]):
            q[r % 4] = q[r % 4] + a[r]
        return (q[0] + q[2]) + (q[1] + q[3])


def col_stats(eta, yr, y=None, math=NUMPY_MATH):
    """(t_rep, ll_rep, ll_obs), each [K] (ll_obs None without y), of eta and yrep [n_rows, K]"""
    eta = np.ascontiguousarray(eta, dtype=np.float64)
    yr = np.ascontiguousarray(yr, dtype=np.float64).reshape(eta.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        sp = np.asarray(_m(math, "softplus")(eta.ravel())).reshape(eta.shape)
        t_rep = sum4(yr)
        ll_rep = sum4(yr * eta - sp)
        ll_obs = None if y is None else sum4(np.asarray(y, dtype=np.float64)[:, None] * eta - sp)
    return t_rep, ll_rep, ll_obs


def summary(y, t_rep, ll_rep, ll_obs):
    """(t_obs, ppp_t, ppp_dev, t_rep_mean); a comparison with a NaN counts as false, the counts and the sum of t_rep are integers"""
    y = np.asarray(y, dtype=np.float64)
    t_rep, ll_rep, ll_obs = (np.asarray(v, dtype=np.float64).ravel() for v in (t_rep, ll_rep, ll_obs))
    K = t_rep.shape[0]
    t_obs = np.float64(0.0)
    for v in y:
        t_obs = t_obs + v
    with np.errstate(invalid="ignore"):
        n_t = int(np.count_nonzero(t_rep >= t_obs))
        n_dev = int(np.count_nonzero(ll_rep <= ll_obs))
    total = sum(int(v) for v in t_rep)
    return np.array([t_obs, float(n_t) / float(K), float(n_dev) / float(K), float(total) / float(K)])


def predict_ref(draws, X, y=None, seed=0, math=NUMPY_MATH):
    """dict of prob, yrep [n_rows, n_keep, C], p_mean, p_var, rep_freq [n_rows], t_rep, ll_rep, ll_obs [n_keep, C] and summary [4] (ll_obs and summary
    None without y) of a slab under a logistic target."""
    draws = np.ascontiguousarray(draws, dtype=np.float64)
    if draws.ndim == 2:
        draws = draws[None]
    n, _, C = draws.shape
    eta = linear(draws, X, math)
    R = eta.shape[0]
    p = prob(draws, X, math, eta=eta)
    yr = yrep(p, uniforms(seed, R, n * C, math))
    p_mean, p_var, rep_freq = row_stats(p, yr, math)
    t_rep, ll_rep, ll_obs = col_stats(eta, yr.reshape(R, -1), y, math)
    return dict(prob=p, yrep=yr, p_mean=p_mean, p_var=p_var, rep_freq=rep_freq, t_rep=t_rep.reshape(n, C), ll_rep=ll_rep.reshape(n, C),
                ll_obs=None if y is None else ll_obs.reshape(n, C), summary=None if y is None else summary(y, t_rep, ll_rep, ll_obs))
