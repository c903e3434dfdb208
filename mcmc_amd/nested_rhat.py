"""Nested R-hat of a draws slab: the numpy statement of what mi_mcmc_draw_stats_nested and mi_mcmc_draw_stats_nested_ranked compute (include/mi_mcmc.h
states the same, every reduction order included), as covariance.py is for mi_mcmc_draws_covariance.

Margossian, Hoffman, Sountsov, Riou-Durand, Vehtari, Gelman (2024), "Nested R-hat: assessing the convergence of Markov chain Monte Carlo when running
many short chains".  The C chains of a slab [N, d, C] are K = C / M superchains of M consecutive chains that share their initial point: chain c is
member c mod M of superchain c // M.  With a, v the mean and variance of a chain's N draws (v = 0 for N = 1),
    A_k = mean_m a,   w_k = var_m a + mean_m v,   mean = mean_k A_k,   between = var_k A_k,   within = mean_k w_k
    nrhat = sqrt(1 + between / within),   mcse_mean = sqrt(between / K)
For stationary superchains with independent members between / within is about 1 / (M * ESS of one chain's N draws): a threshold on nrhat is a
statement about M.

This module never looks at the library.  Every elementary operation below is one IEEE fp64 operation of numpy, rounded once, in the header's order:
sums over the draws run t ascending from +0.0, sums over members and over superchains are SUM64."""
import numpy as np

LANES = 64


def sum64(u):
    """SUM64 along the last axis: lane s adds u[..., s + 64 j], j ascending, from +0.0 (a lane without elements stays +0.0); then
    r[s] = r[s] + r[s + h] for h = 32, 16, .., 1; the result is r[0]."""
    u = np.asarray(u, dtype=np.float64)
    n = u.shape[-1]
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.zeros(u.shape[:-1] + (LANES,))
        for j in range((n + LANES - 1) // LANES):
            blk = u[..., LANES * j:LANES * (j + 1)]
            r[..., :blk.shape[-1]] = r[..., :blk.shape[-1]] + blk
        h = LANES // 2
        while h >= 1:
            r[..., :h] = r[..., :h] + r[..., h:2 * h]
            h //= 2
    return np.ascontiguousarray(r[..., 0])


def _slab(draws):
    x = np.asarray(draws, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    return x


def chain_moments(draws):
    """(a, v), each [d, C]: the mean and the two-pass variance of every chain's N draws, t ascending from +0.0; v = +0.0 for N = 1."""
    x = _slab(draws)
    N = x.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.zeros(x.shape[1:])
        for t in range(N):
            s = s + x[t]
        a = s / np.float64(N)
        q = np.zeros(x.shape[1:])
        if N == 1:
            return a, q
        for t in range(N):
            e = x[t] - a
            p = e * e
            q = q + p
        return a, q / np.float64(N - 1)


def nested_ref(draws, M):
    """What mi_mcmc_draw_stats_nested writes, as a dict: nrhat, mean, between, within, mcse_mean [d] and super_mean [K, d]."""
    x = _slab(draws)
    N, d, C = x.shape
    M = int(M)
    if M < 1 or C % M or C // M < 2 or (N == 1 and M == 1):
        raise ValueError("M must divide C into at least 2 superchains, and not N = 1 with M = 1")
    K = C // M
    a, v = chain_moments(x)
    a, v = a.reshape(d, K, M), v.reshape(d, K, M)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        A = sum64(a) / np.float64(M)                                     # [d, K]
        if M >= 2:
            e = a - A[:, :, None]
            Bt = sum64(e * e) / np.float64(M - 1)
        else:
            Bt = np.zeros((d, K))
        Wt = sum64(v) / np.float64(M)
        w = Bt + Wt
        mean = sum64(A) / np.float64(K)
        e = A - mean[:, None]
        between = sum64(e * e) / np.float64(K - 1)
        within = sum64(w) / np.float64(K)
        nrhat = np.sqrt(1.0 + between / within)
        mcse = np.sqrt(between / np.float64(K))
    return dict(nrhat=nrhat, mean=mean, between=between, within=within, mcse_mean=mcse, super_mean=np.ascontiguousarray(A.T))


def nested_ranked_ref(draws, M):
    """What mi_mcmc_draw_stats_nested_ranked writes, as a dict of [d] arrays: nrhat_bulk from the normal scores of x, nrhat_tail from those of
    |x - median| (rank_stats.py, no split), nrhat the larger of the two, NaN if either is NaN."""
    from . import rank_stats as R
    x = np.ascontiguousarray(_slab(draws))
    rb = nested_ref(R.normal_scores(x), M)["nrhat"]
    rt = nested_ref(R.normal_scores(R.folded(x)), M)["nrhat"]
    return dict(nrhat=np.where(np.isnan(rb) | np.isnan(rt), np.nan, np.maximum(rb, rt)), nrhat_bulk=rb, nrhat_tail=rt)


def superchain_init(points, M):
    """points [d, K] -> initial values [d, K * M]: every point repeated for the M consecutive chains of its superchain."""
    return np.ascontiguousarray(np.repeat(np.asarray(points, dtype=np.float64), int(M), axis=1))
