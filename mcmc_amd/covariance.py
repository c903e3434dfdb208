"""Pooled mean and covariance of a draws slab: the numpy statement of what mi_mcmc_draws_covariance computes (include/mi_mcmc.h states the same, every
reduction order included), as waic.py is for mi_mcmc_draws_waic and quantiles.py for mi_mcmc_draws_quantiles.

The samples are the K = n_keep * C columns k = t * C + c of a slab [n_keep, d, C] (a chains' state [d, C] is the case n_keep = 1).
    mu_i = (sum_k x_ik) / K,   e_ik = x_ik - mu_i,   cov_ij = (sum_k e_ik e_jk) / (K - 1)

This module never looks at the library.  Every elementary operation below is one IEEE fp64 operation of numpy, rounded once; what numpy does not have
-- a fused multiply-add chain -- comes in through `math`, a caller-supplied object or dict of
    dot(a, b)      the fma chain over i ascending of a[i] * b[i], from +0, as a float
The device result is held to these functions bit for bit where `math` is the library's arithmetic (tests: the CPU oracle's); with math=NUMPY_MATH the
same orders run over numpy's own fma-free dot, which states the order but not the last bits."""
import numpy as np

TILE = 128              # rows and columns of an output tile
LANES = 256             # strided sums of a mean group
KC_MIN = 512            # the shortest chunk of the contraction
K_STEP = 16             # a chunk is a whole number of contraction steps

NUMPY_MATH = dict(dot=lambda a, b: float(np.sum(np.asarray(a) * np.asarray(b))))


def _m(math, name):
    return math[name] if isinstance(math, dict) else getattr(math, name)


def _ceil(a, b):
    return (a + b - 1) // b


def plan(n_keep, d, C):
    """dict of K and the header's G, seg (mean) and T, P, KC, n_chunks (cov) -- integers, the divisions as the header writes them."""
    n_keep, d, C = int(n_keep), int(d), int(C)
    K = n_keep * C
    if K < 2 or d < 1:
        raise ValueError("at least 2 samples and one dimension are needed")
    G = min(max(1, 4096 // d), _ceil(K, 4096))
    seg = LANES * _ceil(_ceil(K, G), LANES)
    G = _ceil(K, seg)
    T = _ceil(d, TILE)
    P = T * (T + 1) // 2
    n = max(1, 1024 // P)
    KC = max(KC_MIN, K_STEP * _ceil(_ceil(K, n), K_STEP))
    return dict(K=K, G=G, seg=seg, T=T, P=P, KC=KC, n_chunks=_ceil(K, KC))


def samples(draws):
    """[d, K] of a slab [n_keep, d, C] or a state [d, C]: column k = t * C + c."""
    x = np.asarray(draws, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    n_keep, d, C = x.shape
    return np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(d, n_keep * C)


def mean_ref(draws):
    """mu [d] in the header's order: per group 256 strided sums (m ascending, from +0), the halving tree, the groups ascending from +0, / K."""
    x = samples(draws)
    d, K = x.shape
    p = plan(1, d, K)
    with np.errstate(over="ignore", invalid="ignore"):
        total = np.zeros(d)
        for g in range(p["G"]):
            blk = x[:, g * p["seg"]:min(K, (g + 1) * p["seg"])]
            r = np.zeros((d, LANES))
            for m in range(_ceil(blk.shape[1], LANES)):
                col = blk[:, LANES * m:LANES * (m + 1)]                  # the samples g * seg + s + 256 m of the lanes s that still have one
                r[:, :col.shape[1]] = r[:, :col.shape[1]] + col
            h = LANES // 2
            while h >= 1:
                r[:, :h] = r[:, :h] + r[:, h:2 * h]
                h //= 2
            total = total + r[:, 0]
        return total / np.float64(K)


def centred(draws):
    """e [d, K] = x - mu, rounded once."""
    x = samples(draws)
    with np.errstate(over="ignore", invalid="ignore"):
        return x - mean_ref(draws)[:, None]


def chunk_bounds(K, KC):
    """[(lo, hi)] of the chunks q = 0, 1, ..: [q * KC, min(K, (q + 1) * KC))."""
    return [(lo, min(K, lo + KC)) for lo in range(0, K, KC)]


def element(e_i, e_j, bounds, dot):
    """one cov_ij before its division: per chunk one dot over k ascending, the chunk partials added in ascending q from +0."""
    s = np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for lo, hi in bounds:
            s = s + np.float64(dot(e_i[lo:hi], e_j[lo:hi]))
    return s


def covariance_ref(draws, math=NUMPY_MATH, elements=None):
    """cov in the header's order.  elements=None: the full matrix [d, d], every (i, j) with j <= i computed and (j, i) its copy.
    elements = a list of (i, j) with j <= i: a dict {(i, j): value} of those alone (what a large d affords)."""
    e = centred(draws)
    d, K = e.shape
    p = plan(1, d, K)
    bounds = chunk_bounds(K, p["KC"])
    dot = _m(math, "dot")
    div = np.float64(K - 1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if elements is not None:
            out = {}
            for i, j in elements:
                i, j = int(i), int(j)
                if not 0 <= j <= i < d:
                    raise ValueError(f"element ({i}, {j}) is not in the computed triangle j <= i < {d}")
                out[(i, j)] = element(e[i], e[j], bounds, dot) / div
            return out
        cov = np.empty((d, d))
        for i in range(d):
            for j in range(i + 1):
                cov[i, j] = cov[j, i] = element(e[i], e[j], bounds, dot) / div
    return cov
