"""The two estimator kernels of the mass adaptations (mcmc_amd/csrc/mass_adapt.hip), restated in numpy in the kernels' own order, as mcmc_amd/covariance.py
restates the pooled covariance (helper of tests/test_gpu_mass_adapt_device.py and tests/test_mass_estimators_ref_cpu.py; not collected).

Every elementary operation is one IEEE fp64 operation of numpy, rounded once; the fused multiply-add chain comes in through `dot(a, b)`: the chain over i
ascending of a[i] * b[i], from +0 (tests: orc.dot(a, b, 1), the oracle's fma).

pooled_variance_kernel, one workgroup of 256 lanes per dimension, row = theta[i, :] over the C chains:
    s_l    = row[l] + row[l + 256] + ...                 (lane l, chains ascending, from +0)
    S      = the halving tree over the lanes: m = 128, 64, .., 1: r[l] += r[l + m] for l < m
    mean   = S / C
    e_c    = row[c] - mean
    q_l    = fma chain of e_c * e_c over the lane's chains, ascending, from +0
    var    = (the same tree over q) / (C - 1)             (C = 1: / 1)
    mass_i = 1 / var, or 1 where that is not finite or not positive        (the host, mi_mcmc_hmc_run_mass_adapted)

chain_mass_estimate_kernel, one lane per (dimension, chain), x_t the chain's n draws of one burn-in part:
    s = x_0 + x_1 + ...  (from +0),  mean = s / n,  q = fma chain of (x_t - mean)^2 ascending from +0,  var = q / (n - 1)
    reg = (n var + 5e-3) / (n + 5),  mass = 1 / reg, or 1 where that is not finite or not positive"""
import numpy as np

LANES = 256
NUMPY_MATH = dict(dot=lambda a, b: float(np.sum(np.asarray(a) * np.asarray(b))))      # states the order, not the last bits (no fma)


def _tree(r):
    r = r.copy()
    m = LANES // 2
    while m >= 1:
        r[:m] = r[:m] + r[m:2 * m]
        m //= 2
    return r[0]


def pooled_variance_ref(theta, dot=NUMPY_MATH["dot"]):
    """var [d] of theta [d][C] over the chains"""
    theta = np.asarray(theta, dtype=np.float64)
    d, C = theta.shape
    out = np.empty(d)
    with np.errstate(all="ignore"):
        for i in range(d):
            row = theta[i]
            s = np.zeros(LANES)
            for lo in range(0, C, LANES):
                col = row[lo:lo + LANES]
                s[:col.size] = s[:col.size] + col
            mean = _tree(s) / np.float64(C)
            e = row - mean
            q = np.zeros(LANES)
            for l in range(min(LANES, C)):
                q[l] = dot(e[l::LANES], e[l::LANES])
            out[i] = _tree(q) / np.float64(C - 1 if C > 1 else 1)
    return out


def mass_or_one(m):
    m = np.asarray(m, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(m) & (m > 0.0), m, 1.0)


def pooled_mass_ref(theta, dot=NUMPY_MATH["dot"]):
    """mass [d]: 1 / the pooled variance, 1 where that is not finite or not positive"""
    with np.errstate(all="ignore"):
        return mass_or_one(1.0 / pooled_variance_ref(theta, dot))


def chain_variance_ref(slab, dot=NUMPY_MATH["dot"]):
    """var [d][C] of a slab [n][d][C] over its n draws"""
    slab = np.asarray(slab, dtype=np.float64)
    n, d, C = slab.shape
    with np.errstate(all="ignore"):
        s = np.zeros((d, C))
        for t in range(n):
            s = s + slab[t]
        x = slab - (s / np.float64(n))[None]
        q = np.empty((d, C))
        for i in range(d):
            for c in range(C):
                q[i, c] = dot(x[:, i, c], x[:, i, c])
        return q / np.float64(n - 1)


def chain_mass_ref(slab, dot=NUMPY_MATH["dot"]):
    """mass [d][C]: Stan's regularisation of the per-chain variance, inverted; 1 where that is not finite or not positive"""
    n = np.float64(np.shape(slab)[0])
    with np.errstate(all="ignore"):
        reg = (n * chain_variance_ref(slab, dot) + 5.0e-3) / (n + 5.0)
        return mass_or_one(1.0 / reg)


# ---- the inputs both test modules use
C_POOLED = (2, 255, 256, 257, 1000)
PART_LENGTHS = (3, 7)
DIMS = ("unit", "offset_1e8", "constant", "one_inf", "spread_1e-170")
FINITE_DIMS = ("unit", "offset_1e8", "constant")       # (spread 1e-170: every square underflows to 0, outside the rounding model of the bound)


def pooled_input(C, seed=0):
    """[5][C]: a unit-scale dimension, one offset by 1e8 with spread 1, a constant one (0.75: every partial sum and the mean are exact, the variance is
    exactly 0), one that holds one inf, one with spread 1e-170 (its squares underflow: variance 0, the reciprocal overflows)"""
    rng = np.random.default_rng(seed + C)
    x = np.empty((len(DIMS), C))
    x[0] = rng.standard_normal(C)
    x[1] = 1.0e8 + rng.standard_normal(C)
    x[2] = 0.75
    x[3] = rng.standard_normal(C); x[3, C // 2] = np.inf
    x[4] = 1.0e-170 * rng.standard_normal(C)
    return x


def chain_input(n, C=9, seed=0):
    """[n][5][C] of the same five kinds of dimension over the draws; chain 1 is stuck in every dimension (every draw its first: q = 0, the regularised mass)"""
    rng = np.random.default_rng(seed + n)
    x = np.empty((n, len(DIMS), C))
    x[:, 0] = rng.standard_normal((n, C))
    x[:, 1] = 1.0e8 + rng.standard_normal((n, C))
    x[:, 2] = 0.75
    x[:, 3] = rng.standard_normal((n, C)); x[n // 2, 3, :] = np.inf
    x[:, 4] = 1.0e-170 * rng.standard_normal((n, C))
    x[:, :, 1] = x[0, :, 1][None]
    return x
