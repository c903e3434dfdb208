"""CPU reference of mcmc::aees (ref: src/aees.cpp:28-305, include/mcmc/aees.ipp:30-70) under the engine's RNG contract
(include/mi_mcmc.h, mi_mcmc_aees_run).

A transcription of aees_impl with omp_n_threads = 1 -- the levels in order at every draw -- and the four quirks the header pins, on
what the oracle already exports: Philox (orc_philox_eval), the normal vector (orc_normal_vec), exp / log (orc_math_eval), the
built-in targets (orc.TargetSpec), CHOL_LOWER (orc_chol_lower) and the box transforms.  The window of every equi-energy step is
sorted IN FULL here (a stable argsort of the literal window, every time), which is what checks the kernel's lazy merge.
One run per call; `run` is its global id.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

import orc
import de_ref

STREAM_AEES_NORMAL, STREAM_AEES = 5, 6
_ip = C.POINTER(C.c_int)


def block(seed, chain, n, slot):
    return de_ref.block(seed, chain, n, slot, STREAM_AEES)


u01 = de_ref.u01


def exp(x):
    return float(orc.math_eval(0, np.array([x]))[0][0])


def log(x):
    return float(orc.math_eval(1, np.array([x]))[0][0])


def fma(a, b, c):
    """a * b + c rounded once"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    if a == 0.0 or b == 0.0:
        return c + a * b                                  # the product is an exact +-0
    r = Fraction(a) * Fraction(b) + Fraction(c)
    return float(r) if r != 0 else 0.0                 # an exact zero sum of opposite signs is +0


def key(v):
    """the order quirk 4 pins: ascending, -0 == +0, NaN after +inf (ties are broken by position by the stable sort)"""
    if v != v:
        return (2, 0.0)
    return (0, v + 0.0)


def stable_argsort(w):
    return sorted(range(len(w)), key=lambda i: key(w[i]))


def mixture(x, means, variances, logc):
    """MI_TARGET_GAUSS_MIXTURE as include/mi_mcmc.h states it"""
    M, d = means.shape
    a = []
    for i in range(M):
        dist = 0.0
        for j in range(d):
            df = float(x[j]) - float(means[i, j])
            dist = dist + df * df
        a.append(float(logc[i]) - (0.5 * dist) / float(variances[i]))
    if any(v != v for v in a):
        return math.nan
    m = a[0]
    for v in a[1:]:
        if v > m:
            m = v
    if m == -math.inf or m == math.inf:
        return m
    s = 0.0
    for v in a:
        s = s + exp(v - m)
    return m + log(s)


def mixture_fn(means, variances, weights):
    means = np.asarray(means, dtype=np.float64)
    logc = np.log(np.asarray(weights, dtype=np.float64)) - (means.shape[1] / 2.0) * np.log(2.0 * np.pi * np.asarray(variances, dtype=np.float64))
    return lambda x: mixture(x, means, variances, logc)


def temperatures(temper_vec):
    T = [float(t) for t in (temper_vec if temper_vec is not None else [])] + [1.0]
    return sorted(T, reverse=True)                         # aees.cpp:62-76


def chol_lower(A):
    A = np.ascontiguousarray(A, dtype=np.float64)
    d = A.shape[0]
    L = np.zeros((d, d))
    assert orc.lib().orc_chol_lower(orc._p(A), C.c_size_t(d), orc._p(L)) == 0
    return L


def scaled_matrices(d, T, par_scale, cov_mat):
    """sqrt(T_k) * (par_scale * CHOL_LOWER(cov)) for every level"""
    L = chol_lower(np.asarray(cov_mat, dtype=np.float64).reshape(d, d)) if cov_mat is not None else np.eye(d)
    return [math.sqrt(t) * (par_scale * L) for t in T]


def matvec(A, z):
    """every row one fma chain, columns ascending"""
    d = len(z)
    out = np.empty(d)
    for i in range(d):
        acc = 0.0
        for c in range(d):
            acc = fma(A[i, c], z[c], acc)
        out[i] = acc
    return out


def aees_ref(log_kernel, init, n_burnin, n_keep, seed=0, run=0, lower=None, upper=None, n_initial=1000, par_scale=1.0, cov_mat=None,
             n_rings=5, ee_prob=0.10, temper_vec=None, want_draws=True, trace=None):
    """One run.  log_kernel(x) -> value (a TargetSpec or any Python function of the untransformed values).  Returns (draws
    [n_keep, d] or None, final states [K, d] (transformed space), n_accept [K], n_ee_accept [K]).  trace: a list that receives one
    dict per equi-energy step (for the hand-checked tests)."""
    init = np.asarray(init, dtype=np.float64)
    d = init.size
    if n_rings < 1:
        raise ValueError("n_rings >= 1")
    if isinstance(log_kernel, orc.TargetSpec):
        spec = log_kernel
        log_kernel = lambda x: spec.kernel(x, want_grad=False)[0]
    bd = de_ref.Bounds(d, lower, upper)

    def box_log_kernel(x):                                 # aees.cpp:117-128: no clamp of non-finite values
        if bd.on:
            return log_kernel(bd.inv(x)) + bd.log_jacobian(x)
        return log_kernel(np.asarray(x, dtype=np.float64))

    T = temperatures(temper_vec)
    K = len(T)
    S = n_initial + n_burnin
    n_total = n_keep + K * S
    A = scaled_matrices(d, T, par_scale, cov_mat)
    if bd.on:
        first = np.empty(d)
        orc.lib().orc_transform(orc._p(init), bd.bt.ctypes.data_as(_ip), orc._p(bd.lb), orc._p(bd.ub), C.c_size_t(d), orc._p(first))
    else:
        first = init.copy()
    X = np.zeros((K, d))
    X[0] = first
    cache = [box_log_kernel(X[0])] + [box_log_kernel(np.zeros(d))] * (K - 1)      # the log kernel of every level's current state
    kvp = np.zeros((2, K))                                 # kernel_vals_prev / _new
    kernel_vals = np.zeros((K, n_total))                   # row 0 never written (quirk 1)
    storage = np.zeros((n_total, K, d))                    # draw_storage; an entry not written yet reads as zeros (quirk 3)
    n_acc, n_ee = np.zeros(K, dtype=np.uint64), np.zeros(K, dtype=np.uint64)

    def mh(k, n, u):                                       # single_step_mh (aees.ipp:30-70)
        z = orc.normal_vec(seed, run * K + k, n, STREAM_AEES_NORMAL, d)
        prop = X[k] + matvec(A[k], z)
        vnew = box_log_kernel(prop)
        with np.errstate(invalid="ignore"):
            x = (vnew - cache[k]) / T[k]
        comp = x if x < 0.01 else 0.01                     # std::min(0.01, x): NaN -> 0.01
        if u < exp(comp):
            X[k] = prop
            cache[k] = vnew
            n_acc[k] += 1

    for n in range(n_total):
        for k in range(K):
            chain = run * K + k
            active = k == 0 or n > k * S
            if active:
                w = block(seed, chain, n, 0)
                z_eps, u = u01(w[0], w[1]), u01(w[2], w[3])
                if k == 0:
                    mh(0, n, u)
                elif z_eps > ee_prob:
                    mh(k, n, u)
                    kvp[0, k] = cache[k] / T[k - 1]
                    kvp[1, k] = cache[k] / T[k]
                else:
                    begin = (k - 1) * S
                    m = n - begin + 1
                    s = m // n_rings
                    if s != 0:
                        window = list(kernel_vals[k - 1, begin:n + 1])
                        order = stable_argsort(window)
                        srt = [window[i] for i in order]
                        bounds = [(srt[(i + 1) * s] + srt[(i + 1) * s - 1]) / 2.0 for i in range(n_rings - 1)]
                        kl = kernel_vals[k, n - 1]
                        which = 0
                        while which < n_rings - 1 and kl > bounds[which]:
                            which += 1
                        z_tmp = u01(*block(seed, chain, n, 1)[:2])
                        r = s * which + int(math.floor(z_tmp * s))
                        ind_mix = order[r]                 # a window position, used as an absolute draw index (quirk 2)
                        prop = storage[ind_mix, k - 1].copy()
                        val = box_log_kernel(prop)
                        new0, new1 = val / T[k - 1], val / T[k]
                        with np.errstate(invalid="ignore"):
                            x = (new1 - kvp[1, k]) + (kvp[0, k] - new0)
                        comp = x if x < 0.01 else 0.01
                        accept = not (u > exp(comp))
                        if trace is not None:
                            trace.append(dict(n=n, k=k, s=s, bounds=bounds, which=which, r=r, ind_mix=ind_mix, accept=accept))
                        if accept:
                            X[k] = prop
                            cache[k] = val
                            kvp[0, k], kvp[1, k] = new0, new1
                            n_ee[k] += 1
                kernel_vals[k, n] = cache[k] if k >= 1 else 0.0
        storage[n] = X
    draws = None
    if want_draws:
        rows = storage[K * S:, K - 1]
        draws = np.array([bd.inv(x) for x in rows]) if bd.on else rows.copy()
        draws = draws.reshape(n_keep, d)
    return draws, X.copy(), n_acc, n_ee
