"""Exact reference of mi_mcmc_draw_stats_lags (plain numpy in np.longdouble), its error bounds, and the inputs of tests/test_gpu_draw_stats_lags.py.

reference_lags(x, K) is tests/draw_stats_ref.py::reference_of with the lag window a parameter instead of that file's 128-lag cut: the same longdouble
construction, the same bounds (that docstring derives them) --
  mean    (n C + 2) 2^-53 mean |x_j|
  acov_k  (N + 64) 2^-52 sum (|v_t| + E)(|v_{t+k}| + E) / N,  N = C (n - k)
  R-hat   relative (n + C + 64) 2^-52
  ESS     relative 64 max_{k used} bound_k / |acov_0|
-- and the same margin condition: at every pair up to and including the reference's stopping pair, |pair| exceeds 100 times its bound.  It also
returns ended: 1 if the sum met its non-positive pair inside [0, K], or K = n - 1, or n < 4."""
import functools
import hashlib

import numpy as np

import draw_stats_ref as R

LD = R.LD

# name -> (n, d, C, phi, seed): the issue's table
INPUTS = {
    "L1": (161, 2, 130, (0.2, 0.95), 9161),
    "L2": (400, 3, 130, (0.5, 0.97, 0.99), 9400),
    "L3": (1000, 2, 70, (0.7, 0.995), 9999),
    "L4": (320, 2, 65, (0.9, 0.99), 9320),
    "L5": (100, 2, 130, (0.5, 0.9), 9100),
    "L6": (150, 2, 130, (0.3, 0.97), 9150),
}
TILING = (2500, 1, 20, 0.9, 92500)


@functools.lru_cache(maxsize=None)
def slab_of(n, d, C, phi, seed, dim_offset=None, delta=0.0):
    x = np.ascontiguousarray(R.ar1(n, d, C, phi, seed, dim_offset=dim_offset, delta=delta))
    x.setflags(write=False)
    return x


def slab(name):
    return slab_of(*INPUTS[name])


def window(n, K):
    return n - 1 if K is None else min(int(K), n - 1)


@functools.lru_cache(maxsize=None)
def _all_lags(key):
    """exact values and bounds of EVERY lag of a slab (held by key in _SLABS): computed once, shared by every window"""
    x = _SLABS[key]
    n, d, C = x.shape
    c0 = x[0, :, 0].astype(LD)
    xl = x.astype(LD) - c0[None, :, None]
    mu_s = xl.sum(axis=(0, 2)) / (n * C)
    v = xl - mu_s[None, :, None]
    acov = np.stack([(v[: n - k] * v[k:]).sum(axis=(0, 2)) / (LD(C) * (n - k)) for k in range(n)])
    E = np.abs(v.mean(axis=2)).max(axis=0).astype(np.float64)
    a = np.abs(v).astype(np.float64) + E[None, :, None]
    acov_bound = np.stack([(C * (n - k) + 64) * 2.0 ** -52 * (a[: n - k] * a[k:]).sum(axis=(0, 2)) / (C * (n - k)) for k in range(n)])
    m = xl.mean(axis=0)
    W = (((xl - m[None]) ** 2).sum(axis=0) / (n - 1)).mean(axis=1) if n > 1 else np.zeros(d, dtype=LD)
    B_n = ((m - m.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (C - 1) if C > 1 else np.zeros(d, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        rhat = np.where(W > 0, np.sqrt((LD(n - 1) / n * W + B_n) / np.where(W > 0, W, 1)), LD(1.0))
    return dict(mean=c0 + mu_s, acov=acov, acov_bound=acov_bound, rhat=rhat, mean_bound=(n * C + 2) * 2.0 ** -53 * np.abs(x).mean(axis=(0, 2)),
                rhat_bound=(n + C + 64) * 2.0 ** -52 * np.abs(rhat).astype(np.float64))


_SLABS = {}


def reference_lags(x, K=None):
    """everything the tests compare with, of a float64 slab x[n][d][C] and a window K (None: every lag): exact values (np.longdouble), the bounds
    (float64), ended, and per dimension stop (first lag of the stopping pair or None), used (lags read) and margin"""
    n, d, C = x.shape
    K = window(n, K)
    key = (x.shape, hashlib.sha1(np.ascontiguousarray(x)).digest())
    _SLABS.setdefault(key, x)
    full = _all_lags(key)
    nlag = K + 1
    acov, acov_bound = full["acov"][:nlag], full["acov_bound"][:nlag]
    ess, stop, used, ess_bound, margin, ended = np.zeros(d, dtype=LD), [], [], np.zeros(d), np.full(d, np.inf), np.zeros(d, dtype=np.uint8)
    for j in range(d):
        e, s, u = R.geyer(acov[:, j], n, nlag)
        ess[j] = e; stop.append(s); used.append(u)
        ended[j] = 1 if (s is not None or K == n - 1 or n < 4) else 0
        if u:
            ess_bound[j] = 64.0 * float((acov_bound[:u, j] / abs(acov[0, j])).max()) * float(e)
            pairs = np.abs(acov[0:u - 1:2, j] + acov[1:u:2, j]).astype(np.float64)
            margin[j] = float((pairs / (acov_bound[0:u - 1:2, j] + acov_bound[1:u:2, j])).min())
    return dict(n=n, d=d, C=C, K=K, nlag=nlag, mean=full["mean"], acov=acov, rhat=full["rhat"], ess=ess, ended=ended, stop=stop, used=used, margin=margin,
                mean_bound=full["mean_bound"], acov_bound=acov_bound, rhat_bound=full["rhat_bound"], ess_bound=ess_bound)


def inside(tag, s, ref, extra=""):
    """every element of s (a draw_stats_lags result) inside the bounds of ref; prints the worst ratios; returns them"""
    w = dict(mean=R.worst(s["mean"], ref["mean"], ref["mean_bound"]), rhat=R.worst(s["rhat"], ref["rhat"], ref["rhat_bound"]),
             ess=R.worst(s["ess"], ref["ess"], ref["ess_bound"]))
    if s["acov"] is not None:
        assert s["acov"].shape == (ref["nlag"], ref["d"]), s["acov"].shape
        assert np.isfinite(s["acov"]).all()
        w["acov"] = R.worst(s["acov"], ref["acov"], ref["acov_bound"])
    print(f"draw_stats_lags {tag} (n, d, C, K) = ({ref['n']}, {ref['d']}, {ref['C']}, {ref['K']}):{extra} worst |got - ref| / bound: "
          + ", ".join(f"{k} {v:.3g}" for k, v in w.items()))
    for k, v in w.items():
        assert np.isfinite(s[k]).all(), k
        assert v <= 1.0, (k, v)
    assert np.array_equal(s["ended"], ref["ended"]), (s["ended"], ref["ended"])
    return w
