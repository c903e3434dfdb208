"""Exact reference of mi_mcmc_draw_stats (plain numpy in np.longdouble), its error bounds, and every input of tests/test_gpu_draw_stats.py.

Definitions (those of mcmc_amd/ess.py and of the host code in mcmc_amd/csrc/stats_collate.hip), per dimension j of a slab x[t][j][c], n x d x C:
  mu      = sum_{t,c} x / (n C)                                      the pooled mean
  acov_k  = sum_c sum_{t < n-k} v_t v_{t+k} / (C (n - k)),  v = x - mu      pooled over chains, unbiased per lag
  W       = mean_c var_c (ddof = 1; 0 when n = 1),   B/n = var_c (chain means) (ddof = 1; 0 when C = 1)
  R-hat   = sqrt(((n - 1) / n W + B/n) / W) when W > 0, else 1.0     (the library's rule as it stands; no input here has a constant chain)
  ESS     = Geyer's initial positive sequence over acov, transcribed from ess_per_chain: n when n < 4, rho = acov / acov_0 (acov_0 <= 0: / 1),
            tau = -1 + 2 sum of the adjacent pairs before the first non-positive one, n / max(tau, 1 / n) when tau > 0 else n, at most 10 n.
            Series beyond 160 draws get lags 0..127 only (the streamed route's documented truncation): the reference sums the same 128 lags.

Bounds.  u = 2^-53 is the unit roundoff of float64; a length-m sum of products of once-rounded operands, in any order, with or without fma, errs by
at most gamma_m sum |terms|, gamma_m ~ m u; the bounds below spend twice that, (m + 64) 2^-52, as tests/test_gpu_draws_cov.py does.  All of them are
per element and per dimension, never a global rtol.
  mean:   |mean_j - mu_j| <= (n C + 2) 2^-53 mean |x_j|                one sum of n C terms and a division (the two extra roundings)
  acov_k: N = C (n - k) terms.  A kernel may centre by the pooled mean or by a PROVISIONAL centre a (the one-pass Gram route: the mean over chains of
          the first, middle and last row) and move the centre afterwards; a is an average of row means, so |a - mu| <= E = max_t |mean_c x_t - mu|, and
          whichever centre was used every product a kernel formed is at most (|v_t| + E)(|v_{t+k}| + E) in magnitude.  Hence, for every route,
              |acov_k - ref_k| <= (N + 64) 2^-52 sum_{c,t} (|v_t| + E)(|v_{t+k}| + E) / N.
          The bound's own sum of magnitudes is taken in float64.
  R-hat:  W is a sum of non-negative terms (squared deviations from the chain's own mean), so its relative error is that of the sums themselves;
          B/n is a variance of chain means that are already centred.  Relative bound (n + C + 64) 2^-52:  n pays for the n-term sums within a chain
          (the chain mean and the squared deviations), C for the C-term sums over chains (W, the mean and the sum of squares of the chain means), 64
          for the fixed number of roundings around them (centring, the divisions, (n - 1) / n, the square root, each halved or not by it).
  ESS:    relative 64 max_{k used} bound_k / |acov_0|, k over the lags Geyer's sum read (the stopping pair included) -- PROVIDED the device stops at
          the lag the reference stops at.  That is the margin condition: at the reference's stopping pair and at every earlier pair, |acov_t +
          acov_{t+1}| exceeds 100 times (bound_t + bound_{t+1}).  tests/test_draw_stats_ref_cpu.py asserts it for every input and dimension below.

Inputs.  ar1() extends the AR(1) generator the suite has always used (same bits for the old arguments) with a phi per dimension, an offset per
dimension, an offset per (dimension, chain) uniform in +-delta, and a drifting start amp 0.9^t.  Every input comes from a fixed seed; a slab for n draws
is a prefix of the slab for n + 1 draws of the same seed."""
import functools

import numpy as np

LD = np.longdouble
STATS_GRAM_MAX_N, STATS_MAX_N, STATS_TILED_LAGS = 128, 160, 128


def route_of(n):
    """0 the one-pass Gram kernel, 1 the window + lag-block ladder, 2 the streamed (time-tiled) kernel"""
    return 0 if n <= STATS_GRAM_MAX_N else (1 if n <= STATS_MAX_N else 2)


def gram_groups(n, d, C):
    """chain groups G of a call, and the 64-chain tiles the first (largest) group walks"""
    G = max(1, min(64, (2048 + d - 1) // d, (C + 63) // 64)) if n <= STATS_GRAM_MAX_N else min(64, (C + 63) // 64)
    per = (C + G - 1) // G
    return G, (min(per, C) + 63) // 64


def ar1(n, d, C, phi, seed, dim_offset=None, delta=0.0, drift=0.0):
    rng = np.random.default_rng(seed)
    ph = np.broadcast_to(np.asarray(phi, dtype=np.float64), (d,))[:, None] if np.ndim(phi) else phi
    y = np.zeros((n, d, C))
    y[0] = rng.standard_normal((d, C))
    for t in range(1, n):
        y[t] = ph * y[t - 1] + np.sqrt(1 - ph ** 2) * rng.standard_normal((d, C))
    off = np.arange(d, dtype=np.float64) if dim_offset is None else np.asarray(dim_offset, dtype=np.float64)
    y = y + off[None, :, None]                                   # a different mean per dimension
    if delta:
        y = y + np.random.default_rng([seed, 1]).uniform(-delta, delta, (d, C))[None]       # chains that disagree
    if drift:
        y = y + (drift * 0.9 ** np.arange(n))[:, None, None]     # a start far from the mode, forgotten at rate 0.9
    return y


# ---- the inputs of the GPU tests: name -> (n, d, C, phi, seed, dim_offset, delta, drift).  want_acov is the test's business: one slab serves both.
OFFSETS = (0.0, 1e3, 1e6, -1e8)
LADDER_PHIS = (0.97, 0.0, 0.9, 0.3, 0.99)
GRAM_NS = (1, 2, 3, 4, 15, 16, 17, 48, 49, 64, 65, 80, 96, 97, 112, 113, 127, 128)
DELTAS = (1e2, 1e4, 1e6)
SPECS = {}


def _add(name, n, d, C, phi, seed, dim_offset=None, delta=0.0, drift=0.0):
    assert name not in SPECS
    SPECS[name] = (n, d, C, phi, seed, dim_offset, delta, drift)
    return name


# the shapes the suite has always had
OLD_FULL = [_add(f"old-{n}-{d}-{C}", n, d, C, phi, n) for n, d, C, phi in [(100, 5, 700, 0.6), (40, 3, 64, 0.0), (160, 2, 1000, 0.9), (7, 4, 130, 0.3)]]
OLD_LONG = [_add(f"old-{n}-{d}-{C}", n, d, C, phi, n) for n, d, C, phi in [(1000, 3, 200, 0.7), (161, 2, 130, 0.2), (517, 2, 64, 0.95)]]
OLD_NOACOV = [_add(f"oldq-{n}-{d}-{C}", n, d, C, phi, n + C) for n, d, C, phi in [(100, 5, 700, 0.6), (40, 3, 64, 0.0), (160, 2, 1000, 0.9), (7, 4, 130, 0.3),
                                                                                (1000, 3, 200, 0.7), (100, 2, 300, 0.97), (20, 130, 70, 0.5)]]
FALLS_THROUGH = _add("oldq-150-2-300", 150, 2, 300, 0.97, 150 + 300)
# Gram: the tile loop
TILE_LOOP = [_add("tiles-33-1-40000", 33, 1, 40000, 0.5, 33), _add("tiles-100-1-8200", 100, 1, 8200, 0.8, 100), _add("tiles-5-2049-200", 5, 2049, 200, 0.4, 5)]
TILE_LOOP_EXPECT = {"tiles-33-1-40000": (64, 10, 3), "tiles-100-1-8200": (64, 3, 7), "tiles-5-2049-200": (1, 4, 1)}       # G, tiles, NB
# Gram: every NB and its edges; n = 129 continues the same series on the other side of the route boundary
GRAM_SWEEP = [_add(f"nb-{n}", n, 2, 130, 0.5, 7) for n in GRAM_NS]
BOUNDARY_129 = _add("nb-129", 129, 2, 130, 0.5, 7)
# ladder
LADDER_ACOV = [_add(f"ladder-{n}", n, 3, 130, (0.2, 0.6, 0.9), 1000 + n) for n in (129, 145, 159, 160)]
LADDER_SUBSETS = _add("ladder-subsets", 150, 5, 130, LADDER_PHIS, 150)
# tiled
TILED_EDGES = [_add(f"tiled-{n}", n, 2, 65, 0.6, 2000 + n) for n in (192, 193, 256)]
# chains and groups
CHAIN_EDGES = [_add(f"chains-{C}", 40, 2, C, 0.4, 40 + C) for C in (1, 63, 64, 65)] + [_add("chains-4097", 10, 1, 4097, 0.4, 4097)]
# centring
CENTRING = {n: _add(f"offsets-{n}", n, 4, 130, 0.5, 3000 + n, dim_offset=OFFSETS) for n in (100, 150, 300)}
DRIFT = {n: _add(f"drift-{n}", n, 2, 130, 0.5, 4000 + n, drift=50.0) for n in (100, 150)}
# chains that disagree: the same series at three lengths, offsets uniform in +-delta
DISAGREE = {(delta, n): _add(f"disagree-{delta:g}-{n}", n, 2, 200, 0.3, 5000 + i, delta=delta) for i, delta in enumerate(DELTAS) for n in (100, 150, 300)}
# non-finite samples are poked into these
NONFINITE = [_add("nonfinite-41", 41, 3, 130, 0.5, 41), _add("nonfinite-150", 150, 3, 130, 0.5, 6150)]


@functools.lru_cache(maxsize=None)
def slab(name):
    """the input of a case: float64 [n, d, C], read-only, shared"""
    n, d, C, phi, seed, dim_offset, delta, drift = SPECS[name]
    x = np.ascontiguousarray(ar1(n, d, C, phi, seed, dim_offset=dim_offset, delta=delta, drift=drift))
    x.setflags(write=False)
    return x


def geyer(acov_j, n, nlag):
    """ess_per_chain's loop on one dimension's autocovariances acov_j[0 .. nlag): (ess, t_stop, lags read).  t_stop: the first lag of the
    non-positive pair, None when the sum ran through every lag there is."""
    if n < 4:
        return float(n), None, 0
    a0 = acov_j[0]
    den = a0 if a0 > 0 else type(a0)(1.0)
    tau, t, stop = type(a0)(-1.0), 0, None
    while t + 1 < nlag:
        pair = acov_j[t] / den + acov_j[t + 1] / den
        if pair <= 0:
            stop = t
            break
        tau += 2.0 * pair
        t += 2
    ess = n / max(tau, type(a0)(1.0) / n) if tau > 0 else type(a0)(n)
    return min(ess, type(a0)(10.0 * n)), stop, (stop + 2 if stop is not None else t)


def reference_of(x):
    """everything the tests compare with, of a float64 slab x[n][d][C]: exact values (np.longdouble) and the bounds (float64) of the module docstring"""
    n, d, C = x.shape
    nlag = n if n <= STATS_MAX_N else STATS_TILED_LAGS
    # exact arithmetic needs the shift as much as float64 does: at |mean| / sd = 1e8 a longdouble sum of n C samples is good to ~1e-11 sd only.  x - x[0][j][0]
    # is exact in longdouble (two doubles of about the same size), and every quantity below but the mean does not depend on the shift.
    c0 = x[0, :, 0].astype(LD)
    xl = x.astype(LD) - c0[None, :, None]
    mu_s = xl.sum(axis=(0, 2)) / (n * C)
    mu = c0 + mu_s
    v = xl - mu_s[None, :, None]
    acov = np.stack([(v[: n - k] * v[k:]).sum(axis=(0, 2)) / (LD(C) * (n - k)) for k in range(nlag)])
    mean_bound = (n * C + 2) * 2.0 ** -53 * np.abs(x).mean(axis=(0, 2))
    E = np.abs(v.mean(axis=2)).max(axis=0).astype(np.float64)
    a = np.abs(v).astype(np.float64) + E[None, :, None]
    acov_bound = np.stack([(C * (n - k) + 64) * 2.0 ** -52 * (a[: n - k] * a[k:]).sum(axis=(0, 2)) / (C * (n - k)) for k in range(nlag)])
    m = xl.mean(axis=0)                                                          # [d, C] chain means
    W = (((xl - m[None]) ** 2).sum(axis=0) / (n - 1)).mean(axis=1) if n > 1 else np.zeros(d, dtype=LD)
    B_n = ((m - m.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (C - 1) if C > 1 else np.zeros(d, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        rhat = np.where(W > 0, np.sqrt((LD(n - 1) / n * W + B_n) / np.where(W > 0, W, 1)), LD(1.0))
    rhat_bound = (n + C + 64) * 2.0 ** -52 * np.abs(rhat).astype(np.float64)
    ess, stop, used, ess_bound, margin = np.zeros(d, dtype=LD), [], [], np.zeros(d), np.full(d, np.inf)
    for j in range(d):
        e, s, u = geyer(acov[:, j], n, nlag)
        ess[j] = e; stop.append(s); used.append(u)
        if u:
            ess_bound[j] = 64.0 * float((acov_bound[:u, j] / abs(acov[0, j])).max()) * float(e)
            pairs = np.abs(acov[0:u - 1:2, j] + acov[1:u:2, j]).astype(np.float64)
            margin[j] = float((pairs / (acov_bound[0:u - 1:2, j] + acov_bound[1:u:2, j])).min())
    return dict(n=n, d=d, C=C, nlag=nlag, mean=mu, acov=acov, rhat=rhat, ess=ess, W=W, B_n=B_n, stop=stop, used=used, margin=margin,
                mean_bound=mean_bound, acov_bound=acov_bound, rhat_bound=rhat_bound, ess_bound=ess_bound)


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(slab(name))


def worst(got, ref, bound):
    """max |got - ref| / bound over the elements (0 / 0 counts as 0: an exact value with a zero bound)"""
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


def ladder_plan(ref):
    """What the host ladder of a want_acov=False call at 129 <= n <= 160 launches, derived from the reference autocovariances alone: the window
    kernel's 16 lags, then lag passes of 2, then 3 blocks of 16 for the dimensions whose Geyer sum has not met its non-positive pair inside the lags
    known so far.  Returns dict(passes = [(first lag, last lag + 1, open dimensions)], lag_passes, subset_passes, smallest_subset, open_after_window)."""
    n, d = ref["n"], ref["d"]
    assert STATS_GRAM_MAX_N < n <= STATS_MAX_N
    opened = lambda known: [j for j in range(d) if not (ref["stop"][j] is not None and ref["stop"][j] + 1 < known) and known < n]
    known, passes = 16, []
    active = opened(known)
    after_window = list(active)
    b_all = (n + 15) // 16
    while active and known < n:
        b_lo = known // 16
        b_hi = min(b_all, b_lo + (2 if b_lo == 1 else 3))
        passes.append((16 * b_lo, min(n, 16 * b_hi), list(active)))
        known = min(n, 16 * b_hi)
        active = [j for j in active if j in opened(known)]
    subsets = [len(p[2]) for p in passes if len(p[2]) < d]
    return dict(passes=passes, lag_passes=len(passes), subset_passes=len(subsets), smallest_subset=min(subsets) if subsets else 0,
                open_after_window=after_window)
