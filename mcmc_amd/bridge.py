"""The log marginal likelihood by bridge sampling with a Gaussian proposal (Meng and Wong 1996; Gronau et al. 2017): the numpy statement of what
mi_mcmc_bridge_proposal, mi_mcmc_bridge_estimate and mi_mcmc_draws_bridge compute (include/mi_mcmc.h states the same, orders and constants included), as
waic.py is for mi_mcmc_draws_waic and psis.py for mi_mcmc_draws_psis_loo.

The slab is [n_keep, d, C].  Rows t < n_fit are the FIT PART (K0 = n_fit * C samples): the proposal N(mu, S) is fitted to them.  Rows t >= n_fit are the
ITERATION PART (n_it rows, N1 = n_it * C samples, sample j = (t - n_fit) * C + c).  N2 proposal draws y = mu + L z are generated.  With l1 = logp - logg on
the iteration part and l2 likewise on the proposal draws, the estimate r of Z / exp(l*) is the fixed point of
    r = (mean_i a_i / (s1 a_i + s2 r)) / (mean_j 1 / (s1 b_j + s2 r)),   a = exp(l2 - l*), b = exp(l1 - l*), s1 = n_eff / (n_eff + N2), s2 = N2 / (n_eff + N2).

This module never looks at the library.  Every elementary operation is one IEEE fp64 operation of numpy, rounded once; what numpy does not have comes in
through `math`, a caller-supplied object or dict of
    dot(a, b)                the fma chain over i ascending of a[i] * b[i], from +0
    dot4(a, b)               four such chains q[i % 4], met as (q0 + q2) + (q1 + q3)
    exp(x), log(x), softplus(x)      arrays -> arrays, elementwise (the library's det_math.hpp)
    normal_vec(seed, i, d)   the d normals of Philox stream STREAM_BRIDGE with "chain" i and draw 0
    chol_lower(S), inverse(S)        CHOL_LOWER and INV of a d x d matrix in the engine's operation order
The device result is held to these functions bit for bit where `math` is the library's arithmetic (tests: the CPU oracle's); NUMPY_MATH runs the same
orders over numpy's own functions and generator, which states the estimator but not the last bits.

The conventions are the library's own: SUMP is the body fold of psis.py (pieces of 16 384, tree_sum each, the pieces ascending from +0), the median l* is
quantiles.quantiles_ref at 0.5, the moments of the error terms are waic.py's chunks and merge, (mu, S) are covariance.py's."""
import numpy as np

from . import covariance, psis, quantiles, waic

STREAM_BRIDGE = 7
PIECE = psis.BODY_PIECE
LOG_2PI = waic.LOG_2PI
ISO, DIAG, DENSE, LOGISTIC = 1, 2, 3, 4          # mi_target_kind: the targets whose support is R^d
TOL, MAX_ITER = 1e-10, 1000
SUMMARY = ("logml", "status", "it", "rel", "lstar", "cv1", "cv2", "n_prop")


def _np_normal_vec(seed, i, d):
    return np.random.default_rng([int(seed), int(i), STREAM_BRIDGE]).standard_normal(d)


def _np_dot(a, b):
    return float(np.sum(np.asarray(a) * np.asarray(b)))


def _np_chol(S):
    try:
        return np.linalg.cholesky(S)
    except np.linalg.LinAlgError:                     # not positive definite: the engine's loop gives NaN from the first bad pivot on
        return np.full_like(S, np.nan)


def _np_inv(S):
    try:
        return np.linalg.inv(S)
    except np.linalg.LinAlgError:
        return np.full_like(S, np.nan)


NUMPY_MATH = dict(waic.NUMPY_MATH, dot=_np_dot, dot4=_np_dot, normal_vec=_np_normal_vec, chol_lower=_np_chol, inverse=_np_inv)

_m = waic._m


def _f(math, name, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.asarray(_m(math, name)(a.ravel()), dtype=np.float64).reshape(a.shape)


def columns(slab):
    """[n, d, C] -> [n * C, d]: row k = t * C + c is column (t, c)."""
    x = np.ascontiguousarray(slab, dtype=np.float64)
    n, d, C = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(n * C, d)


def sum4(a):
    """q[i % 4] = q[i % 4] + a_i, i ascending, each from +0; (q0 + q2) + (q1 + q3)."""
    q = np.zeros(4)
    for i, v in enumerate(np.asarray(a, dtype=np.float64)):
        q[i % 4] = q[i % 4] + v
    return (q[0] + q[2]) + (q[1] + q[3])


def log_kernel(kind, cols, prec=None, X=None, y=None, math=NUMPY_MATH):
    """mi_mcmc_draws_log_kernel's DEFINITION for the columns cols [N, d] -> [N]  (ISO, DIAG, DENSE, LOGISTIC)."""
    cols = np.ascontiguousarray(cols, dtype=np.float64)
    N, d = cols.shape
    dot, dot4 = _m(math, "dot"), _m(math, "dot4")
    out = np.empty(N)
    with np.errstate(all="ignore"):
        if kind == LOGISTIC:
            X = np.ascontiguousarray(X, dtype=np.float64)
            yv = np.ascontiguousarray(y, dtype=np.float64)
            eta = np.empty((N, X.shape[0]))
            for k in range(N):
                for r in range(X.shape[0]):
                    eta[k, r] = dot(X[r], cols[k])
            term = yv[None, :] * eta - _f(math, "softplus", eta)
            for k in range(N):
                out[k] = sum4(term[k]) - 0.5 * np.float64(dot4(cols[k], cols[k]))
            return out
        if kind == DENSE:
            P = np.ascontiguousarray(prec, dtype=np.float64).reshape(d, d)
        elif kind == DIAG:
            pd = np.ascontiguousarray(prec, dtype=np.float64).ravel()
        elif kind != ISO:
            raise ValueError(f"target kind {kind}: bridge sampling takes ISO, DIAG, DENSE and LOGISTIC")
        for k in range(N):
            x = cols[k]
            if kind == ISO:
                w = x
            elif kind == DIAG:
                w = pd * x
            else:
                w = np.array([dot(P[i], x) for i in range(d)])
            out[k] = -0.5 * np.float64(dot4(x, w))
    return out


def fit(fit_slab, math=NUMPY_MATH):
    """Steps A and B: dict of mean [d], cov [d, d], L, Pg (None with status 1), ldh, status."""
    x = np.ascontiguousarray(fit_slab, dtype=np.float64)
    d = x.shape[1]
    with np.errstate(all="ignore"):
        mu = covariance.mean_ref(x)
        S = covariance.covariance_ref(x, math)
        res = dict(mean=mu, cov=S, L=None, Pg=None, ldh=np.float64(np.nan), status=1)
        if not np.isfinite(S).all():
            return res
        L = np.array(_m(math, "chol_lower")(S), dtype=np.float64).reshape(d, d)
        Pg = np.array(_m(math, "inverse")(S), dtype=np.float64).reshape(d, d)
        if not (np.isfinite(L).all() and np.isfinite(Pg).all()):
            return res
        diag = np.ascontiguousarray(np.diag(L))
        if not (diag > 0.0).all():
            return res
        lg = _f(math, "log", diag)
        s = np.float64(0.0)
        for a in range(d):
            s = s + lg[a]
        ldh = s + (0.5 * np.float64(d)) * LOG_2PI
    res.update(L=np.tril(L), Pg=Pg, ldh=ldh, status=0)
    return res


def propose(fitted, N2, seed, math=NUMPY_MATH):
    """Step C: y [d, N2], y[a, i] = mu_a + (the chain over b = 0 .. a of L_ab z_b)."""
    mu, L = fitted["mean"], fitted["L"]
    d = mu.shape[0]
    dot, nv = _m(math, "dot"), _m(math, "normal_vec")
    y = np.empty((d, N2))
    for i in range(N2):
        z = np.asarray(nv(seed, i, d), dtype=np.float64)
        for a in range(d):
            y[a, i] = mu[a] + np.float64(dot(L[a, :a + 1], z[:a + 1]))
    return y


def logg(fitted, cols, math=NUMPY_MATH):
    """Step D: the proposal's log-density of the columns cols [N, d] -> [N]."""
    mu, Pg, ldh = fitted["mean"], fitted["Pg"], fitted["ldh"]
    cols = np.ascontiguousarray(cols, dtype=np.float64)
    N, d = cols.shape
    dot, dot4 = _m(math, "dot"), _m(math, "dot4")
    out = np.empty(N)
    with np.errstate(all="ignore"):
        for k in range(N):
            e = cols[k] - mu
            w = np.array([dot(Pg[a], e) for a in range(d)])
            out[k] = (-0.5 * np.float64(dot4(e, w))) - ldh
    return out


def split(draws, n_fit=0):
    """(fit part [n_fit, d, C], iteration part [n_it, d, C]) of a slab; n_fit 0: n_keep // 2."""
    x = np.ascontiguousarray(draws, dtype=np.float64)
    n_keep = x.shape[0]
    n_fit = int(n_fit) if n_fit else n_keep // 2
    if not 1 <= n_fit < n_keep:
        raise ValueError(f"n_fit = {n_fit} is not in 1 .. n_keep - 1 = {n_keep - 1}")
    return x[:n_fit], x[n_fit:]


def proposal_ref(draws, n_fit=0, n_prop=0, seed=0, math=NUMPY_MATH):
    """mi_mcmc_bridge_proposal: dict of prop [1, d, N2], logg_post [n_it, C], logg_prop [N2], mean, cov, status, ldh; all NaN with status 1."""
    head, tail = split(draws, n_fit)
    n_it, d, C = tail.shape
    N2 = int(n_prop) if n_prop else n_it * C
    f = fit(head, math)
    if f["status"] != 0:
        nan = np.float64(np.nan)
        return dict(prop=np.full((1, d, N2), nan), logg_post=np.full((n_it, C), nan), logg_prop=np.full(N2, nan), mean=np.full(d, nan), cov=np.full((d, d), nan),
                    status=1, ldh=nan, fit=f)
    y = propose(f, N2, seed, math)
    return dict(prop=y[None], logg_post=logg(f, columns(tail), math).reshape(n_it, C), logg_prop=logg(f, np.ascontiguousarray(y.T), math), mean=f["mean"], cov=f["cov"],
                status=0, ldh=f["ldh"], fit=f)


def sump(v):
    """SUMP: the pieces of 16 384 values, ascending from +0, of psis.tree_sum(piece) -- the body fold of psis.psis_rows."""
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for e0 in range(0, v.size, PIECE):
            s = s + psis.tree_sum(v[e0:e0 + PIECE])
    return s


def moments(f):
    """(mean, M2) of the values f in THE ORDER of mi_mcmc_draws_waic: waic.chunk_partials per chunk of 2 048, the merge of waic.row_stats."""
    f = np.ascontiguousarray(f, dtype=np.float64).ravel()[None, :]
    K = f.shape[1]
    with np.errstate(all="ignore"):
        n = mean = M2 = None
        for b, c0 in enumerate(range(0, K, waic.CHUNK)):
            part = f[:, c0:min(K, c0 + waic.CHUNK)]
            nb = np.float64(part.shape[1])
            sh, _, S1, S2 = waic.chunk_partials(part, waic.NUMPY_MATH)     # (A, the sum of exp, is not used: numpy's exp will do)
            mb = sh + S1 / nb
            M2b = S2 - (S1 * S1) / nb
            if b == 0:
                n, mean, M2 = nb, mb, M2b
            else:
                delta = mb - mean
                nn = n + nb
                mean = mean + delta * (nb / nn)
                M2 = (M2 + M2b) + (delta * delta) * ((n * nb) / nn)
                n = nn
    return mean[0], M2[0]


def estimate_ref(logp_post, logg_post, logp_prop, logg_prop, n_eff=0.0, tol=0.0, max_iter=0, math=NUMPY_MATH):
    """mi_mcmc_bridge_estimate: dict of f2 [n_it, C] and summary [8] = (logml, status, it, rel, l*, cv1, cv2, N2)."""
    lp1 = np.ascontiguousarray(logp_post, dtype=np.float64)
    n_it, C = lp1.shape
    N1 = n_it * C
    lp2 = np.ascontiguousarray(logp_prop, dtype=np.float64).ravel()
    N2 = lp2.size
    n_eff = np.float64(n_eff) if n_eff else np.float64(N1)
    tol = np.float64(tol) if tol else np.float64(TOL)
    max_iter = int(max_iter) if max_iter else MAX_ITER
    with np.errstate(all="ignore"):
        l1 = lp1 - np.ascontiguousarray(logg_post, dtype=np.float64).reshape(n_it, C)
        l2 = lp2 - np.ascontiguousarray(logg_prop, dtype=np.float64).ravel()
        lstar = np.float64(quantiles.quantiles_ref(l1.reshape(n_it, 1, C), [0.5])[0, 0])
        n1, n2 = np.float64(N1), np.float64(N2)
        s1 = n_eff / (n_eff + n2)
        s2 = n2 / (n_eff + n2)
        a = _f(math, "exp", l2 - lstar)
        b = _f(math, "exp", (l1 - lstar).ravel())
        r, it = np.float64(1.0), 0
        while True:
            s2r = s2 * r
            num = sump(a / (s1 * a + s2r)) / n2
            den = sump(1.0 / (s1 * b + s2r)) / n1
            rn = num / den
            it += 1
            rel = np.abs(rn - r) / np.abs(rn)
            r = rn
            if not (np.isfinite(r) and r > 0.0):
                status = 3
                break
            if rel <= tol:
                status = 0
                break
            if it == max_iter:
                status = 2
                break
        s2r = s2 * r
        f1 = a / (s1 * a + s2r)
        f2 = 1.0 / (s1 * b + s2r)
        m1, M21 = moments(f1)
        m2, M22 = moments(f2)
        cv1 = (M21 / np.float64(N2 - 1)) / ((m1 * m1) * n2)
        cv2 = (M22 / np.float64(N1 - 1)) / ((m2 * m2) * n1)
        logml = _f(math, "log", np.array([r]))[0] + lstar
    return dict(f2=f2.reshape(n_it, C), summary=np.array([logml, status, it, rel, lstar, cv1, cv2, n2]))


def bridge_ref(kind, draws, prec=None, X=None, y=None, n_fit=0, n_prop=0, seed=0, n_eff=0.0, tol=0.0, max_iter=0, math=NUMPY_MATH):
    """mi_mcmc_draws_bridge: dict of f2, mean, cov, summary (and the pieces: proposal, logp_post, logp_prop).  Status 1: summary = (NaN, 1, NaN, ..., N2)."""
    p = proposal_ref(draws, n_fit, n_prop, seed, math)
    _, tail = split(draws, n_fit)
    n_it, d, C = tail.shape
    N2 = p["logg_prop"].size
    if p["status"] != 0:
        nan = np.float64(np.nan)
        return dict(f2=np.full((n_it, C), nan), mean=p["mean"], cov=p["cov"], summary=np.array([nan, 1.0, nan, nan, nan, nan, nan, np.float64(N2)]), proposal=p,
                    logp_post=None, logp_prop=None)
    lp1 = log_kernel(kind, columns(tail), prec, X, y, math).reshape(n_it, C)
    lp2 = log_kernel(kind, np.ascontiguousarray(p["prop"][0].T), prec, X, y, math)
    e = estimate_ref(lp1, p["logg_post"], lp2, p["logg_prop"], n_eff, tol, max_iter, math)
    return dict(f2=e["f2"], mean=p["mean"], cov=p["cov"], summary=e["summary"], proposal=p, logp_post=lp1, logp_prop=lp2)


def rel_mse(summary, n_it, ess_per_chain):
    """Fruehwirth-Schnatter's relative mean-squared error of the estimate of Z: cv1 + (n_it / ESS) * cv2, ESS the per-chain effective size of f2 (ess.py,
    mi_mcmc_draw_stats) -- N1 / (C ESS) is n_it / ESS.  Its root is the approximate standard error of logml."""
    s = np.asarray(summary, dtype=np.float64)
    return s[5] + (np.float64(n_it) / np.float64(ess_per_chain)) * s[6]
