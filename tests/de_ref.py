"""CPU reference of mcmc::de (ref: src/de.cpp:28-232) under the engine's RNG contract (include/mi_mcmc.h, mi_mcmc_de_run).

A transcription of de_impl with omp_n_threads = 1 -- members swept in order, in place -- on what the oracle already exports:
the built-in targets (orc_target_kernel through orc.TargetSpec, W = 4 and the literal kernels' blocked orders), Philox
(orc_philox_eval), log (orc_math_eval), and the box transforms.  One population per call; `pop` is its global id.
"""
import ctypes as C
import math

import numpy as np

import orc

STREAM_DE_INIT, STREAM_DE = 3, 4
_ip = C.POINTER(C.c_int)


def de_blocks(d):
    """Philox blocks per member and generation: block 0 (partners, z) and one per pair of dimensions"""
    return 1 + (d + 1) // 2


def block(seed, pop, gen, slot, tag):
    return orc.philox([pop & 0xffffffff, gen, slot, tag | ((pop >> 32) << 8)], [seed & 0xffffffff, seed >> 32])


def u01(lo, hi):
    k = ((int(hi) << 32) | int(lo)) >> 12
    return float(2 * k + 1) * 2.0 ** -53


def partners(w, i, n_pop):
    c1 = (int(w[0]) * (n_pop - 1)) >> 32
    c1 += c1 >= i
    lo, hi = min(i, c1), max(i, c1)
    c2 = (int(w[1]) * (n_pop - 2)) >> 32
    c2 += c2 >= lo
    c2 += c2 >= hi
    return c1, c2


def uniforms(seed, pop, gen, member, d, tag):
    """u_k of dimensions 0..d-1 of one member: blocks 1..ceil(d/2) of its slots"""
    nb = de_blocks(d)
    u = np.empty(d)
    for blk in range(1, nb):
        w = block(seed, pop, gen, member * nb + blk, tag)
        k = 2 * (blk - 1)
        u[k] = u01(w[0], w[1])
        if k + 1 < d:
            u[k + 1] = u01(w[2], w[3])
    return u


def gamma(d):
    return 2.38 / math.sqrt(2.0 * d)                      # de.cpp:61-62 (par_gamma is not read)


def gamma_at(gen, d, jumps, gamma_jump):
    return gamma_jump if (jumps and (gen + 1) % 10 == 0) else gamma(d)


def log(x):
    return orc.math_eval(1, np.array([x]))[0]


def target_spec(kind, d, prec=None, X=None, y=None):
    """The built-in target in the reduction orders the device kernels use (literal_host.hpp: lit_orders)"""
    if kind == orc.TARGET_LOGISTIC and d <= 512:
        bs = 16 if d <= 64 else 32 if d <= 128 else 64 if d <= 256 else 128
        return orc.TargetSpec(kind, d, X=X, y=y, W=4, blocks=4, block_size=bs, eta_chains=2)
    if kind == orc.TARGET_DENSE and 128 < d <= 512:
        bs = 48 if d <= 192 else 64 if d <= 256 else 96 if d <= 384 else 128
        return orc.TargetSpec(kind, d, prec=prec, W=4, blocks=4, block_size=bs)
    return orc.TargetSpec(kind, d, prec=prec, X=X, y=y, W=4)


class Bounds:
    def __init__(self, d, lower=None, upper=None):
        self.d, self.on = d, lower is not None
        self.lb = np.ascontiguousarray(lower if self.on else np.zeros(d), dtype=np.float64)
        self.ub = np.ascontiguousarray(upper if self.on else np.zeros(d), dtype=np.float64)
        self.bt = np.ones(d, dtype=np.int32)
        orc.lib().orc_determine_bounds_type(int(self.on), C.c_size_t(d), orc._p(self.lb), orc._p(self.ub), self.bt.ctypes.data_as(_ip))

    def inv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty(self.d)
        orc.lib().orc_inv_transform(orc._p(x), self.bt.ctypes.data_as(_ip), orc._p(self.lb), orc._p(self.ub), C.c_size_t(self.d), orc._p(out))
        return out

    def log_jacobian(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        return orc.lib().orc_log_jacobian(orc._p(x), self.bt.ctypes.data_as(_ip), orc._p(self.lb), orc._p(self.ub), C.c_size_t(self.d))


def initial_box(init, d, bounds, initial_lb=None, initial_ub=None):
    """de.cpp:65-68 with sampling_bounds_check (bounds_check.hpp:37-48)"""
    init = np.asarray(init, dtype=np.float64)
    lo = np.array(initial_lb, dtype=np.float64) if initial_lb is not None else init + -0.5
    hi = np.array(initial_ub, dtype=np.float64) if initial_ub is not None else init + 0.5
    if bounds.on:
        for k in range(d):
            if bounds.bt[k] in (2, 4):
                lo[k] = lo[k] if bounds.lb[k] < lo[k] else bounds.lb[k]      # std::max(hard, sampling)
            if bounds.bt[k] in (3, 4):
                hi[k] = hi[k] if hi[k] < bounds.ub[k] else bounds.ub[k]      # std::min(hard, sampling)
    return lo, hi


def de_ref(log_kernel, init, n_pop, n_burnin, n_keep, seed=0, pop=0, lower=None, upper=None, jumps=False, par_b=1e-4,
           par_gamma_jump=2.0, initial_lb=None, initial_ub=None, draw0=0, population=None, want_draws=True):
    """One population.  log_kernel(x) -> value (a TargetSpec's kernel or any Python function of the untransformed values).
    population: [n_pop, d] in the sampler's space to continue at generation draw0.  Returns (draws [n_keep, n_pop, d] or None,
    final population [n_pop, d] (transformed space), n_accept)."""
    init = np.asarray(init, dtype=np.float64)
    d = init.size
    if n_pop < 3:
        raise ValueError("n_pop >= 3")
    if isinstance(log_kernel, orc.TargetSpec):
        spec = log_kernel
        log_kernel = lambda x: spec.kernel(x, want_grad=False)[0]
    bd = Bounds(d, lower, upper)

    def box_log_kernel(x):                               # de.cpp:101-112
        v = log_kernel(bd.inv(x)) + bd.log_jacobian(x) if bd.on else log_kernel(x)
        return v if math.isfinite(v) else -math.inf

    if draw0 == 0:
        lo, hi = initial_box(init, d, bd, initial_lb, initial_ub)
        X = np.array([lo + (hi - lo) * uniforms(seed, pop, 0, i, d, STREAM_DE_INIT) for i in range(n_pop)])
    else:
        X = np.array(population, dtype=np.float64, copy=True)
    tv = np.array([box_log_kernel(X[i]) for i in range(n_pop)])
    draws = np.zeros((n_keep, n_pop, d)) if want_draws else None
    nb = de_blocks(d)
    n_accept = 0
    for g in range(n_burnin + n_keep):
        gen = draw0 + g
        gam = gamma_at(gen, d, jumps, par_gamma_jump)
        for i in range(n_pop):
            w = block(seed, pop, gen, i * nb, STREAM_DE)
            c1, c2 = partners(w, i, n_pop)
            z = u01(w[2], w[3])
            r = -par_b + (par_b + par_b) * uniforms(seed, pop, gen, i, d, STREAM_DE)
            prop = (X[i] + (X[c1] - X[c2]) * gam) + r
            pv = box_log_kernel(prop)
            with np.errstate(invalid="ignore"):
                accept = bool(pv - tv[i] > log(z))
            if accept:
                X[i] = prop
                tv[i] = pv
                if g >= n_burnin:
                    n_accept += 1
        if g >= n_burnin and want_draws:
            draws[g - n_burnin] = np.array([bd.inv(x) for x in X]) if bd.on else X
    return draws, X, n_accept
