"""GPU: every sampler route with mi_chains.mem = MI_MEM_DEVICE on a caller's non-blocking stream -- what bench.py, mcmc_amd.dist and production callers do, and
what the parity tests (host-staged, NULL stream, freshly allocated outputs, a synchronisation before anything is read) never see.  tests/device_resident.py
puts every output between guards, fills outputs and inputs with sentinels, produces the inputs on the stream behind work that takes a while, and waits for the
stream alone.  Per route: the kernel that ran, the oracle's bits (configured as the route's parity test configures it: their helpers, imported), the
host-staged call's bits for every output, the guards, and the header's contract for the outputs (include/mi_mcmc.h: mi_chains)."""
import functools

import numpy as np
import pytest
import torch

import device_resident as dr
import mcmc_amd
import orc
import test_gpu_lds_bounds as p_ldsb
import test_gpu_mass_adapt as p_mass
import test_gpu_parity_dense_lds as p_dlds
import test_gpu_parity_gemm_bounds as p_gb
import test_gpu_parity_gemm_dense_m as p_gm
import test_gpu_parity_gemm_nuts as p_gn
import test_gpu_parity_hmc as p_hmc
import test_gpu_parity_mala as p_mala
import test_gpu_parity_nuts as p_nuts
import test_gpu_parity_nuts_lds as p_nlds
import test_gpu_parity_rwmh as p_rwmh
import test_gpu_parity_small as p_small
import test_gpu_parity_small_logistic as p_slog
from mcmc_amd import synth

pytestmark = pytest.mark.gpu

ORC_ALGO = {"hmc": orc.ALGO_HMC, "mala": orc.ALGO_MALA, "rwmh": orc.ALGO_RWMH, "nuts": orc.ALGO_NUTS, "rmhmc": orc.ALGO_RMHMC}
GK = {"iso": mcmc_amd.TARGET_GAUSS_ISO, "diag": mcmc_amd.TARGET_GAUSS_DIAG, "dense": mcmc_amd.TARGET_GAUSS_DENSE}
OK_ = {"iso": orc.TARGET_ISO, "diag": orc.TARGET_DIAG, "dense": orc.TARGET_DENSE}
_O = dict(rng_seed_value="seed", n_burnin_draws="n_burnin", n_keep_draws="n_keep", n_leap_steps="n_leap", step_size="step", n_adapt_draws="n_adapt",
          max_tree_depth="max_depth", precond_mat="precond", lower_bounds="lower", upper_bounds="upper", n_fp_steps="n_fp")
N_DEPTH_CHAINS = 8          # chains whose depth trace is held to the oracle (one oracle run per chain: run_many returns no trace)


def oracle_settings(skw, **extra):
    """the oracle's settings from the library's, field by field"""
    return orc.make_settings(**{_O[k]: v for k, v in skw.items() if k in _O}, **extra)


class Case:
    """algo, the library's target (kind, tkw), init [C, d], the settings' keywords, the oracle's target and what its settings take beyond the library's
    (W, hoist, blocks, block_size), what last_kernel() must say, and what the route's parity test asserts of the accept counts:
    "some" 0 < sum, "both" 0 < sum < keep C, "leq" 0 < sum <= keep C, None nothing"""

    def __init__(self, algo, kind, tkw, init, skw, spec, oextra, kernel, chain0=0, hint=mcmc_amd.KERNEL_AUTO, mass_diag=None, mixed=None, oracle=None, memo=False):
        self.algo, self.kind, self.tkw, self.init, self.skw, self.spec, self.oextra = algo, kind, tkw, np.ascontiguousarray(init), dict(skw), spec, dict(oextra)
        self.kernel, self.chain0, self.hint, self.mass_diag, self.mixed, self.custom_oracle, self.memo = kernel, chain0, hint, mass_diag, mixed, oracle, memo

    def settings(self, **over):
        return mcmc_amd.default_settings(**{**self.skw, **over})

    def n_draws(self):
        return int(self.skw["n_burnin_draws"]), int(self.skw["n_keep_draws"])

    def oracle(self, init=None):
        init = self.init if init is None else init
        if self.custom_oracle is not None:
            return self.custom_oracle(self, init)
        o_draws, o = orc.run_many(ORC_ALGO[self.algo], self.spec, init, oracle_settings(self.skw, **self.oextra), chain0=self.chain0)
        if self.algo == "nuts":
            n = min(init.shape[0], N_DEPTH_CHAINS)
            o["depth_first"] = np.stack([orc.run_chain(orc.ALGO_NUTS, self.spec, init[c], oracle_settings(self.skw, chain_id=self.chain0 + c, **self.oextra),
                                                       traces=True)[1]["depth"] for c in range(n)], axis=1)
        return o_draws, o

    def host(self, init=None, st=None, **kw):
        """the host-staged call of the same case: mcmc_amd.sample (NULL stream, fresh buffers)"""
        init = self.init if init is None else init
        st = self.settings() if st is None else st
        if self.mass_diag is None:
            return mcmc_amd.sample(self.algo, self.kind, init, st, chain0=self.chain0, kernel_hint=self.hint, want_adapt_state=self.algo == "nuts", **self.tkw, **kw)
        C, d = init.shape                                  # (sample() has no mass_diag: its lines with one more array)
        theta = np.ascontiguousarray(init.T.copy()); draws = np.zeros((int(st.n_keep_draws), d, C))
        g = dict(n_accept=np.zeros(C, dtype=np.uint64), n_leap=np.zeros(C, dtype=np.uint64), n_exec=np.zeros(C, dtype=np.uint64), eps=np.zeros(C), theta=theta,
                 depth=None, adapt_state=None)
        t = mcmc_amd.make_target(self.kind, d, kernel_hint=self.hint, **self.tkw)
        mcmc_amd.run(self.algo, t, st, mcmc_amd.make_chains(theta, C, chain0=self.chain0, draws=draws, n_accept=g["n_accept"], n_leapfrogs=g["n_leap"],
                                                            n_leapfrogs_executed=g["n_exec"], step_size=g["eps"], mass_diag=self.mass_diag))
        return draws, g

    def device(self, stream, init=None, st=None, **kw):
        init = self.init if init is None else init
        st = self.settings() if st is None else st
        return dr.run_case(stream, self.algo, self.kind, init, st, chain0=self.chain0, kernel_hint=self.hint, mass_diag=self.mass_diag, **self.tkw, **kw)

    def device_call(self, init=None, st=None, **kw):
        init = self.init if init is None else init
        st = self.settings() if st is None else st
        return dr.Call(self.algo, self.kind, init, st, chain0=self.chain0, kernel_hint=self.hint, mass_diag=self.mass_diag, **self.tkw, **kw)


def S(seed, burn, keep, **kw):
    return dict(rng_seed_value=seed, n_burnin_draws=burn, n_keep_draws=keep, **kw)


def _starts(*prefixes, has=(), ends=None):
    def check(name):
        return name.startswith(prefixes) and all(h in name for h in has) and (ends is None or name.endswith(ends))
    return check


def _logit_blk(d):
    return dict(blocks=4, block_size=p_nlds._bs("logistic", d))


def _logit(d, N, seed, C, init_seed, scale):
    X, y = synth.logistic_problem(d, N, seed=seed)
    spec = orc.TargetSpec(orc.TARGET_LOGISTIC, d, X=X, y=y, W=4, eta_chains=2, **_logit_blk(d))
    return dict(X=X, y=y), spec, synth.initial_states(C, d, seed=init_seed) * scale


def _gauss(kind, d, prec, **okw):
    return GK[kind], dict(prec=prec), orc.TargetSpec(OK_[kind], d, prec=prec, W=4, **okw)


def _bounds_kw(lb, ub):
    return dict(vals_bound=1, lower_bounds=lb, upper_bounds=ub)


def _normal_model(n, C):
    x = p_small._data(n, seed=n)
    return dict(y=x), orc.TargetSpec(orc.TARGET_NORMAL_MODEL, 2, y=x, W=1), p_small._init(C, seed=C)


# ---------------------------------------------------------------- the table: d at the route's lower edge, C <= 70 and no multiple of 16, at most 10 draws
def _hmc_dense(d, L, eps, burn, keep):
    k, tkw, spec = _gauss("dense", d, synth.dense_gaussian_precision(d, seed=5))
    return Case("hmc", k, tkw, synth.initial_states(37, d, seed=11), S(1234, burn, keep, n_leap_steps=L, step_size=eps), spec, dict(W=4),
                _starts("hmc_gauss_mfma_kernel<", "hmc_gauss_split_kernel<"), chain0=1000)


def _hmc_diag_d24():
    d = 24
    k, tkw, spec = _gauss("diag", d, synth.ill_conditioned_diag(d, 100.0))
    return Case("hmc", k, tkw, synth.initial_states(37, d, seed=11), S(1234, 4, 6, n_leap_steps=8, step_size=0.02), spec, dict(W=4),
                _starts("hmc_gauss_mfma_kernel<"), chain0=1000)


def _hmc_diag_d200():
    d = 200
    k, tkw, spec = _gauss("diag", d, synth.ill_conditioned_diag(d, 1.0e4))
    return Case("hmc", k, tkw, synth.initial_states(37, d, seed=12), S(55, 3, 5, n_leap_steps=6, step_size=0.01), spec, dict(W=4), _starts("hmc_diag"), chain0=9)


def _hmc_d24_bounds_dense_m():
    d, C = 24, 37
    k, tkw, spec = _gauss("dense", d, synth.dense_gaussian_precision(d, seed=5))
    M = p_hmc._spd(d, seed=d)
    lb, ub = p_hmc._bounds(d, seed=4)
    init = np.clip(synth.initial_states(C, d, seed=16) * 0.3, -1.0, 1.5)
    return Case("hmc", k, tkw, init, S(8, 3, 7, n_leap_steps=4, step_size=0.05, precond_mat=M, **_bounds_kw(lb, ub)), spec, dict(W=4),
                _starts("hmc_gauss_mfma_kernel<", ends=", true, true, false>"), chain0=2, mixed="some")


def _hmc_d20_chain_mass():
    d, C, burn, keep, L, eps = 20, 21, 3, 6, 5, 0.2
    prec = synth.dense_gaussian_precision(d, seed=4)
    k, tkw, spec = _gauss("dense", d, prec)
    init = np.clip(synth.initial_states(C, d, seed=3) * 0.5, -1.0, 1.5)
    mass = np.ascontiguousarray(np.random.default_rng(7).uniform(0.2, 5.0, (d, C)))

    def oracle(case, init_):
        o_draws, nacc = p_mass._oracle_per_chain(orc.TARGET_DENSE, d, prec, init_, mass, 9, burn, keep, L, eps)
        return o_draws, dict(n_accept=nacc)
    return Case("hmc", k, tkw, init, S(9, burn, keep, n_leap_steps=L, step_size=eps), spec, dict(W=4), _starts("hmc_gauss_mfma_kernel<", ends="true, true>"),
                mass_diag=mass, mixed="some", oracle=oracle)


def _hmc_logit_d70():
    d = 70
    tkw, spec, init = _logit(d, 60, 4, 37, 41, 0.1)
    return Case("hmc", mcmc_amd.TARGET_LOGISTIC, tkw, init, S(77, 2, 6, n_leap_steps=4, step_size=0.02), spec, dict(W=4, hoist=1, **_logit_blk(d)),
                _starts("logit_lds_kernel<"), chain0=5)


def _hmc_logit_d70_bounds_diag_m():
    d, C = 70, 37
    k, tkw, spec = p_nlds._problem("logistic", d, 60, seed=d + 2)
    lb, ub = p_ldsb._bounds(d, d)
    init = np.clip(synth.initial_states(C, d, seed=d + 4) * 0.1, -1.0, 1.5)
    M = np.diag(np.random.default_rng(d + 1).uniform(0.4, 2.5, d))
    return Case("hmc", k, tkw, init, S(17, 2, 4, n_leap_steps=4, step_size=0.05, precond_mat=M, **_bounds_kw(lb, ub)), spec, dict(W=4, hoist=1, **_logit_blk(d)),
                _starts("logit_lds_kernel<", ends="true, true>"), chain0=6, mixed="some")


def _hmc_d130_dense_m():
    d, C = 130, 37
    prec = synth.dense_gaussian_precision(d, seed=d % 89)
    k, tkw, spec = _gauss("dense", d, prec, **p_dlds._blk(d))
    return Case("hmc", k, tkw, synth.initial_states(C, d, seed=d + 1) * 0.5, S(3, 2, 4, n_leap_steps=3, step_size=0.3, precond_mat=p_dlds._dense_m(d, d)), spec,
                dict(W=4, hoist=1, **p_dlds._blk(d)), _starts("logit_lds_kernel<", ends="1, false, false, true>"), chain0=11, mixed="both")


def _gemm(algo, variant):
    """d = 520 on the matrix-product route: plain, logistic, a dense precond_mat, bounds (tests/test_gpu_parity_gemm*.py)"""
    d, C, L = 520, 37, 3
    eps = {"hmc": 0.02, "mala": 0.03, "rwmh": 0.012}[algo]
    has, kw, mixed, chain0 = (), {}, "some", 11
    if variant == "logit":
        k, tkw, spec, init = p_gm._problem("logit", d, 40, C)
        has = (", 1>",)
    elif variant == "bounds":
        k, tkw, spec, init = p_gb._problem("dense", d, 0, C)
        lo, hi = p_gb.bounds(d, "a")
        kw, has, mixed, chain0, eps = _bounds_kw(lo, hi), ("bounds",), "both", 0, p_gb.STEP
    else:
        k, tkw, spec, init = p_gm._problem("dense", d, 0, C)
        if variant == "dense_m":
            kw, has, mixed, chain0, eps = dict(precond_mat=p_gm.dense_mass(d, d + 1)), ("dense precond_mat",), "both", 0, p_gm.MIXED[("dense", algo)]
    keep = 6 if variant in ("bounds", "dense_m") else 4
    return Case(algo, k, tkw, init, S(7, 2, keep, n_leap_steps=L, step_size=eps, **kw), spec, dict(W=4, hoist=1), _starts("gemm_step_kernel<", has=has),
                chain0=chain0, mixed=mixed)


def _hmc_d150_bounds_dense_m():
    d, C = 150, 21
    prec = synth.dense_gaussian_precision(d, seed=3)
    k, tkw, spec = _gauss("dense", d, prec, **p_dlds._blk(d))
    lb = np.full(d, -np.inf); ub = np.full(d, np.inf); lb[::3] = -1.5; ub[::5] = 2.0
    init = np.clip(synth.initial_states(C, d, seed=4) * 0.5, -1.0, 1.5)
    return Case("hmc", k, tkw, init, S(5, 1, 3, n_leap_steps=3, step_size=0.04, precond_mat=p_dlds._dense_m(d, 1), **_bounds_kw(lb, ub)), spec,
                dict(W=4, hoist=1, **p_dlds._blk(d)), _starts("literal_kernel<0>"))


def _small_normal(algo):
    tkw, spec, init = _normal_model(257 if algo != "rmhmc" else 1000, 70 if algo == "rmhmc" else 37)
    if algo == "hmc":
        return Case(algo, mcmc_amd.TARGET_NORMAL_MODEL, tkw, init, S(17, 2, 8, n_leap_steps=5, step_size=0.03), spec, dict(W=1, hoist=0),
                    _starts("hmc_small_kernel<NormalModel>"), chain0=5, mixed="both")
    if algo == "nuts":
        return Case(algo, mcmc_amd.TARGET_NORMAL_MODEL, tkw, init, S(23, 5, 5, step_size=1.0, n_adapt_draws=6, max_tree_depth=5), spec, dict(W=1),
                    _starts("nuts_small_kernel<NormalModel>"), chain0=11)
    return Case(algo, mcmc_amd.TARGET_NORMAL_MODEL, tkw, init, S(41, 3, 7, n_leap_steps=1, step_size=0.02, n_fp_steps=5), spec, dict(W=1),
                _starts("rmhmc_small_kernel<NormalModel>"), chain0=123, mixed="both")


def _hmc_logit_d5_bounds():
    d, N, C, burn, keep, L, eps = 5, 40, 37, 3, 7, 6, 0.05
    X, y = synth.logistic_problem(d, N, seed=4)
    init = synth.initial_states(C, d, seed=41) * 0.3
    bd = p_slog._bounds(d, "box")

    def oracle(case, init_):
        o_draws, o = p_slog._oracle("hmc", d, X, y, init_, 11, bounds=bd, seed=321, n_burnin=burn, n_keep=keep, n_leap=L, step=eps, n_adapt=burn, max_depth=7)
        return o_draws, dict(n_accept=o["n_accept"].astype(np.uint64), n_leap=o["n_leap"].astype(np.uint64))
    return Case("hmc", mcmc_amd.TARGET_LOGISTIC, dict(X=X, y=y), init, S(321, burn, keep, n_leap_steps=L, step_size=eps, n_adapt_draws=burn, max_tree_depth=7,
                                                                         **_bounds_kw(*bd)), None, {}, _starts("hmc_small_kernel<LogisticSmallModel<5>>"),
                chain0=11, mixed="some", oracle=oracle)


def _mala_dense(d, dense_m):
    C = 37
    if dense_m:
        k, tkw, spec = _gauss("dense", d, synth.dense_gaussian_precision(d, seed=5))
        return Case("mala", k, tkw, synth.initial_states(C, d, seed=15) * 0.3, S(6, 3, 7, step_size=0.15, precond_mat=p_mala._spd(d, seed=d)), spec,
                    dict(W=4, hoist=1), _starts("mala_gauss_dense_m_kernel<"), chain0=1, mixed="some")
    k, tkw, spec = _gauss("dense", d, synth.dense_gaussian_precision(d, seed=7))
    return Case("mala", k, tkw, synth.initial_states(C, d, seed=31), S(99, 3, 7, step_size=0.15), spec, dict(W=4, hoist=1), _starts("mala_gauss_mfma_kernel<"), chain0=77)


def _mala_logit_d70():
    d = 70
    tkw, spec, init = _logit(d, 60, 4, 37, 41, 0.1)
    return Case("mala", mcmc_amd.TARGET_LOGISTIC, tkw, init, S(123, 3, 7, step_size=0.05), spec, dict(W=4, hoist=1, **_logit_blk(d)), _starts("logit_lds_kernel<"), chain0=3)


def _mala_d150_bounded():
    d, C = 150, 21
    prec = synth.dense_gaussian_precision(d, seed=d)
    k, tkw, spec = _gauss("dense", d, prec, **p_dlds._blk(d))
    lb, ub = p_ldsb._bounds(d, d)
    init = np.clip(synth.initial_states(C, d, seed=d + 1) * 0.5, -1.0, 1.5)
    return Case("mala", k, tkw, init, S(3, 2, 4, step_size=0.1, **_bounds_kw(lb, ub)), spec, dict(W=4, hoist=1, **p_dlds._blk(d)), _starts("literal_kernel<1>"), chain0=5)


def _rwmh_d37_bounds():
    d, C = 37, 21
    k, tkw, spec = _gauss("dense", d, synth.dense_gaussian_precision(d, seed=7))
    lb, ub = p_rwmh._bounds(d, seed=d)
    init = np.clip(synth.initial_states(C, d, seed=31) * 0.4, -1.0, 1.5)
    return Case("rwmh", k, tkw, init, S(99, 2, 8, step_size=0.10, **_bounds_kw(lb, ub)), spec, dict(W=4), _starts("rwmh_gauss_mfma_kernel<"), chain0=77, mixed="leq")


def _rwmh_logit_d100():
    d = 100
    tkw, spec, init = _logit(d, 33, 4, 37, 41, 0.1)
    return Case("rwmh", mcmc_amd.TARGET_LOGISTIC, tkw, init, S(123, 2, 6, step_size=0.03), spec, dict(W=4, **_logit_blk(d)), _starts("logit_lds_kernel<"),
                chain0=3, mixed="both")


def _nuts_d32(hint):
    d, C = 32, 37
    k, tkw, spec = _gauss("dense", d, synth.dense_gaussian_precision(d, seed=6))
    memo = hint == mcmc_amd.KERNEL_AUTO
    return Case("nuts", k, tkw, synth.initial_states(C, d, seed=21), S(77, 4, 4, n_adapt_draws=5, max_tree_depth=5, step_size=1.0), spec, dict(W=4),
                _starts("nuts_gauss_memo_kernel" if memo else "nuts_gauss_async_kernel"), chain0=500, hint=hint, memo=memo)


def _nuts_general(d, dense_m):
    C = 21
    prec = synth.dense_gaussian_precision(d, seed=5)
    k, tkw, spec = _gauss("dense", d, prec)
    init = np.clip(synth.initial_states(C, d, seed=14) * 0.3, -1.0, 1.5)
    if dense_m:
        return Case("nuts", k, tkw, init, S(80, 4, 4, n_adapt_draws=4, max_tree_depth=5, precond_mat=p_nuts._spd(d, seed=d)), spec, dict(W=4),
                    _starts("nuts_gauss_async_kernel<", ends="true, true>"), chain0=4)
    lb, ub = p_nuts._bounds(d, seed=d)
    return Case("nuts", k, tkw, init, S(79, 4, 4, n_adapt_draws=4, max_tree_depth=5, **_bounds_kw(lb, ub)), spec, dict(W=4),
                _starts("nuts_tile_kernel<built-in Gaussian"), chain0=4, memo=True)


def _nuts_lds(kind, d, n_rows):
    C = 21
    k, tkw, spec = p_nlds._problem(kind, d, n_rows, seed=d)
    init = synth.initial_states(C, d, seed=d + 1) * (0.1 if kind == "logistic" else 0.5)
    return Case("nuts", k, tkw, init, S(7, 3, 3, n_adapt_draws=4, max_tree_depth=5, step_size=0.05 if kind == "logistic" else 0.1), spec,
                dict(W=4, blocks=4, block_size=p_nlds._bs(kind, d)), _starts("logit_lds_kernel<", has=("nuts",)), chain0=3, memo=True)


def _nuts_d520(bounded):
    d, C = 520, 21
    if bounded:
        k, tkw, spec, init = p_gb._problem("dense", d, 0, C)
        kw, has = _bounds_kw(*p_gb.bounds(d, "a")), ("nuts", "memoised", "bounds")
    else:
        k, tkw, spec, init = p_gn._problem("dense", d, 0, C)
        kw, has = {}, ("nuts", "memoised")
    return Case("nuts", k, tkw, init, S(p_gn.SEED, 2, 4, n_adapt_draws=3, max_tree_depth=5, step_size=p_gn.STEP, **kw), spec, dict(W=4, hoist=1),
                _starts("gemm_step_kernel<", has=has), memo=True, mixed="both")


def _nuts_d150_dense_m_literal():
    d, C = 150, 9
    prec = synth.dense_gaussian_precision(d, seed=d % 89)
    k, tkw, spec = _gauss("dense", d, prec, **p_dlds._blk(d))
    return Case("nuts", k, tkw, synth.initial_states(C, d, seed=d + 1) * 0.5, S(3, 2, 3, n_adapt_draws=3, max_tree_depth=4, step_size=0.1, precond_mat=p_dlds._dense_m(d, d)),
                spec, dict(W=4, hoist=1, **p_dlds._blk(d)), _starts("literal_kernel<2>"), chain0=5, hint=mcmc_amd.KERNEL_LITERAL)


def _rmhmc_logit_d3():
    d, C = 3, 37
    X, y = synth.logistic_problem(d, 60, seed=8)
    spec = orc.TargetSpec(orc.TARGET_LOGISTIC, d, X=X, y=y, W=4, blocks=4, block_size=16, eta_chains=2)
    return Case("rmhmc", mcmc_amd.TARGET_LOGISTIC, dict(X=X, y=y), synth.initial_states(C, d, seed=7) * 0.3, S(43, 3, 7, step_size=0.05, n_leap_steps=2, n_fp_steps=5),
                spec, dict(W=4, blocks=4, block_size=16), _starts("rmhmc_small_kernel<LogisticSmallModel<3>>"), chain0=5, mixed="some")


def _rmhmc_dense_d6():
    d, C = 6, 9
    k, tkw, spec = _gauss("dense", d, synth.dense_gaussian_precision(d, seed=3))
    return Case("rmhmc", k, tkw, synth.initial_states(C, d, seed=7) * 0.4, S(11, 2, 6, step_size=0.1, n_leap_steps=2, n_fp_steps=3), spec, dict(W=4),
                _starts("literal_kernel<4>"), chain0=2)


CASES = {  # case: what builds it                                             # the kernel it runs on an MI355X (mi_mcmc_last_kernel())
    "hmc_dense_d20": lambda: _hmc_dense(20, 4, 0.10, 3, 6),             # hmc_gauss_mfma_kernel<2, 8, false, false, false>
    "hmc_dense_d100": lambda: _hmc_dense(100, 3, 0.05, 2, 5),           # hmc_gauss_split_kernel<8, 4, 4>
    "hmc_diag_d24": _hmc_diag_d24,                                      # hmc_gauss_mfma_kernel<2, 8, false, false, false> (mi_mcmc.hip: dense_precision_on_device)
    "hmc_diag_d200": _hmc_diag_d200,                                    # hmc_diag4_kernel<false>
    "hmc_dense_d24_bounds_dense_m": _hmc_d24_bounds_dense_m,            # hmc_gauss_mfma_kernel<2, 4, true, true, false>
    "hmc_dense_d20_chain_mass": _hmc_d20_chain_mass,                    # hmc_gauss_mfma_kernel<2, 8, false, false, true, true>
    "hmc_logit_d70": _hmc_logit_d70,                                    # logit_lds_kernel<2, 1, 0, false>
    "hmc_logit_d70_bounds_diag_m": _hmc_logit_d70_bounds_diag_m,        # logit_lds_kernel<2, 1, 0, true, true>
    "hmc_dense_d130_dense_m": _hmc_d130_dense_m,                        # logit_lds_kernel<3, 1, 1, false, false, true>
    "hmc_dense_d520": lambda: _gemm("hmc", "plain"),                    # gemm_step_kernel<0, 0> (hmc, graph)
    "hmc_logit_d520": lambda: _gemm("hmc", "logit"),                    # gemm_step_kernel<0, 1> (hmc, graph)
    "hmc_dense_d520_dense_m": lambda: _gemm("hmc", "dense_m"),          # gemm_step_kernel<6, 0> (hmc, graph, dense precond_mat)
    "hmc_dense_d520_bounds": lambda: _gemm("hmc", "bounds"),            # gemm_step_kernel<10, 0> (hmc, graph, bounds)
    "hmc_dense_d150_bounds_dense_m_literal": _hmc_d150_bounds_dense_m,  # literal_kernel<0>
    "hmc_normal_model": lambda: _small_normal("hmc"),                   # hmc_small_kernel<NormalModel>
    "hmc_logit_d5_bounds": _hmc_logit_d5_bounds,                        # hmc_small_kernel<LogisticSmallModel<5>>
    "mala_dense_d40": lambda: _mala_dense(40, False),                   # mala_gauss_mfma_kernel<4, false>
    "mala_dense_d24_dense_m": lambda: _mala_dense(24, True),            # mala_gauss_dense_m_kernel<2>
    "mala_logit_d70": _mala_logit_d70,                                  # logit_lds_kernel<2, 0, 0, false>
    "mala_dense_d520": lambda: _gemm("mala", "plain"),                  # gemm_step_kernel<2, 0> (mala, graph)
    "mala_dense_d150_bounded_literal": _mala_d150_bounded,              # literal_kernel<1>
    "rwmh_dense_d37_bounds": _rwmh_d37_bounds,                          # rwmh_gauss_mfma_kernel<4, true, false>
    "rwmh_logit_d100": _rwmh_logit_d100,                                # logit_lds_kernel<2, 2, 0, false>
    "rwmh_dense_d520": lambda: _gemm("rwmh", "plain"),                  # gemm_step_kernel<2, 0> (rwmh, graph)
    "nuts_dense_d32_memo": lambda: _nuts_d32(mcmc_amd.KERNEL_AUTO),     # nuts_gauss_memo_kernel<2, false, true>
    "nuts_dense_d32_tick_local": lambda: _nuts_d32(mcmc_amd.KERNEL_NUTS_TICK_LOCAL),# nuts_gauss_async_kernel<2, false, false>
    "nuts_dense_d20_dense_m": lambda: _nuts_general(20, True),          # nuts_gauss_async_kernel<2, true, true>
    "nuts_gauss_d24_bounds": lambda: _nuts_general(24, False),          # nuts_tile_kernel<built-in Gaussian 2, true>
    "nuts_logit_d70": lambda: _nuts_lds("logistic", 70, 60),            # logit_lds_kernel<2, nuts, 0, false>
    "nuts_dense_d130": lambda: _nuts_lds("dense", 130, 0),              # logit_lds_kernel<3, nuts, 1, false>
    "nuts_dense_d520": lambda: _nuts_d520(False),                       # gemm_step_kernel<12, 0> (nuts, memoised, graph)
    "nuts_dense_d520_bounds": lambda: _nuts_d520(True),                 # gemm_step_kernel<13, 0> (nuts, memoised, graph, bounds)
    "nuts_dense_d150_dense_m_literal": _nuts_d150_dense_m_literal,      # literal_kernel<2> (by MI_KERNEL_LITERAL: AUTO runs logit_lds_kernel<., nuts, 1, false, false, true>)
    "nuts_normal_model": lambda: _small_normal("nuts"),                 # nuts_small_kernel<NormalModel>
    "rmhmc_normal_model": lambda: _small_normal("rmhmc"),               # rmhmc_small_kernel<NormalModel>
    "rmhmc_logit_d3": _rmhmc_logit_d3,                                  # rmhmc_small_kernel<LogisticSmallModel<3>>
    "rmhmc_dense_d6_literal": _rmhmc_dense_d6,                          # literal_kernel<4>
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    return case(name).oracle()


@functools.lru_cache(maxsize=None)
def host_of(name):
    return case(name).host()


@pytest.fixture(scope="module")
def stream():
    s = torch.cuda.Stream()                               # non-blocking: it does not order itself behind the NULL stream
    yield s
    mcmc_amd.release_workspace()                          # the cached workspaces of every stream, before the stream dies


@pytest.fixture(scope="module")
def stream2():
    s = torch.cuda.Stream()
    yield s
    mcmc_amd.release_workspace()


OUT = ("theta", "draws", "n_accept", "n_leap", "n_exec", "depth", "adapt_state")


def same_as_host(dv, h_draws, h, names=OUT, nan=False):
    """every output of the device-resident call against the host-staged one (eps: nuts alone writes it)"""
    for k in names:
        want = h_draws if k == "draws" else h.get(k)
        if want is None and dv[k] is None:
            continue
        assert dv[k] is not None and want is not None, k
        assert dv[k].dtype == want.dtype and np.array_equal(dv[k], want, equal_nan=nan and want.dtype == np.float64), k


def same_as_oracle(c, dv, o_draws, o, nan=False):
    assert np.array_equal(dv["n_accept"], o["n_accept"])
    assert np.array_equal(dv["draws"], o_draws, equal_nan=nan)
    if o_draws.shape[0]:
        assert np.array_equal(dv["theta"], o_draws[-1], equal_nan=nan)           # state out = last kept draw
    if "n_leap" in o and c.algo in ("hmc", "nuts", "rmhmc"):
        assert np.array_equal(dv["n_leap"], o["n_leap"])
    if c.algo == "nuts":
        assert np.array_equal(dv["eps"], o["eps"], equal_nan=nan)
        if "depth_first" in o:
            assert np.array_equal(dv["depth"][:, :o["depth_first"].shape[1]], o["depth_first"])


def outputs_contract(c, dv, st=None, deep_trees=True):
    """include/mi_mcmc.h, mi_chains: what every output holds after a call, whatever the caller's memory held before.  deep_trees: the call is a case's
    whole run, whose trees reach the depths at which a memoised doubling computes fewer points than it has leaves (2^j leaves, 1 + j (j + 1) / 2 points:
    from j = 3 on); the first draws of a run cut in two grow trees of one or two levels, where the two counts are equal"""
    burn, keep, L = (int(st.n_burnin_draws), int(st.n_keep_draws), int(st.n_leap_steps)) if st is not None else (*c.n_draws(), int(c.skw.get("n_leap_steps", 1)))
    assert dv["guards_ok"], "a store outside an output's extent"
    if c.algo in ("mala", "rwmh"):
        assert (dv["n_leap"] == 0).all()
    if c.algo == "hmc":
        assert (dv["n_leap"] == (burn + keep) * L).all()
    if c.memo:                                            # every distinct point of a doubling once: never more than the reference counts, and fewer over the call
        assert (dv["n_exec"] <= dv["n_leap"]).all()
        if deep_trees:                                    # memoisation happened, it is no replay that executes every leaf
            assert dv["n_exec"].sum() < dv["n_leap"].sum()
    else:
        assert np.array_equal(dv["n_exec"], dv["n_leap"])
    if c.algo == "nuts":
        assert dv["sentinel_left"] == set(), dv["sentinel_left"]
    else:
        assert "step_size" in dv["untouched"], "samplers other than nuts leave step_size unchanged"
        assert dv["sentinel_left"] == {"step_size"}, dv["sentinel_left"]


@pytest.mark.parametrize("name", list(CASES))
def test_device_resident_route(name, stream):
    c = case(name)
    dv = c.device(stream)
    print(f"{name}: {dv['kernel']}")
    assert c.kernel(dv["kernel"]), dv["kernel"]                                     # (a)
    o_draws, o = oracle_of(name)
    burn, keep = c.n_draws()
    acc, C = int(o["n_accept"].sum()), c.init.shape[0]
    print(f"{name}: the oracle accepts {acc} of {keep * C}")
    if c.mixed == "some":                                                           # (f)
        assert 0 < acc
    elif c.mixed == "both":
        assert 0 < acc < keep * C
    elif c.mixed == "leq":
        assert 0 < acc <= keep * C
    same_as_oracle(c, dv, o_draws, o)                                               # (b)
    h_draws, h = host_of(name)
    same_as_host(dv, h_draws, h)                                                    # (c)
    if c.algo == "nuts":
        assert np.array_equal(dv["eps"], h["eps"])
    outputs_contract(c, dv)                                                         # (d), (e)


# ---------------------------------------------------------------- a chain started non-finite: the flags, the replay workspace and the literal launch ride the stream
@pytest.mark.parametrize("name", ["hmc_dense_d20", "hmc_diag_d200", "hmc_logit_d70", "hmc_dense_d520", "nuts_dense_d32_memo"])
def test_a_chain_started_at_1e200_is_replayed_on_the_callers_stream(name, stream):
    c = case(name)
    init = c.init.copy()
    init[1] = 1e200
    dv = c.device(stream, init=init)
    assert c.kernel(dv["kernel"]), dv["kernel"]
    o_draws, o = c.oracle(init)
    same_as_oracle(c, dv, o_draws, o, nan=True)
    h_draws, h = c.host(init)
    same_as_host(dv, h_draws, h, nan=True)
    if c.algo == "nuts":
        assert np.array_equal(dv["eps"], h["eps"], equal_nan=True)
    outputs_contract(c, dv)


# ---------------------------------------------------------------- a run cut inside the adaptation window, both halves in device memory
@pytest.mark.parametrize("name", ["nuts_dense_d32_memo", "nuts_dense_d520"])
def test_a_nuts_run_cut_inside_the_window_in_device_memory(name, stream):
    c = case(name)
    burn, keep = c.n_draws()
    tot, cut = burn + keep, 2
    assert 0 < cut < int(c.skw["n_adapt_draws"]) < tot
    w_draws, w = c.host(st=c.settings(n_burnin_draws=0, n_keep_draws=tot))
    a = c.device(stream, st=c.settings(n_burnin_draws=0, n_keep_draws=cut))
    st_b = c.settings(n_burnin_draws=0, n_keep_draws=tot - cut)
    b = c.device(stream, init=np.ascontiguousarray(a["theta"].T), st=st_b, draw0=cut, step_size_in=a["eps"], adapt_state_in=a["adapt_state"])
    assert c.kernel(a["kernel"]) and c.kernel(b["kernel"])
    assert np.array_equal(np.concatenate([a["draws"], b["draws"]]), w_draws)
    assert np.array_equal(np.concatenate([a["depth"], b["depth"]]), w["depth"])
    assert np.array_equal(a["n_accept"] + b["n_accept"], w["n_accept"]) and np.array_equal(a["n_leap"] + b["n_leap"], w["n_leap"])
    for k in ("theta", "eps", "adapt_state"):
        assert np.array_equal(b[k], w[k]), k
    outputs_contract(c, a, st=c.settings(n_burnin_draws=0, n_keep_draws=cut), deep_trees=False)
    outputs_contract(c, b, st=st_b, deep_trees=False)


# ---------------------------------------------------------------- the optional outputs left out
@pytest.mark.parametrize("what", ["theta_and_draws", "theta_alone", "no_kept_draws"])
@pytest.mark.parametrize("name", ["hmc_dense_d20", "nuts_dense_d32_memo", "hmc_dense_d520", "mala_logit_d70"])
def test_device_resident_calls_without_the_optional_outputs(name, what, stream):
    c = case(name)
    if what == "no_kept_draws":                            # n_keep_draws = 0: the burn-in alone, against the host-staged call of the same settings
        st = c.settings(n_keep_draws=0)
        dv = c.device(stream, st=st)
        h_draws, h = c.host(st=st)
        assert dv["draws"].shape[0] == 0
        same_as_host(dv, h_draws, h)
        outputs_contract(c, dv, st=st, deep_trees=False)
        return
    dv = c.device(stream, outputs=("draws",) if what == "theta_and_draws" else ())
    h_draws, h = host_of(name)
    assert c.kernel(dv["kernel"]), dv["kernel"]
    assert np.array_equal(dv["theta"], h["theta"])
    if what == "theta_and_draws":
        assert np.array_equal(dv["draws"], h_draws)
    assert dv["guards_ok"] and dv["sentinel_left"] == set()


# ---------------------------------------------------------------- two callers' streams from one host thread: the per-(device, stream) workspace cache
def test_two_cases_queued_back_to_back_on_two_streams(stream, stream2):
    ca, cb = case("hmc_dense_d520"), case("nuts_dense_d32_memo")
    a, b = ca.device_call(), cb.device_call()
    torch.cuda.synchronize()
    a.enqueue(stream)
    b.enqueue(stream2)
    stream.synchronize()
    stream2.synchronize()
    for c, call, name in ((ca, a, "hmc_dense_d520"), (cb, b, "nuts_dense_d32_memo")):
        dv = call.collect()
        assert c.kernel(dv["kernel"]), dv["kernel"]
        h_draws, h = host_of(name)
        same_as_host(dv, h_draws, h)
        outputs_contract(c, dv)
