"""GPU: settings.vals_bound beyond d = 512 for hmc (identity / diagonal precond_mat) and rwmh (no cov_mat) on the matrix-product route (ref: src/hmc.cpp:84-95,
107-122,134-136,211-218, src/rwmh.cpp:105-107,113,128).  The chains live in the transformed space, the products are taken at x = inv_transform(theta), the half-kicks
take J(theta) g in the product's epilogue and the energies add log_jacobian(theta) (mcmc_amd/csrc/gemm_samplers.hip: gemm_step_kernel<10 / 11, .>); before, such a
call ran on the literal kernel.  Bit for bit against the oracle, against the literal kernel of the same library on more chains, across a continuation and in the
non-finite regime; and the law itself on 4096 chains."""
import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import synth

pytestmark = pytest.mark.gpu
ALGO = {"hmc": orc.ALGO_HMC, "mala": orc.ALGO_MALA, "rwmh": orc.ALGO_RWMH, "nuts": orc.ALGO_NUTS}
# accepts AND rejects on every case below (the oracle's counts, checked on the CPU beforehand, are asserted per case).  hmc at 0.1 rejects everything on the bounded
# patterns; with every bound infinite (pattern c: the unbounded dynamics) hmc at 0.02 accepts every draw at d = 1024, L = 4, and at 0.12 it accepts 220 of 270
STEP = 0.02
STEP_HMC_UNBOUNDED = 0.12
LB, UB = -1.5, 2.0


def bounds(d, pattern, seed=None):
    """(a) about a quarter of the dimensions bounded, types 2 / 3 / 4 mixed; (b) every dimension type 4; (c) vals_bound with all bounds infinite"""
    lo, hi = np.full(d, -np.inf), np.full(d, np.inf)
    if pattern == "a":
        t = np.random.default_rng(d if seed is None else seed).choice([1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 4], size=d)
        lo[(t == 2) | (t == 4)] = LB
        hi[(t == 3) | (t == 4)] = UB
    elif pattern == "b":
        lo[:], hi[:] = LB, UB
    return lo, hi


def diag_mass(d, seed):
    return np.diag(np.random.default_rng(seed).uniform(0.5, 2.0, d))


def _problem(target, d, N, C, seed_t=5):
    """target keywords for mcmc_amd.sample, the oracle's TargetSpec, initial states inside [-1, 1.5] (inside the bounds of every pattern)"""
    if target == "dense":
        prec = synth.dense_gaussian_precision(d, seed=d % 89)
        init = np.clip(synth.initial_states(C, d, seed=d + 2) * 0.5, -1.0, 1.5)
        return mcmc_amd.TARGET_GAUSS_DENSE, dict(prec=prec), orc.TargetSpec(orc.TARGET_DENSE, d, prec=prec, W=4), init
    X, y = synth.logistic_problem(d, N, seed=seed_t)
    init = np.clip(synth.initial_states(C, d, seed=d + 2) * 0.1, -1.0, 1.5)
    return mcmc_amd.TARGET_LOGISTIC, dict(X=X, y=y), orc.TargetSpec(orc.TARGET_LOGISTIC, d, X=X, y=y, W=4), init


def _oracle(algo, spec, init, lo, hi, M, L, eps, burn, keep, seed, chain0=0):
    s = orc.make_settings(seed=seed, n_burnin=burn, n_keep=keep, n_leap=L, step=eps, W=4, hoist=1, precond=M, lower=lo, upper=hi)
    return orc.run_many(ALGO[algo], spec, init, s, chain0=chain0)


def _run_both(algo, target, d, N, C, L, pattern, diag, eps, burn, keep, seed, init_edit=None, chain0=0):
    kind, tkw, spec, init = _problem(target, d, N, C)
    if init_edit is not None:
        init_edit(init)
    lo, hi = bounds(d, pattern)
    M = diag_mass(d, d + 1) if diag else None
    st = mcmc_amd.default_settings(rng_seed_value=seed, n_burnin_draws=burn, n_keep_draws=keep, n_leap_steps=L, step_size=eps, precond_mat=M,
                                   vals_bound=1, lower_bounds=lo, upper_bounds=hi)
    g_draws, g = mcmc_amd.sample(algo, kind, init, st, chain0=chain0, **tkw)
    kern = mcmc_amd.last_kernel()
    o_draws, o = _oracle(algo, spec, init, lo, hi, M, L, eps, burn, keep, seed, chain0)
    return kern, g_draws, g, o_draws, o, lo, hi


def _strictly_inside(draws, lo, hi):
    """draws [n_keep][d][C] against the finite bounds"""
    return bool(np.all(draws > lo[None, :, None]) and np.all(draws < hi[None, :, None]))


CASES = [  # target, d, N, C, L, bound pattern, diagonal precond_mat (hmc)?, chain0
    ("dense", 513, 0, 45, 3, "a", False, 0), ("dense", 640, 0, 130, 1, "b", True, 11), ("dense", 640, 0, 45, 3, "b", True, 0), ("dense", 1024, 0, 45, 4, "c", False, 11),
    ("dense", 1100, 0, 45, 3, "a", False, 0),
    ("logit", 513, 40, 130, 1, "a", True, 11), ("logit", 600, 70, 45, 3, "a", False, 0), ("logit", 700, 300, 45, 3, "b", False, 5),
]


@pytest.mark.parametrize("algo", ["hmc", "rwmh"])
@pytest.mark.parametrize("target,d,N,C,L,pattern,diag,chain0", CASES)
def test_bounds_beyond_d512_equal_the_oracle(algo, target, d, N, C, L, pattern, diag, chain0):
    """ragged d and N, ragged chain tiles (C = 45; C = 130: two tiles of 128), one and several leapfrog steps, the three bound patterns; the route is the
    matrix-product one (on the commit before this it was literal_kernel<...>)"""
    diag = diag and algo == "hmc"          # (rwmh's precond_mat is a cov_mat: the literal kernel)
    eps = STEP_HMC_UNBOUNDED if (algo == "hmc" and pattern == "c") else STEP
    kern, g_draws, g, o_draws, o, lo, hi = _run_both(algo, target, d, N, C, L, pattern, diag, eps, 2, 6, 7, chain0=chain0)
    assert kern.startswith("gemm_step_kernel<") and "bounds" in kern, kern
    assert (", 1>" in kern) == (target == "logit"), kern
    assert ("diagonal precond_mat" in kern) == diag, kern
    print(f"{algo} {target} d={d} C={C} L={L} pattern {pattern} diag={diag}: oracle accepts {int(o['n_accept'].sum())} of {6 * C}")
    assert np.all(np.isfinite(o_draws))
    assert 0 < o["n_accept"].sum() < 6 * C
    assert np.array_equal(g["n_accept"], o["n_accept"])
    assert np.array_equal(g_draws, o_draws)
    assert np.array_equal(g["theta"], o_draws[-1])
    assert _strictly_inside(g_draws, lo, hi)
    if algo == "hmc":
        assert np.array_equal(g["n_leap"], o["n_leap"])


@pytest.mark.parametrize("algo", ["hmc", "rwmh"])
@pytest.mark.parametrize("target", ["dense", "logit"])
def test_bounds_equal_the_literal_kernel_on_more_chains(algo, target):
    """three chain tiles (one ragged) x six row tiles, 4 + 8 draws: the same call on the literal kernel (one workgroup per chain)"""
    d, N, C = 700, 200, 300
    kind, tkw, _, init = _problem(target, d, N, C, seed_t=9)
    lo, hi = bounds(d, "a")
    st = mcmc_amd.default_settings(rng_seed_value=21, n_burnin_draws=4, n_keep_draws=8, n_leap_steps=4, step_size=STEP, vals_bound=1, lower_bounds=lo, upper_bounds=hi)
    g_draws, g = mcmc_amd.sample(algo, kind, init, st, chain0=1000, **tkw)
    kern = mcmc_amd.last_kernel()
    assert kern.startswith("gemm_step_kernel<") and "bounds" in kern, kern
    l_draws, l = mcmc_amd.sample(algo, kind, init, st, chain0=1000, kernel_hint=mcmc_amd.KERNEL_LITERAL, **tkw)
    assert mcmc_amd.last_kernel().startswith("literal_kernel<")
    print(f"{algo} {target}: literal kernel accepts {int(l['n_accept'].sum())} of {8 * C}")
    assert 0 < l["n_accept"].sum() <= 8 * C
    assert np.array_equal(g["n_accept"], l["n_accept"]) and np.array_equal(g_draws, l_draws) and np.array_equal(g["theta"], l["theta"])
    assert np.array_equal(g["n_leap"], l["n_leap"])
    assert _strictly_inside(g_draws, lo, hi)


def _poison(init):
    """huge / +inf / NaN starts in single chains, on bounded and on unbounded dimensions of pattern (a) at d = 640"""
    d = init.shape[1]
    lo, hi = bounds(d, "a")
    bounded = np.flatnonzero(np.isfinite(lo) | np.isfinite(hi))
    free = np.flatnonzero(~(np.isfinite(lo) | np.isfinite(hi)))
    init[3] *= 1e200
    init[7, bounded[2]] = np.inf
    init[12, free[2]] = np.inf
    init[20, bounded[-1]] = np.nan
    init[26, free[-1]] = np.nan
    init[33] *= 1e160


POISONED = (3, 7, 12, 20, 26, 33)


@pytest.mark.parametrize("algo", ["hmc", "rwmh"])
@pytest.mark.parametrize("target", ["dense", "logit"])
def test_bounds_in_the_non_finite_regime(algo, target):
    """step sizes that blow chains up and initial values that are huge / +inf / NaN already (hmc: flagged by the accept step and replayed literally with the
    bounds); the healthy chains in the neighbouring columns of every product keep the oracle's bits and stay finite at the small step size"""
    d, N, C = 640, 64, 45
    for eps in (STEP, 1e6):
        kern, g_draws, g, o_draws, o, lo, hi = _run_both(algo, target, d, N, C, 3, "a", False, eps, 2, 3, 5, init_edit=_poison)
        assert kern.startswith("gemm_step_kernel<") and "bounds" in kern, kern
        print(f"{algo} {target} eps={eps}: oracle accepts {int(o['n_accept'].sum())} of {3 * C}")
        assert np.array_equal(g["n_accept"], o["n_accept"]), eps
        assert np.array_equal(g_draws, o_draws, equal_nan=True), eps
        assert np.array_equal(g["theta"], o_draws[-1], equal_nan=True), eps
        if eps < 1.0:
            healthy = [c for c in range(C) if c not in POISONED]
            assert np.all(np.isfinite(g_draws[:, :, healthy]))


def _cut_run(algo, pattern, hint):
    """6 draws in one call, and as 2 + 4 through mi_chains.draw0 with the final state of the first call as the initial values of the second"""
    d, C = 520, 33
    kind, tkw, _, init = _problem("dense", d, 0, C)
    lo, hi = bounds(d, pattern)
    S = lambda keep: mcmc_amd.default_settings(rng_seed_value=8, n_burnin_draws=0, n_keep_draws=keep, n_leap_steps=3, step_size=STEP, vals_bound=1, lower_bounds=lo, upper_bounds=hi)
    whole, w = mcmc_amd.sample(algo, kind, init, S(6), kernel_hint=hint, **tkw)
    kern = mcmc_amd.last_kernel()
    a, ga = mcmc_amd.sample(algo, kind, init, S(2), kernel_hint=hint, **tkw)
    b, gb = mcmc_amd.sample(algo, kind, np.ascontiguousarray(ga["theta"].T), S(4), draw0=2, kernel_hint=hint, **tkw)
    return kern, whole, w, a, ga, b, gb


@pytest.mark.parametrize("algo", ["hmc", "rwmh"])
def test_bounds_continue_a_run(algo):
    """a run cut into two calls (mi_chains.draw0) equals the run in one piece.  Bit for bit this can hold only where the hand-over is exact: the final state leaves
    through inv_transform (hmc.cpp:211-218) and a continued call -- like any call of the reference -- puts its initial values through transform (:134-136), and
    transform(inv_transform(theta)) is theta only up to rounding on a bounded dimension.  So the equality with the run in one piece is asserted with vals_bound
    set and every bound infinite (pattern c: type 1, both maps the identity), where the whole bounded route runs and nothing is rounded; with finite bounds
    (pattern a) the cut run is asserted equal to the literal kernel's cut run, call by call -- what mi_mcmc.h promises for theta -- and its first piece to the
    head of the run in one piece.  (Measured on pattern a, hmc: the literal kernel's run in one piece and its cut run differ from the third draw on as well.)"""
    kern, whole, w, a, ga, b, gb = _cut_run(algo, "c", mcmc_amd.KERNEL_AUTO)
    assert kern.startswith("gemm_step_kernel<") and "bounds" in kern, kern
    assert 0 < w["n_accept"].sum()
    assert np.array_equal(whole, np.concatenate([a, b]))
    assert np.array_equal(w["n_accept"], ga["n_accept"] + gb["n_accept"])
    assert np.array_equal(w["theta"], gb["theta"])
    kern, whole, w, a, ga, b, gb = _cut_run(algo, "a", mcmc_amd.KERNEL_AUTO)
    assert kern.startswith("gemm_step_kernel<") and "bounds" in kern, kern
    lkern, lwhole, lw, la, lga, lb_, lgb = _cut_run(algo, "a", mcmc_amd.KERNEL_LITERAL)
    assert lkern.startswith("literal_kernel<"), lkern
    assert 0 < w["n_accept"].sum() < 6 * 33
    assert np.array_equal(whole, lwhole) and np.array_equal(w["theta"], lw["theta"]) and np.array_equal(w["n_accept"], lw["n_accept"])
    assert np.array_equal(a, la) and np.array_equal(ga["theta"], lga["theta"]) and np.array_equal(ga["n_accept"], lga["n_accept"])
    assert np.array_equal(b, lb_) and np.array_equal(gb["theta"], lgb["theta"]) and np.array_equal(gb["n_accept"], lgb["n_accept"])
    assert np.array_equal(a, whole[:2])


LAW_STEP = 7e-5


def test_bounded_hmc_recovers_the_covariance():
    """the law, at d = 576 on 4096 chains, every dimension bounded to [-50, 50] -- far outside the mass, so the target is the plain Gaussian to rounding:
    per-dimension variances of one kept draw against diag(P^-1) within 0.15 (the bound and chain count of test_dense_precond_mat_hmc_recovers_the_covariance:
    the sd of a variance ratio at 4096 chains is sqrt(2 / 4096) = 0.022) and mean acceptance above 0.5.
    The step size.  dx / dtheta is about 25 at the centre of [-50, 50], so the search started at the unbounded 0.12 / 25 = 0.0048.  The CPU oracle on the first
    48 chains of this very call (L = 8, 31 draws) accepts 0 of its draws there and at 0.0024 / 0.0012, 0.04 at 0.0006, 0.30 at 0.0003, 0.59 at 0.00015 and 0.78 at
    0.00007, which is the value taken.  Why so small: the reference kicks the momentum with INV(dx / dtheta) g (inv_jacobian_adjust, hmc.cpp:114-122) where the
    gradient of the transformed density is (dx / dtheta) g + d log_jacobian / dtheta, so its trajectories do not conserve the energy its accept step computes
    (box_log_kernel, the right density); kick and drift are still shears, so the chain keeps the right law at the price of a small step.  The chains start
    from the target, so the variances must come out whatever the mixing."""
    d, C = 576, 4096
    prec = synth.dense_gaussian_precision(d, seed=5)
    cov = np.linalg.inv(prec)
    rng = np.random.default_rng(1)
    init = rng.multivariate_normal(np.zeros(d), cov, size=C)
    st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=30, n_keep_draws=1, n_leap_steps=8, step_size=LAW_STEP,
                                   vals_bound=1, lower_bounds=np.full(d, -50.0), upper_bounds=np.full(d, 50.0))
    g_draws, g = mcmc_amd.hmc(mcmc_amd.TARGET_GAUSS_DENSE, init, st, prec=prec)
    kern = mcmc_amd.last_kernel()
    assert kern.startswith("gemm_step_kernel<") and "bounds" in kern, kern
    v = g_draws[0].var(axis=1)
    print(f"variance ratio {float((v / np.diag(cov)).min()):.3f} .. {float((v / np.diag(cov)).max()):.3f}, accept rate {float(g['n_accept'].mean()):.3f}")
    assert np.all(np.abs(v / np.diag(cov) - 1.0) < 0.15)
    assert g["n_accept"].mean() > 0.5


def test_what_stays_on_the_literal_kernel_with_bounds():
    """bounded nuts, bounds + chains.mass_diag, bounded rwmh with a cov_mat beyond d = 512 run on the literal kernel as before.  Bounded mala beyond d = 512 runs nowhere,
    as before: the literal kernel refuses it (ten d x d matrices per workgroup: its proposal covariance is J M per chain) with MI_ERR_UNSUPPORTED, and the
    matrix-product route must not pick it up"""
    d, C = 520, 6
    prec = synth.dense_gaussian_precision(d, seed=3)
    init = np.clip(synth.initial_states(C, d, seed=2) * 0.5, -1.0, 1.5)
    lo, hi = bounds(d, "a")
    B = dict(vals_bound=1, lower_bounds=lo, upper_bounds=hi)
    st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=2, step_size=0.01, **B)
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.sample("mala", mcmc_amd.TARGET_GAUSS_DENSE, init, st, prec=prec)
    assert e.value.code == 3 and "mala: vals_bound with d > 512 is not implemented" in str(e.value), str(e.value)
    st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=2, n_adapt_draws=1, max_tree_depth=2, step_size=0.01, **B)
    mcmc_amd.sample("nuts", mcmc_amd.TARGET_GAUSS_DENSE, init, st, prec=prec)
    assert mcmc_amd.last_kernel().startswith("literal_kernel<"), mcmc_amd.last_kernel()
    st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=2, n_leap_steps=2, step_size=0.01, **B)
    theta = np.array(init.T, order="C", copy=True)
    mass = np.ascontiguousarray(np.random.default_rng(4).uniform(0.5, 2.0, (d, C)))
    mcmc_amd.run("hmc", mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=prec), st, mcmc_amd.make_chains(theta, C, mass_diag=mass))
    assert mcmc_amd.last_kernel().startswith("literal_kernel<"), mcmc_amd.last_kernel()
    st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=2, step_size=0.01, precond_mat=diag_mass(d, 1), **B)
    mcmc_amd.sample("rwmh", mcmc_amd.TARGET_GAUSS_DENSE, init, st, prec=prec)
    assert mcmc_amd.last_kernel().startswith("literal_kernel<"), mcmc_amd.last_kernel()


def test_vals_bound_without_the_bound_arrays_is_a_bad_argument():
    d, C = 520, 4
    prec = synth.dense_gaussian_precision(d, seed=3)
    init = synth.initial_states(C, d, seed=2) * 0.5
    st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=2, n_leap_steps=2, step_size=0.01, vals_bound=1)
    for algo in ("hmc", "rwmh"):
        with pytest.raises(mcmc_amd.MiMcmcError) as e:
            mcmc_amd.sample(algo, mcmc_amd.TARGET_GAUSS_DENSE, init, st, prec=prec)
        assert "vals_bound needs lower_bounds and upper_bounds" in str(e.value), str(e.value)


def test_fuzz_slice():
    """a short slice of tests/fuzz_gemm_bounds.py (the long sweep: test_fuzz_long, gpu_slow)"""
    import fuzz_gemm_bounds
    assert fuzz_gemm_bounds.sweep(n_cases=6, seed=3, verbose=True) == 0


@pytest.mark.gpu_slow
def test_fuzz_long():
    import fuzz_gemm_bounds
    assert fuzz_gemm_bounds.sweep(n_cases=40, seed=1, verbose=True) == 0
