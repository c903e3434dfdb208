"""GPU: mi_mcmc_{hmc,mala}_run_mass_adapted_dense -- hmc / mala with a DENSE mass matrix pooled over the chains (NOT a reference mode).
What is checked: given the reported matrix the run is the oracle's mcmc::hmc bit for bit; the matrix is the header's five steps, transcribed
in numpy; the whole run is the chain of ordinary calls the header says it is, on every route a dense precond_mat has; a degenerate start runs
with M = I; and it does what it is for: a ROTATED ill-conditioned Gaussian, which defeats the identity and the diagonal mass alike, mixes.
Step 1 of the five takes S from mcmc_amd.draws_covariance itself; so that S has a reference of its own, the starting state's S is held bit for bit to
mcmc_amd/covariance.py, the numpy statement of the header's order, over the oracle's fma chain: the full matrix at d = 24 and d = 130, the corners and
random elements of each of the 15 tiles at d = 520 (tests/draws_cov_cases.py)."""
import numpy as np
import pytest

import draws_cov_cases as cov_cases
import mcmc_amd
import orc
from mcmc_amd import synth

pytestmark = pytest.mark.gpu

_ADAPT = {"hmc": mcmc_amd.hmc_mass_adapted_dense, "mala": mcmc_amd.mala_mass_adapted_dense}


def _settings(seed, burn, keep, L, eps, **kw):
    return mcmc_amd.default_settings(rng_seed_value=seed, n_burnin_draws=burn, n_keep_draws=keep, n_leap_steps=L, step_size=eps, **kw)


def _adapted(algo, kind, prec, init, n_windows, burn, keep, L, eps, seed=5):
    C, d = init.shape
    t = mcmc_amd.make_target(kind, d, prec=prec)
    theta = np.ascontiguousarray(init.T.copy())
    draws = np.zeros((keep, d, C))
    nacc = np.zeros(C, dtype=np.uint64)
    M = _ADAPT[algo](t, _settings(seed, burn, keep, L, eps), mcmc_amd.make_chains(theta, C, draws=draws, n_accept=nacc), n_windows=n_windows)
    return draws, nacc, M, theta


def _five_steps(theta, mirror_S=False):
    """include/mi_mcmc.h, mi_mcmc_hmc_run_mass_adapted_dense: THE ESTIMATE, from the chains' state [d][C]; mirror_S: S is first held to the mirror"""
    d, C = theta.shape
    _, S = mcmc_amd.draws_covariance(theta, want_mean=False)                             # 1.
    if mirror_S:
        ref = cov_cases.mirror(theta)
        assert (ref["cov"] is None) == (d > 400) and (d <= 400 or len(ref["elements"]) >= 5 * len(cov_cases.tiles(d)))
        cov_cases.assert_is_the_mirror(None, S, ref, ("S of the state", d, C))
        assert np.array_equal(cov_cases.bits(S), cov_cases.bits(S.T))
    ok = bool(np.isfinite(S).all() and (np.diag(S) > 0.0).all())
    M = None
    if ok:
        a, b = C / (C + 5.0), 1e-3 * (5.0 / (C + 5.0))                                   # 2.
        Sp = a * S                                                                       # 3.
        Sp[np.diag_indices(d)] = a * np.diag(S) + b
        M0 = mcmc_amd.mat_inverse(Sp)                                                    # 4.
        M = 0.5 * (M0 + M0.T)                                                            # 5.
        ok = bool(np.isfinite(M).all() and np.isfinite(mcmc_amd.mat_cholesky_lower(M)).all())
    return M if ok else np.eye(d)


def _by_hand(algo, kind, prec, init, n_windows, burn, keep, L, eps, seed=5, mirror_S=False):
    """the same run from draws_covariance -> the five steps -> an ordinary call with that precond_mat, part by part through draw0
    (mirror_S: the S of the STARTING state is held to the mirror of the header's order on the way)"""
    state = np.ascontiguousarray(init.T.copy())                                          # [d][C]
    n_parts, done, Ms = n_windows + 1, 0, []
    draws = nacc = None
    M = _five_steps(state, mirror_S)
    for part in range(n_parts):
        last = part + 1 == n_parts
        upto = burn if last else (burn * (part + 1)) // n_parts
        Ms.append(M)
        if (upto - done) + (keep if last else 0) > 0:
            st = _settings(seed, upto - done, keep if last else 0, L, eps, precond_mat=M)
            dr, info = mcmc_amd.sample(algo, kind, state.T, st, prec=prec, draw0=done)
            state = info["theta"]
            if last:
                draws, nacc = dr, info["n_accept"]
        done = upto
        if not last:
            M = _five_steps(state)
    return draws, nacc, M, state, Ms


def test_given_the_matrix_the_run_is_the_oracles_hmc_and_the_matrix_is_the_five_steps():
    d, C, burn, keep, L, eps = 24, 200, 9, 12, 6, 0.25
    prec = synth.dense_gaussian_precision(d)
    init = synth.initial_states(C, d, seed=2)
    draws, nacc, M, _ = _adapted("hmc", mcmc_amd.TARGET_GAUSS_DENSE, prec, init, 0, burn, keep, L, eps)
    assert np.array_equal(M, _five_steps(np.ascontiguousarray(init.T), mirror_S=True)) and np.array_equal(M, M.T) and not np.array_equal(M, np.eye(d))
    t = orc.TargetSpec(orc.TARGET_DENSE, d, prec=prec, W=4)
    s = orc.make_settings(seed=5, n_burnin=burn, n_keep=keep, n_leap=L, step=eps, W=4, precond=M)
    o, info = orc.run_many(orc.ALGO_HMC, t, init, s)
    assert info["n_accept"].sum() > 0
    assert np.array_equal(nacc, info["n_accept"]) and np.array_equal(draws, o)


@pytest.mark.parametrize("algo,d,C,burn,keep,L,want", [("hmc", 24, 200, 30, 6, 6, None), ("mala", 40, 300, 30, 6, 1, None),
                                                        ("hmc", 130, 3000, 4, 2, 3, "lds"), ("hmc", 520, 2000, 4, 2, 3, "gemm")],
                         ids=["hmc_d24", "mala_d40", "hmc_d130_lds", "hmc_d520_gemm"])
def test_the_run_is_a_chain_of_ordinary_calls(algo, d, C, burn, keep, L, want):
    n_windows = 2 if want is None else 1
    eps = 0.25 if algo == "hmc" else 0.4
    prec = synth.dense_gaussian_precision(d)
    init = synth.initial_states(C, d, seed=4)
    kind = mcmc_amd.TARGET_GAUSS_DENSE
    h_draws, h_nacc, h_M, h_theta, Ms = _by_hand(algo, kind, prec, init, n_windows, burn, keep, L, eps, mirror_S=want is not None)
    draws, nacc, M, theta = _adapted(algo, kind, prec, init, n_windows, burn, keep, L, eps)
    name = mcmc_amd.last_kernel()
    if want == "lds":
        assert name.startswith("logit_lds_kernel<"), name
    if want == "gemm":
        assert name.startswith("gemm_step_kernel<") and "dense precond_mat" in name, name
    assert np.array_equal(M, h_M) and np.array_equal(draws, h_draws) and np.array_equal(nacc, h_nacc) and np.array_equal(theta, h_theta)
    assert all(not np.array_equal(Ms[k], Ms[k + 1]) for k in range(n_windows))           # every part ran with its own estimate
    assert np.isfinite(draws).all() and nacc.sum() > 0
    if want is None:                                                                     # reproducible
        again = _adapted(algo, kind, prec, init, n_windows, burn, keep, L, eps)
        assert all(np.array_equal(x, y) for x, y in zip((draws, nacc, M, theta), again))


def test_a_degenerate_start_runs_with_the_identity():
    """All chains at one point whose sums are exact in fp64: the pooled covariance is exactly 0, its diagonal is not positive, the part runs
    with M = I -- the bits of a plain call.  The chains spread during it, and the later parts adapt."""
    d, C, L, eps = 24, 200, 6, 0.2
    prec = synth.dense_gaussian_precision(d)
    init = np.tile((np.arange(d) % 7 - 3) / 8.0, (C, 1))
    draws, nacc, M, _ = _adapted("hmc", mcmc_amd.TARGET_GAUSS_DENSE, prec, init, 0, 10, 5, L, eps)
    assert np.array_equal(M, np.eye(d))
    plain, info = mcmc_amd.hmc(mcmc_amd.TARGET_GAUSS_DENSE, init, _settings(5, 10, 5, L, eps), prec=prec)
    assert np.array_equal(draws, plain) and np.array_equal(nacc, info["n_accept"]) and nacc.sum() > 0
    _, _, M2, _ = _adapted("hmc", mcmc_amd.TARGET_GAUSS_DENSE, prec, init, 2, 30, 5, L, eps)
    assert np.isfinite(M2).all() and not np.array_equal(M2, np.eye(d))
    assert np.array_equal(M2, _by_hand("hmc", mcmc_amd.TARGET_GAUSS_DENSE, prec, init, 2, 30, 5, L, eps)[2])


def test_the_dense_mass_makes_a_rotated_ill_conditioned_gaussian_mix():
    """P = Q diag(1 .. 400) Q^T at eps = 0.3: eps sqrt(lambda_max) = 6 is past the leapfrog's stability limit of 2, so the identity mass
    accepts nothing, and the rotation hides the scales from a diagonal mass.  (A numpy model of the procedure gave 0.96 / 0.00 / 0.00.)"""
    d, C, burn, keep, L, eps = 24, 400, 30, 10, 6, 0.3
    rng = np.random.default_rng(11)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = np.logspace(0.0, np.log10(400.0), d)
    P = (Q * lam[None, :]) @ Q.T
    P = 0.5 * (P + P.T)
    init = 1.5 * (rng.standard_normal((C, d)) / np.sqrt(lam)[None, :]) @ Q.T               # 1.5 N(0, P^-1)
    kind = mcmc_amd.TARGET_GAUSS_DENSE
    _, nacc_dense, M, _ = _adapted("hmc", kind, P, init, 3, burn, keep, L, eps)
    t = mcmc_amd.make_target(kind, d, prec=P)
    nacc_diag = np.zeros(C, dtype=np.uint64)
    mcmc_amd.hmc_mass_adapted(t, _settings(5, burn, keep, L, eps),
                              mcmc_amd.make_chains(np.ascontiguousarray(init.T.copy()), C, draws=np.zeros((keep, d, C)), n_accept=nacc_diag), n_windows=3)
    _, plain = mcmc_amd.hmc(kind, init, _settings(5, burn, keep, L, eps), prec=P)
    r_dense, r_diag, r_plain = nacc_dense.mean() / keep, nacc_diag.mean() / keep, plain["n_accept"].mean() / keep
    print(f"mean acceptance of the kept draws: dense pooled mass {r_dense:.3f}, diagonal pooled mass {r_diag:.3f}, identity {r_plain:.3f}")
    assert r_dense > 0.5
    assert r_diag < 0.05
    assert r_plain < 0.05
