"""No GPU: mi_mcmc_draws_psis_loo rejects bad arguments before any device call; the tail length and the plan of a call (draws_psis.hpp: row groups, tail
route, body pieces) are the stated functions of the shape and of the budgets; and mcmc_amd/psis.py, the numpy statement of include/mi_mcmc.h's
definition, gives the known answers on exactly Pareto ratios, the stated degenerate and non-finite results, bits that do not depend on the order of the
columns, and agrees with an evaluation of the same formulas in 60-digit arithmetic.

ACCURACY of the mirror over the CPU oracle's exp / log (the library's arithmetic) on the same ll values, against (a) mpmath at 60 digits with true
log1p / expm1 and exact sums, and (b) a plain libm-numpy transcription (np.sum, np.log, np.exp).  Measured worst cases over the recorded inputs
(K = 25, 200, 4100; LOGISTIC and NORMAL_MODEL rows, every fit finite):
    against (a): elpd_loo_r 8.4e-15 relative, khat_r 4.0e-14 absolute  (both at NORMAL_MODEL, K = 4100)
    against (b): elpd_loo_r 8.9e-16 relative, khat_r 6.3e-15 absolute
The bounds asserted are those figures times 10, rounded up to a power of ten: (a) 1e-13 and 1e-12, (b) 1e-14 and 1e-13.  (b) shares log(1 - t) and
exp(t) - 1 with the mirror, (a) does not: the distance between the two lines is what the missing log1p / expm1 cost, a few 1e-14 -- eleven orders
below the Monte Carlo error of either quantity, so det_math.hpp gets no log1p / expm1 for this."""
import ctypes as C
import math

import mpmath
import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import psis, synth, waic

_X = np.zeros((5, 3, 5))
_ROWS = np.zeros((5, 3))
_Y = np.zeros(5)
_ELPD, _PK, _LPPD, _SUMM = np.zeros(5), np.zeros(5), np.zeros(5), np.zeros(5)

ORC_MATH = dict(dot=lambda a, b: orc.dot(a, b, 1), exp=lambda x: orc.math_eval(0, x)[0], log=lambda x: orc.math_eval(1, x)[0],
                softplus=lambda x: orc.math_eval(3, x)[0])
L, N = mcmc_amd.TARGET_LOGISTIC, mcmc_amd.TARGET_NORMAL_MODEL


def _target(kind=L, d=3, prec=None, X=_ROWS, y=_Y, n_rows=None, struct_size=None):
    t = mcmc_amd.make_target(kind, d, prec=prec, X=X, y=y)
    if n_rows is not None:
        t.n_rows = n_rows
    if struct_size is not None:
        t.struct_size = struct_size
    return t


def _rc(target, slab=_X.ctypes.data, n_keep=5, n_chains=5, outs=(True, True, True, True)):
    ptrs = [a.ctypes.data if on else None for a, on in zip((_ELPD, _PK, _LPPD, _SUMM), outs)]
    return mcmc_amd.lib().mi_mcmc_draws_psis_loo(None if target is None else C.byref(target), slab, mcmc_amd.MEM_HOST,
                                                n_keep, n_chains, *[p for p in ptrs], None)


_NORMAL = dict(kind=N, d=2, X=None)
_BAD = {
    "null_target": (None, {}, "target"),
    "null_slab": ({}, dict(slab=None), "slab"),
    "all_outputs_null": ({}, dict(outs=(False, False, False, False)), "all NULL"),
    "struct_size": (dict(struct_size=3), {}, "struct_size"),
    "d_is_0": (dict(d=0), {}, "d "),
    "n_keep_is_0": ({}, dict(n_keep=0), "K "),
    "n_chains_is_0": ({}, dict(n_chains=0), "K "),
    "K_is_1": ({}, dict(n_keep=1, n_chains=1), "K = n_keep * n_chains = 1"),
    "K_is_24": ({}, dict(n_keep=4, n_chains=6), "K = n_keep * n_chains = 24, at least 25"),
    "K_is_2_to_32": ({}, dict(n_keep=1 << 16, n_chains=1 << 16), "below 2^32"),
    "n_keep_past_32_bits": ({}, dict(n_keep=1 << 32), "n_keep"),
    "n_chains_past_32_bits": ({}, dict(n_chains=1 << 32), "n_chains"),
    "d_past_65536": (dict(d=65537), {}, "d = 65537"),
    "logistic_without_X": (dict(X=None, n_rows=5), {}, "logistic"),
    "logistic_without_y": (dict(y=None), {}, "logistic"),
    "logistic_n_rows_is_0": (dict(n_rows=0), {}, "n_rows"),
    "normal_model_without_y": (dict(_NORMAL, y=None, n_rows=5), {}, "NORMAL_MODEL"),
    "normal_model_n_rows_is_0": (dict(_NORMAL, n_rows=0), {}, "n_rows"),
    "normal_model_d_is_3": (dict(_NORMAL, d=3), {}, "d = 2"),
    "kind_is_0": (dict(kind=0), {}, "kind"),
    "kind_is_7": (dict(kind=7), {}, "kind"),
}


@pytest.mark.parametrize("case", sorted(_BAD))
def test_psis_loo_rejects_bad_arguments_without_a_gpu(case):
    tkw, kw, names = _BAD[case]
    target = None if tkw is None else _target(**tkw)
    assert _rc(target, **kw) == mcmc_amd.MI_ERR_BAD_ARG
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_psis_loo:") and names in msg, msg


@pytest.mark.parametrize("kind,prec", [(mcmc_amd.TARGET_GAUSS_ISO, None), (mcmc_amd.TARGET_GAUSS_DIAG, np.ones(3)), (mcmc_amd.TARGET_GAUSS_DENSE, np.eye(3)),
                                       (mcmc_amd.TARGET_GAUSS_MIXTURE, np.ones(5))], ids=["iso", "diag", "dense", "mixture"])
def test_targets_without_observations_are_unsupported_without_a_gpu(kind, prec):
    assert _rc(_target(kind=kind, prec=prec)) == mcmc_amd.MI_ERR_UNSUPPORTED
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_psis_loo:") and "no observations" in msg, msg


def test_K_of_25_and_each_single_output_pass_the_argument_checks():
    assert "mi_mcmc_draws_psis_loo" in mcmc_amd.EXPORTS and hasattr(mcmc_amd.lib(), "mi_mcmc_draws_psis_loo")
    for name in ("mi_mcmc_test_psis_plan", "mi_mcmc_test_set_psis_ll_bytes", "mi_mcmc_test_set_psis_lds_tail"):
        assert hasattr(mcmc_amd.lib(), name)
    with pytest.raises(ValueError):
        mcmc_amd.draws_psis_loo(_target(), np.zeros((5, 4, 5)))           # the slab's d is not the target's
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_psis_loo(_target(), np.zeros((4, 3, 6)))           # K = 24
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    if mcmc_amd.lib().mi_mcmc_device_count() == 0:
        assert _rc(_target()) == mcmc_amd.MI_ERR_NO_DEVICE                # K = 25: accepted as far as the device check; there is no CPU path
        for i in range(4):
            assert _rc(_target(), outs=tuple(j == i for j in range(4))) == mcmc_amd.MI_ERR_NO_DEVICE


_TAILS = [(25, 5), (200, 40), (224, 44), (226, 45), (4100, 193), (120002, 1040), (2 ** 32 - 1, 196608)]


@pytest.mark.parametrize("K,M", _TAILS)
def test_tail_length(K, M):
    assert psis.tail_length(K) == M
    assert isinstance(psis.tail_length(K), int) and 5 <= M < K
    m3 = psis.tail_length(K) if M < K // 5 else None                      # the sqrt branch: the smallest integer whose square is >= 9 K
    if m3 is not None:
        assert m3 * m3 >= 9 * K > (m3 - 1) * (m3 - 1)
    n_keep, C_ = (1, K) if K < 2 ** 31 else (3, (2 ** 32 - 1) // 3)       # 2^32 - 1 = 3 * 1431655765
    assert n_keep * C_ == K
    plan = mcmc_amd.test_psis_plan(N, 2, 7, n_keep, C_)
    assert plan["M"] == M and plan["m"] == 30 + math.isqrt(M) == psis.fit_points(M)


def test_tail_length_is_exact_next_to_every_square():
    """9 K next to a square is where a floating-point 3 sqrt(K) would round the wrong way"""
    for r in (16, 30, 31, 1000, 65535, 196607, 196608):
        for K in range(max(25, (r * r) // 9 - 2), (r * r) // 9 + 3):
            want = min(K // 5, next(v for v in range(max(0, math.isqrt(9 * K) - 1), math.isqrt(9 * K) + 3) if v * v >= 9 * K))
            assert psis.tail_length(K) == want
            if K < 2 ** 32:
                assert mcmc_amd.test_psis_plan(N, 2, 1, 1, K)["M"] == want


def _ceil(a, b):
    return (a + b - 1) // b


def test_the_plan_is_the_stated_function_of_the_shape_and_the_budgets():
    lib = mcmc_amd
    try:
        # the real budgets: the measured shape is one group, its tail in LDS
        p = lib.test_psis_plan(L, 1024, 4096, 1, 65536, slab_host=False, target_host=False)
        assert (p["M"], p["m"], p["G"], p["n_groups"], p["last_rows"], p["tail_route"], p["lds_bytes"]) == (768, 57, 4096, 1, 4096, 0, 768 * 8)
        assert p["n_pieces"] == _ceil(65536 - 768, 16384) and p["piece"] == 16384 and p["ll_bytes"] == 4096 * 65536 * 8
        # 6.5 M draws x 4 096 rows: 213 GB of ll in groups of 128 rows that take 6.7 GB each with the sort beside them
        p = lib.test_psis_plan(L, 1024, 4096, 100, 65536, slab_host=False, target_host=False)
        assert p["G"] == 128 and p["n_groups"] == 32 and p["M"] == 7680 and p["tail_route"] == 0 and p["ll_bytes"] == 128 * 6553600 * 8
        # 300 rows of K = 100 under a budget of 128 rows of ll (and up to one byte short of 256): 128 + 128 + 44
        for budget in (128 * 100 * 8, 256 * 100 * 8 - 1):
            lib.test_set_psis_ll_bytes(budget)
            p = lib.test_psis_plan(N, 2, 300, 2, 50)
            assert (p["G"], p["n_groups"], p["last_rows"]) == (128, 3, 44), (budget, p)
        lib.test_set_psis_ll_bytes(256 * 100 * 8)
        p = lib.test_psis_plan(N, 2, 300, 2, 50)
        assert (p["G"], p["n_groups"], p["last_rows"]) == (256, 2, 44)
        lib.test_set_psis_ll_bytes(1)                                       # never fewer than 128 rows
        assert lib.test_psis_plan(N, 2, 300, 2, 50)["G"] == 128
        assert lib.test_psis_plan(N, 2, 100, 2, 50)["G"] == 100             # ... but at most n_rows
        lib.test_set_psis_ll_bytes(0)
        assert lib.test_psis_plan(N, 2, 300, 2, 50)["n_groups"] == 1
        # the tail route on both sides of the capacity: M = 260 at K = 7500
        assert psis.tail_length(7500) == 260
        for cap, route in ((0, 0), (260, 0), (259, 1), (128, 1)):
            lib.test_set_psis_lds_tail(cap)
            p = lib.test_psis_plan(N, 2, 21, 3, 2500)
            assert p["tail_route"] == route and p["lds_bytes"] == (0 if route else 260 * 8), (cap, p)
        lib.test_set_psis_lds_tail(0)
        # ... and of the real one, 8 192: M = 8 192 up to K = 7 456 540, 8 193 one sample later
        K0 = next(K for K in range(7456000, 7458000) if psis.tail_length(K) == 8192 and psis.tail_length(K + 1) == 8193)
        assert lib.test_psis_plan(N, 2, 1, 1, K0)["tail_route"] == 0 and lib.test_psis_plan(N, 2, 1, 1, K0 + 1)["tail_route"] == 1
    finally:
        lib.test_set_psis_ll_bytes(0)
        lib.test_set_psis_lds_tail(0)


def _pareto_row(k_true, K=20000, seed=11):
    u = (np.arange(K) + 0.5) / K
    ll = k_true * np.log(1.0 - u)                        # the ratios exp(-ll) = (1 - u)^(-k): exactly Pareto with shape k
    np.random.default_rng(seed).shuffle(ll)
    return ll[None, :]


def test_known_answers_on_exactly_pareto_ratios():
    assert psis.tail_length(20000) == 425
    got = {}
    for k_true in (0.1, 0.5, 0.9):
        elpd, pk = psis.psis_rows(_pareto_row(k_true), math=ORC_MATH)
        got[k_true] = (float(elpd[0]), float(pk[0]))
        print(f"k_true = {k_true}: khat = {pk[0]:.6f}, elpd_loo = {elpd[0]:.8f}, log(1 - k) = {math.log(1.0 - k_true):.8f}")
        assert abs(pk[0] - k_true) <= 0.02, (k_true, pk[0])
    assert got[0.1][1] < got[0.5][1] < got[0.9][1]
    # the exact value: -log of the ratios' mean, E (1 - u)^(-k) = 1 / (1 - k)
    assert abs(got[0.1][0] - math.log(1.0 - 0.1)) <= 1e-4
    assert abs(got[0.5][0] - math.log(1.0 - 0.5)) <= 5e-3


def test_a_constant_row_and_a_nan():
    c = -1.2345678901234567
    row = np.full((1, 64), c)
    elpd, pk = psis.psis_rows(row, math=ORC_MATH)
    assert pk[0] == np.inf
    # the stated expression on a constant row: W = 64 raw weights of exp(0) = 1, N = K
    want = (c + math.log(64.0)) - math.log(64.0)
    assert abs(elpd[0] - want) <= np.spacing(abs(want)), (elpd[0], want)
    two = np.vstack([row, np.linspace(-3.0, -1.0, 64)[None, :]])
    clean = psis.psis_rows(two, math=ORC_MATH)
    two[0, 7] = np.nan
    elpd, pk = psis.psis_rows(two, math=ORC_MATH)
    assert np.isnan(elpd[0]) and np.isnan(pk[0])
    assert elpd[1] == clean[0][1] and pk[1] == clean[1][1] and np.isfinite(pk[1])            # the other row is untouched
    for v in (np.inf, -np.inf):
        two[0, 7] = v
        elpd, pk = psis.psis_rows(two, math=ORC_MATH)
        assert np.isnan(elpd[0]) and np.isnan(pk[0]) and elpd[1] == clean[0][1]


def _rows(name, K, n_rows):
    """ll [n_rows, K] of a LOGISTIC / NORMAL_MODEL target at a random slab, over the oracle's arithmetic"""
    rng = np.random.default_rng(K + n_rows)
    if name == "logistic":
        d = 3
        X, y = synth.logistic_problem(d, n_rows)
        return waic.loglik(waic.LOGISTIC, rng.standard_normal((1, d, K)), y, X, math=ORC_MATH).reshape(n_rows, K)
    x = rng.standard_normal((1, 2, K))
    x[:, 1, :] = np.abs(x[:, 1, :]) + 0.5
    y = 1.5 + 2.0 * rng.standard_normal(n_rows)
    return waic.loglik(waic.NORMAL_MODEL, x, y, math=ORC_MATH).reshape(n_rows, K)


def _psis_libm(row):
    """include/mi_mcmc.h's definition, transcribed plainly over numpy's libm and np.sum"""
    s = np.sort(row)
    K = s.size
    M = psis.tail_length(K)
    n, m = float(M), 30 + math.isqrt(M)
    ec = np.exp(max(s[0] - s[M], psis.LOG_MIN_NORMAL))
    st = s[:M][::-1]
    x = np.exp(s[0] - st) - ec
    q, xM = x[(M + 2) // 4 - 1], x[M - 1]
    j = np.arange(1, m + 1)
    b = (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * q) + 1.0 / xM
    kj = np.log(1.0 - b[:, None] * x[None, :]).sum(axis=1) / n
    Lj = n * (np.log(-(b / kj)) - kj - 1.0)
    w = 1.0 / np.exp(Lj[None, :] - Lj[:, None]).sum(axis=1)
    keep = w >= psis.W_MIN
    w = w[keep] / w[keep].sum()
    bh = (b[keep] * w).sum()
    k0 = np.log(1.0 - bh * x).sum() / n
    sigma, kh = -k0 / bh, (n * k0 + 5.0) / (n + 10.0)
    p = (np.arange(1, M + 1) - 0.5) / n
    g = sigma * (np.exp(-kh * np.log(1.0 - p)) - 1.0) / kh
    t = np.minimum(np.log(g + ec), 0.0)
    W = np.exp(s[0] - s[M:]).sum() + np.exp(t).sum()
    Nn = float(K - M) + np.exp(t + (st - s[0])).sum()
    return (s[0] + np.log(Nn)) - np.log(W), kh


def _psis_mp(row):
    """the same formulas at 60 digits, with true log1p / expm1 and exact sums"""
    mp = mpmath.mp
    s = [mpmath.mpf(float(v)) for v in np.sort(row)]
    K = len(s)
    M = psis.tail_length(K)
    n, m = mpmath.mpf(M), 30 + math.isqrt(M)
    ec = mp.exp(max(s[0] - s[M], mpmath.mpf(psis.LOG_MIN_NORMAL)))
    st = s[:M][::-1]
    x = [mp.exp(s[0] - v) - ec for v in st]
    q, xM = x[(M + 2) // 4 - 1], x[M - 1]
    b = [(1 - mp.sqrt(mpmath.mpf(m) / (mpmath.mpf(j) - 0.5))) / (3 * q) + 1 / xM for j in range(1, m + 1)]
    kj = [mp.fsum(mp.log1p(-bj * xi) for xi in x) / n for bj in b]
    Lj = [n * (mp.log(-(bj / k)) - k - 1) for bj, k in zip(b, kj)]
    w = [1 / mp.fsum(mp.exp(Ll - Lme) for Ll in Lj) for Lme in Lj]
    keep = [wi >= psis.W_MIN for wi in w]
    sw = mp.fsum(wi for wi, kp in zip(w, keep) if kp)
    bh = mp.fsum(bj * wi / sw for bj, wi, kp in zip(b, w, keep) if kp)
    k0 = mp.fsum(mp.log1p(-bh * xi) for xi in x) / n
    sigma, kh = -k0 / bh, (n * k0 + 5) / (n + 10)
    t = []
    for jj in range(1, M + 1):
        p = (mpmath.mpf(jj) - 0.5) / n
        g = sigma * mp.expm1(-kh * mp.log1p(-p)) / kh
        t.append(min(mp.log(g + ec), mpmath.mpf(0)))
    W = mp.fsum(mp.exp(s[0] - v) for v in s[M:]) + mp.fsum(mp.exp(v) for v in t)
    Nn = (K - M) + mp.fsum(mp.exp(tj + (v - s[0])) for tj, v in zip(t, st))
    return (s[0] + mp.log(Nn)) - mp.log(W), kh


_ACC = [("normal", 25, 4), ("normal", 200, 4), ("normal", 4100, 3), ("logistic", 25, 4), ("logistic", 200, 4), ("logistic", 4100, 3)]
MP_ELPD_REL, MP_K_ABS, LIBM_ELPD_REL, LIBM_K_ABS = 1e-13, 1e-12, 1e-14, 1e-13


@pytest.mark.parametrize("name,K,n_rows", _ACC, ids=lambda v: str(v))
def test_the_mirror_over_the_library_arithmetic_agrees_with_60_digits_and_with_libm(name, K, n_rows):
    ll = _rows(name, K, n_rows)
    elpd, pk = psis.psis_rows(ll, math=ORC_MATH)
    assert np.isfinite(pk).all() and np.isfinite(elpd).all()              # the fitted path
    old = mpmath.mp.dps
    mpmath.mp.dps = 60
    try:
        worst = dict(mp_elpd=0.0, mp_k=0.0, libm_elpd=0.0, libm_k=0.0)
        for r in range(n_rows):
            e_mp, k_mp = _psis_mp(ll[r])
            e_lm, k_lm = _psis_libm(ll[r])
            worst["mp_elpd"] = max(worst["mp_elpd"], float(abs((mpmath.mpf(float(elpd[r])) - e_mp) / e_mp)))
            worst["mp_k"] = max(worst["mp_k"], float(abs(mpmath.mpf(float(pk[r])) - k_mp)))
            worst["libm_elpd"] = max(worst["libm_elpd"], abs((elpd[r] - e_lm) / e_lm))
            worst["libm_k"] = max(worst["libm_k"], abs(pk[r] - k_lm))
    finally:
        mpmath.mp.dps = old
    print(f"{name} K = {K}, {n_rows} rows: against 60 digits elpd {worst['mp_elpd']:.3e} relative, khat {worst['mp_k']:.3e} absolute; "
          f"against libm elpd {worst['libm_elpd']:.3e} relative, khat {worst['libm_k']:.3e} absolute")
    assert worst["mp_elpd"] <= MP_ELPD_REL and worst["libm_elpd"] <= LIBM_ELPD_REL, worst
    assert worst["mp_k"] <= MP_K_ABS and worst["libm_k"] <= LIBM_K_ABS, worst


def test_permuting_the_columns_changes_no_bit():
    ll = np.vstack([_rows("normal", 200, 3), _pareto_row(0.4, K=200), np.full((1, 200), -0.5)])
    ll[1, 50:100] = ll[1, 0:50]                                           # ties
    ref = psis.psis_ref(ll, math=ORC_MATH)
    rng = np.random.default_rng(5)
    for _ in range(3):
        got = psis.psis_rows(ll[:, rng.permutation(200)], math=ORC_MATH)
        for a, b in zip(got, (ref["elpd_loo"], ref["pareto_k"])):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    n_bad = sum(1 for k in ref["pareto_k"] if not k <= 0.7)
    assert ref["pareto_k"][4] == np.inf and ref["summary"][4] == n_bad >= 1               # n_bad counts the constant row
    assert ref["summary"][1] == ref["summary"][2] - ref["summary"][0]
