"""No GPU: mi_mcmc_draws_waic rejects bad arguments before any device call (MI_ERR_BAD_ARG / MI_ERR_UNSUPPORTED even where no device is visible -- a call
that reached the device probe would answer MI_ERR_NO_DEVICE there); the plan of a call (draws_waic.hpp: chunks, grids, LDS, workspace) is the stated
function of the shape and of what is staged; and mcmc_amd/waic.py, the numpy statement of the arithmetic, agrees with a brute-force computation on the
same ll values in exact rational arithmetic.

The bounds of the last part.  lppd = log(A / K): the mirror's A is a sum of K positive terms, each exp within an ulp, added in chains of at most 32 and a
tree of 6 levels, so its relative error is a few 2^-53, and log carries it over as an ABSOLUTE error of that size; the shapes keep |lppd| >= 1 (an
ulp of lppd is then >= 2^-52), where "4 ulp" leaves room for it.  p_waic: 1e-12 relative, four orders above the rounding of sums of K <= 4100 squares."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import waic

_X = np.zeros((2, 3, 4))
_ROWS = np.zeros((5, 3))
_Y = np.zeros(5)
_LPPD, _PW, _LL, _SUMM = np.zeros(5), np.zeros(5), np.zeros((5, 2, 4)), np.zeros(4)

ORC_MATH = dict(dot=lambda a, b: orc.dot(a, b, 1), exp=lambda x: orc.math_eval(0, x)[0], log=lambda x: orc.math_eval(1, x)[0],
                softplus=lambda x: orc.math_eval(3, x)[0])


def _target(kind=mcmc_amd.TARGET_LOGISTIC, d=3, prec=None, X=_ROWS, y=_Y, n_rows=None, struct_size=None):
    t = mcmc_amd.make_target(kind, d, prec=prec, X=X, y=y)
    if n_rows is not None:
        t.n_rows = n_rows
    if struct_size is not None:
        t.struct_size = struct_size
    return t


def _rc(target, slab=_X.ctypes.data, n_keep=2, n_chains=4, outs=(True, True, True, True)):
    ptrs = [a.ctypes.data if on else None for a, on in zip((_LPPD, _PW, _LL, _SUMM), outs)]
    return mcmc_amd.lib().mi_mcmc_draws_waic(None if target is None else C.byref(target), slab, mcmc_amd.MEM_HOST,
                                            n_keep, n_chains, *[p for p in ptrs], None)


_NORMAL = dict(kind=mcmc_amd.TARGET_NORMAL_MODEL, d=2, X=None)
_BAD = {
    "null_target": (None, {}, "target"),
    "null_slab": ({}, dict(slab=None), "slab"),
    "all_outputs_null": ({}, dict(outs=(False, False, False, False)), "all NULL"),
    "struct_size": (dict(struct_size=3), {}, "struct_size"),
    "d_is_0": (dict(d=0), {}, "d "),
    "n_keep_is_0": ({}, dict(n_keep=0), "K "),
    "n_chains_is_0": ({}, dict(n_chains=0), "K "),
    "K_is_1": ({}, dict(n_keep=1, n_chains=1), "K = n_keep * n_chains = 1"),
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
def test_waic_rejects_bad_arguments_without_a_gpu(case):
    tkw, kw, names = _BAD[case]
    target = None if tkw is None else _target(**tkw)
    assert _rc(target, **kw) == mcmc_amd.MI_ERR_BAD_ARG
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_waic:") and names in msg, msg


@pytest.mark.parametrize("kind,prec", [(mcmc_amd.TARGET_GAUSS_ISO, None), (mcmc_amd.TARGET_GAUSS_DIAG, np.ones(3)), (mcmc_amd.TARGET_GAUSS_DENSE, np.eye(3)),
                                       (mcmc_amd.TARGET_GAUSS_MIXTURE, np.ones(5))], ids=["iso", "diag", "dense", "mixture"])
def test_targets_without_observations_are_unsupported_without_a_gpu(kind, prec):
    assert _rc(_target(kind=kind, prec=prec)) == mcmc_amd.MI_ERR_UNSUPPORTED
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_waic:") and "no observations" in msg, msg


def test_each_single_output_is_a_valid_request_and_the_entry_is_exported():
    assert "mi_mcmc_draws_waic" in mcmc_amd.EXPORTS and hasattr(mcmc_amd.lib(), "mi_mcmc_draws_waic")
    assert hasattr(mcmc_amd.lib(), "mi_mcmc_test_waic_plan")
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_waic(_target(X=None, n_rows=5), _X)
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(ValueError):
        mcmc_amd.draws_waic(_target(), np.zeros((2, 4, 4)))               # the slab's d is not the target's
    if mcmc_amd.lib().mi_mcmc_device_count() == 0:
        for i in range(4):                                                 # valid calls: no CPU path
            assert _rc(_target(), outs=tuple(j == i for j in range(4))) == mcmc_amd.MI_ERR_NO_DEVICE


def _ceil(a, b):
    return (a + b - 1) // b


def _a256(n):
    return _ceil(n, 256) * 256


def _want_plan(kind, d, n_rows, n_keep, C_, slab_host, target_host, want_loglik):
    """draws_waic.hpp's statement, restated"""
    K = n_keep * C_
    product = kind == mcmc_amd.TARGET_LOGISTIC
    n_chunks, ldR = _ceil(K, 2048), 128 * _ceil(n_rows, 128)
    w = dict(route=int(product), chunk=2048, n_chunks=n_chunks, ldR=ldR, merge_grid=_ceil(n_rows, 256))
    if product:
        w.update(grid=n_chunks * (ldR // 128), block=512, lds_bytes=2 * 32 * 144 * 8 + 2 * 128 * 8, Kp=16 * _ceil(d, 16))
        pack, mat = w["Kp"] * ldR * 8, n_rows * d
    else:
        w.update(grid=n_chunks * _ceil(n_rows, 16), block=256, lds_bytes=0, Kp=0)
        pack, mat = 0, 0
    ws = _a256(pack) + _a256(n_chunks * 4 * ldR * 8) + 2 * _a256(ldR * 8)
    if target_host:
        ws += _a256(mat * 8) + _a256(n_rows * 8)
    if slab_host:
        ws += _a256(K * d * 8) + (_a256(K * n_rows * 8) if want_loglik else 0)
    w["ws_bytes"] = ws
    return w


L, N = mcmc_amd.TARGET_LOGISTIC, mcmc_amd.TARGET_NORMAL_MODEL
# (kind, d, n_rows, n_keep, C): the GPU tests' shapes, then the measured ones (K = 65 536, and the 6.5 M draws of the issue)
PLAN_SHAPES = [(L, 3, 5, 2, 5), (L, 70, 130, 3, 37), (L, 520, 70, 1, 19), (L, 5, 9, 3, 1366), (L, 32, 16, 2, 5), (N, 2, 50, 4, 37), (N, 2, 21, 3, 1366),
               (L, 1024, 4096, 1, 65536), (L, 1024, 4096, 16, 65536), (L, 1024, 4096, 100, 65536)]


@pytest.mark.parametrize("staged", [(True, True, True), (True, True, False), (False, False, True), (False, True, False)],
                         ids=["host_with_ll", "host", "device_with_ll", "device_slab_host_target"])
@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_the_plan_is_the_stated_function_of_the_shape(shape, staged):
    got = mcmc_amd.test_waic_plan(*shape, slab_host=staged[0], target_host=staged[1], want_loglik=staged[2])
    assert got == _want_plan(*shape, *staged)
    assert got == mcmc_amd.test_waic_plan(*shape, slab_host=staged[0], target_host=staged[1], want_loglik=staged[2])        # nothing else enters


def test_the_chunks_cover_every_column_once_and_the_partials_stay_small():
    for shape in PLAN_SHAPES:
        p = mcmc_amd.test_waic_plan(*shape, slab_host=False, target_host=False)
        K = shape[3] * shape[4]
        assert (p["n_chunks"] - 1) * p["chunk"] < K <= p["n_chunks"] * p["chunk"]
        assert p["grid"] < 2 ** 31 and p["lds_bytes"] <= 160 * 1024 and p["chunk"] % 128 == 0
    # 6.5 M draws x 4 096 rows: the matrix is 213 GB, a partial per 128 columns would be 6.7 GB; the chunk partials are 32 bytes per (chunk, row)
    p = mcmc_amd.test_waic_plan(L, 1024, 4096, 100, 65536, slab_host=False, target_host=False)
    assert p["ws_bytes"] - 1024 * 4096 * 8 < 2 ** 29


def test_every_column_has_one_slot_and_one_place_in_it():
    o = np.arange(2048)
    s = waic.slot(o)
    assert s.min() == 0 and s.max() == 63 and (np.bincount(s) == 32).all()
    assert (waic.slot(o[:128]) == 16 * (o[:128] // 32) + o[:128] % 16).all()


def _exact(ll):
    """(lppd, p_waic) of ll [R, K]: the sums in exact arithmetic, rounded once at the end"""
    R, K = ll.shape
    lppd, pw = np.empty(R), np.empty(R)
    for r in range(R):
        A = math.fsum(math.exp(v) for v in ll[r])
        lppd[r] = math.log(A / K)
        f = [Fraction(float(v)) for v in ll[r]]
        mean = sum(f) / K
        pw[r] = float(sum((v - mean) ** 2 for v in f) / (K - 1))
    return lppd, pw


_BRUTE = [("normal", (4, 2, 37), 50), ("normal", (3, 2, 1366), 7), ("logistic", (2, 5, 130), 9)]


@pytest.mark.parametrize("name,shape,n_rows", _BRUTE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_mirror_agrees_with_exact_arithmetic_on_the_same_ll(name, shape, n_rows):
    rng = np.random.default_rng(shape[0] * 7919 + shape[2])
    x = rng.standard_normal(shape)
    if name == "normal":
        x[:, 1, :] = np.abs(x[:, 1, :]) + 2.0                               # sigma >= 2: ll <= -(0.5 log 2 pi + log 2) = -1.6, so |lppd| >= 1
        y = 1.5 + 2.0 * rng.standard_normal(n_rows)
        ll = waic.loglik(waic.NORMAL_MODEL, x, y, math=ORC_MATH)
    else:
        X = rng.standard_normal((n_rows, shape[1]))
        X[:, 0] = 3.0                                                       # with x_0 = -1: an intercept of -3 under y = 1, ll = -softplus(3 - ...) about -3
        x[:, 0, :] = -1.0
        y = np.ones(n_rows)
        ll = waic.loglik(waic.LOGISTIC, x, y, X, math=ORC_MATH)
    K = shape[0] * shape[2]
    lppd, pw = waic.row_stats(ll, math=ORC_MATH)
    want_lppd, want_pw = _exact(ll.reshape(n_rows, K))
    assert (np.abs(want_lppd) >= 1.0).all()
    ulps = np.abs(lppd - want_lppd) / np.spacing(np.abs(want_lppd))
    rel = np.abs(pw - want_pw) / want_pw
    print(f"{name} {shape} rows={n_rows}: lppd off by at most {ulps.max():.2f} ulp, p_waic by {rel.max():.3e} relative")
    assert ulps.max() <= 4.0, ulps.max()
    assert rel.max() <= 1e-12, rel.max()
    # the summary: its own definition, against exact sums of the mirror's rows
    s = waic.summary(lppd, pw)
    e = lppd - pw
    assert s[0] == pytest.approx(math.fsum(e), rel=1e-14) and s[1] == pytest.approx(math.fsum(pw), rel=1e-14) and s[2] == pytest.approx(math.fsum(lppd), rel=1e-14)
    assert s[3] == pytest.approx(math.sqrt(n_rows * np.var(e, ddof=1)), rel=1e-12)
    assert np.isnan(waic.summary(lppd[:1], pw[:1])[3])                      # one row: no variance
