"""GPU: mi_mcmc_draws_waic -- the pointwise log-likelihood ll[r][k] of every data row at every column of a slab [n_keep][d][C], lppd_r, p_waic_r and the
WAIC summary (mcmc_amd/csrc/draws_waic.hip) against mcmc_amd/waic.py, the numpy statement of include/mi_mcmc.h's definition, run over the CPU oracle's
arithmetic (orc.dot(x, y, 1): the fma chain; orc.math_eval 0 / 1 / 3: exp / log / softplus).  BIT FOR BIT: outputs are compared as uint64 and any NaN
matches any NaN; the two tolerances in this file are the composition with draw_stats (another summation order: 1e-13) and the stability bound
(1e-9 against the exactly rounded variance, see there).

A workgroup of the product kernel owns a 128-row tile and a chunk of 2048 columns, and walks column tiles of 128 with the contraction in steps of 16.
Which shape (n_keep, d, C) reaches what:
  LOGISTIC (2, 3, 5), 5 rows       K = 10, below every tile: 54 of the 64 slots stay empty
           (3, 70, 37), 130 rows   two row tiles, the second with 2 rows; a ragged contraction; a column tile that spans t; an odd C
           (1, 520, 19), 70 rows   33 contraction steps
           (3, 5, 1366), 9 rows    K = 4098 = 2 * 2048 + 2: three chunks, the last with two columns
           (2, 32, 5), 16 rows     d a multiple of 16: a contraction of full steps only, no ragged last step
  NORMAL_MODEL (4, 2, 37), 50 rows    K = 148: two column tiles, four row groups of 16, the last with 2 rows
               (3, 2, 1366), 21 rows  three chunks, the last with two columns"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import synth, waic

pytestmark = pytest.mark.gpu

ORC_MATH = dict(dot=lambda a, b: orc.dot(a, b, 1), exp=lambda x: orc.math_eval(0, x)[0], log=lambda x: orc.math_eval(1, x)[0],
                softplus=lambda x: orc.math_eval(3, x)[0])
LOGIT_SHAPES = [((2, 3, 5), 5), ((3, 70, 37), 130), ((1, 520, 19), 70), ((3, 5, 1366), 9)]
NORMAL_SHAPES = [((4, 2, 37), 50), ((3, 2, 1366), 21)]
FULL_STEPS = ((2, 32, 5), 16)            # d a multiple of 16; behind the others, which the tests below pick by index
CASES = [("logistic", s, r) for s, r in LOGIT_SHAPES] + [("normal", s, r) for s, r in NORMAL_SHAPES] + [("logistic",) + FULL_STEPS]
_IDS = [f"{n}-{'x'.join(map(str, s))}-{r}rows" for n, s, r in CASES]
_KIND = {"logistic": (mcmc_amd.TARGET_LOGISTIC, waic.LOGISTIC), "normal": (mcmc_amd.TARGET_NORMAL_MODEL, waic.NORMAL_MODEL)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """bit patterns; any NaN matches any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb]))


def _assert_same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((np.isnan(got) & np.isnan(want)) | (_bits(got) == _bits(want)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _slab(name, shape):
    rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2])
    x = rng.standard_normal(shape)
    if name == "normal":
        x[:, 1, :] = np.abs(x[:, 1, :]) + 0.5            # sigma > 0
    return _frozen(x)[0]


@functools.lru_cache(maxsize=None)
def _problem(name, d, n_rows):
    """(X, y) of a target, read-only"""
    if name == "logistic":
        return _frozen(*synth.logistic_problem(d, n_rows))
    return _frozen(None, 1.5 + 2.0 * np.random.default_rng(n_rows).standard_normal(n_rows))


def _target(name, d, n_rows):
    X, y = _problem(name, d, n_rows)
    return mcmc_amd.make_target(_KIND[name][0], d, X=X, y=y)


def _mirror(name, slab, n_rows):
    X, y = _problem(name, slab.shape[1], n_rows)
    return waic.waic_ref(_KIND[name][1], slab, y, X, math=ORC_MATH)


@functools.lru_cache(maxsize=None)
def _reference(name, shape, n_rows):
    ref = _mirror(name, _slab(name, shape), n_rows)
    _frozen(*ref.values())
    return ref


def _summary(res):
    return np.array([res["summary"][k] for k in ("elpd_waic", "p_waic", "lppd", "se_elpd")])


def _assert_result(res, ref, what):
    if res["loglik"] is not None:
        _assert_same(res["loglik"], ref["loglik"], (what, "loglik"))
    if res["lppd"] is not None:
        _assert_same(res["lppd"], ref["lppd"], (what, "lppd"))
    if res["p_waic"] is not None:
        _assert_same(res["p_waic"], ref["p_waic"], (what, "p_waic"))
    if res["summary"] is not None:
        _assert_same(_summary(res), ref["summary"], (what, "summary"))


@pytest.mark.parametrize("name,shape,n_rows", CASES, ids=_IDS)
def test_row_terms_and_statistics_are_the_mirror_bit_for_bit(name, shape, n_rows):
    res = mcmc_amd.draws_waic(_target(name, shape[1], n_rows), _slab(name, shape), want_loglik=True)
    ref = _reference(name, shape, n_rows)
    assert res["loglik"].shape == (n_rows, shape[0], shape[2])
    _assert_result(res, ref, (name, shape))
    assert np.isfinite(res["loglik"]).all() and np.isfinite(res["lppd"]).all() and (res["p_waic"] > 0.0).all() and np.isfinite(_summary(res)).all()


def _sum4(a):
    q = [0.0, 0.0, 0.0, 0.0]
    for i, v in enumerate(a):
        q[i % 4] = q[i % 4] + float(v)
    return (q[0] + q[2]) + (q[1] + q[3])


@pytest.mark.parametrize("shape,n_rows", LOGIT_SHAPES[:3], ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else f"{s}rows")
def test_the_logistic_row_terms_sum_to_the_log_kernel_of_the_merged_reducer(shape, n_rows):
    """sum4 over r of loglik[:, t, c] minus 0.5 dot4(x, x) is mi_mcmc_draws_log_kernel's value: the two kernels form the same term_r, without the mirror"""
    tgt, slab = _target("logistic", shape[1], n_rows), _slab("logistic", shape)
    ll = mcmc_amd.draws_waic(tgt, slab, want_lppd=False, want_p_waic=False, want_loglik=True, want_summary=False)["loglik"]
    lp = mcmc_amd.draws_log_kernel(tgt, slab)
    want = np.empty_like(lp)
    for t in range(shape[0]):
        for c in range(shape[2]):
            x = np.ascontiguousarray(slab[t, :, c])
            want[t, c] = _sum4(ll[:, t, c]) - 0.5 * orc.dot(x, x, 4)
    _assert_same(lp, want, shape)


@pytest.mark.parametrize("name,shape,n_rows", [CASES[1], CASES[4]], ids=[_IDS[1], _IDS[4]])
def test_every_call_variant_gives_the_same_bits(name, shape, n_rows):
    import torch
    ref = _reference(name, shape, n_rows)
    slab = _slab(name, shape)
    n, d, C_ = shape
    tgt = _target(name, d, n_rows)
    # a host slab, each output alone (the other three NULL)
    for k in ("lppd", "p_waic", "loglik", "summary"):
        res = mcmc_amd.draws_waic(tgt, slab, want_lppd=k == "lppd", want_p_waic=k == "p_waic", want_loglik=k == "loglik", want_summary=k == "summary")
        assert [j for j in res if res[j] is not None] == [k]
        _assert_result(res, ref, ("host slab, only", k))
    # a device slab with a host target, then with a device target; every output NULL in turn
    dev = torch.from_numpy(np.array(slab)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    X, y = _problem(name, d, n_rows)
    y_dev = torch.from_numpy(np.array(y)).cuda()
    X_dev = None if X is None else torch.from_numpy(np.array(X)).cuda()
    tgt_dev = mcmc_amd.make_target(_KIND[name][0], d, X=X_dev, y=y_dev, mem=mcmc_amd.MEM_DEVICE)
    tgt_dev.n_rows = n_rows
    for target, what in ((tgt, "host target"), (tgt_dev, "device target")):
        for skip in (None, "lppd", "p_waic", "loglik", "summary"):
            outs = dict(lppd=torch.full((n_rows,), -7.0, dtype=torch.float64, device="cuda"), p_waic=torch.full((n_rows,), -7.0, dtype=torch.float64, device="cuda"),
                        loglik=torch.full((n_rows, n, C_), -7.0, dtype=torch.float64, device="cuda"))
            if skip in outs:
                outs[skip] = None
            res = mcmc_amd.draws_waic(target, dev, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, want_summary=skip != "summary", **outs)
            torch.cuda.synchronize()
            got = {k: (None if v is None else v.cpu().numpy()) for k, v in outs.items()}
            got["summary"] = res["summary"]
            assert (got["summary"] is None) == (skip == "summary")
            _assert_result(got, ref, ("device slab", what, "without", skip))
    assert np.array_equal(dev.cpu().numpy(), slab)                              # the slab is read only


def test_a_row_of_loglik_is_a_slab_the_diagnostics_take():
    name, shape, n_rows = CASES[1]
    ref = _reference(name, shape, n_rows)
    ll = mcmc_amd.draws_waic(_target(name, shape[1], n_rows), _slab(name, shape), want_loglik=True)["loglik"]
    K = shape[0] * shape[2]
    for r in (0, 77, 129):
        row = ll[r].reshape(shape[0], 1, shape[2])                             # [n_keep][1][C]: as it is
        s = mcmc_amd.draw_stats(row)
        want = float(np.sum(ref["loglik"][r].astype(np.longdouble)) / K)
        assert abs(s["mean"][0] - want) <= 1e-13 * abs(want), (r, s["mean"][0], want)
        q = mcmc_amd.draws_quantiles(row, [0.5])
        assert q.shape == (1, 1) and ll[r].min() <= q[0, 0] <= ll[r].max()


def _exact_variance(ll_row):
    f = [Fraction(float(v)) for v in ll_row]
    K = len(f)
    mean = sum(f) / K
    return float(sum((v - mean) ** 2 for v in f) / (K - 1)), float(mean)


@pytest.mark.parametrize("K", [37, 200, 4100])
def test_p_waic_is_stable_where_the_mean_dwarfs_the_spread(K):
    """Logistic rows with y = 0 and eta = X_r (30 + 1e-4 N(0, 1)): ll is about -30 with a spread of 1e-4, mean^2 / variance >= 1e10 in every row.
    p_waic within 1e-9 relative of the exactly rounded sample variance of the same ll values: the textbook one-pass formula is off by 2.6e-6 to 6.4e-6
    on this input, shifted sums and Welford by <= 2e-11 (both computed on the CPU at these three K)."""
    rng = np.random.default_rng(K)
    slab = (30.0 + 1e-4 * rng.standard_normal((1, 1, K)))
    X = np.array([[1.0], [1.03125], [0.96875]])
    y = np.zeros(3)
    tgt = mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, 1, X=X, y=y)
    res = mcmc_amd.draws_waic(tgt, slab, want_loglik=True)
    ref = waic.waic_ref(waic.LOGISTIC, slab, y, X, math=ORC_MATH)
    _assert_same(res["loglik"], ref["loglik"], "loglik")
    _assert_same(res["p_waic"], ref["p_waic"], "p_waic")
    _assert_same(res["lppd"], ref["lppd"], "lppd")
    for r in range(3):
        var, mean = _exact_variance(ref["loglik"][r].ravel())
        assert mean * mean / var >= 1e10, (r, mean, var)
        rel = abs(res["p_waic"][r] - var) / var
        print(f"K = {K} row {r}: mean^2 / var = {mean * mean / var:.3e}, p_waic off by {rel:.3e} relative")
        assert rel <= 1e-9, (K, r, res["p_waic"][r], var, rel)


@pytest.mark.parametrize("name,shape,n_rows", [CASES[1], CASES[4]], ids=[_IDS[1], _IDS[4]])
def test_non_finite_draws_propagate_and_stay_in_their_own_column(name, shape, n_rows):
    n, d, C_ = shape
    x = np.array(_slab(name, shape))
    x[1, :, 5] = np.nan
    x[n - 1, :, 20] = 1e308
    touched = np.zeros((n, C_), dtype=bool)
    touched[1, 5] = touched[n - 1, 20] = True
    res = mcmc_amd.draws_waic(_target(name, d, n_rows), x, want_loglik=True)
    ref = _mirror(name, x, n_rows)
    _assert_result(res, ref, "the touched columns included")
    assert np.isnan(ref["loglik"][:, 1, 5]).all()                                # the NaN column did something, in every row
    assert not np.array_equal(_bits(ref["loglik"][:, n - 1, 20]), _bits(_reference(name, shape, n_rows)["loglik"][:, n - 1, 20]))      # and so did 1e308
    clean = _reference(name, shape, n_rows)["loglik"]
    assert np.array_equal(_bits(res["loglik"])[:, ~touched], _bits(clean)[:, ~touched])       # every other column: the untouched run
    assert np.isfinite(res["loglik"][:, ~touched]).all()
    assert np.isnan(res["p_waic"]).all()                                         # a NaN among a row's K values: by the IEEE rules, nothing is filtered


def test_the_result_does_not_depend_on_the_call():
    import torch
    name, shape, n_rows = CASES[3]                                               # three chunks
    n, d, C_ = shape
    ref = _reference(name, shape, n_rows)
    tgt, slab = _target(name, d, n_rows), _slab(name, shape)
    dev = torch.from_numpy(np.array(slab)).cuda()

    def run(stream):
        outs = dict(lppd=torch.zeros(n_rows, dtype=torch.float64, device="cuda"), p_waic=torch.zeros(n_rows, dtype=torch.float64, device="cuda"),
                    loglik=torch.zeros((n_rows, n, C_), dtype=torch.float64, device="cuda"))
        res = mcmc_amd.draws_waic(tgt, dev, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=stream.cuda_stream, **outs)
        stream.synchronize()
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        got["summary"] = res["summary"]
        return got

    torch.cuda.synchronize()
    a = run(torch.cuda.Stream())
    b = run(torch.cuda.Stream())
    mcmc_amd.release_workspace()
    c = run(torch.cuda.current_stream())
    for got, what in ((a, "stream 1"), (b, "stream 2"), (c, "after release_workspace")):
        _assert_result(got, ref, what)
