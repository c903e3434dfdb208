"""GPU: mi_mcmc_draws_psis_loo -- PSIS-LOO elpd_loo_r and the Pareto shape pareto_k_r of every data row of a slab [n_keep][d][C], with lppd_r and the
summary (mcmc_amd/csrc/draws_psis.hip behind draws_waic.hip and draws_rank.hip) against mcmc_amd/psis.py, the numpy statement of include/mi_mcmc.h's
definition, run over the CPU oracle's arithmetic as in test_gpu_draws_waic.py.  BIT FOR BIT: outputs are compared as uint64 and any NaN matches any NaN;
there is no tolerance in this file.

Which shape (n_keep, d, C) x n_rows reaches what (K = n_keep C samples, M the tail, m the fit points):
  LOGISTIC (1, 3, 25) x 5          the smallest K, M = 5: 251 of the 256 slots of a tail sum stay empty
           (2, 70, 100) x 130      M = K div 5 = 40; two row tiles of the product, the second ragged
           (3, 5, 1366) x 9        the sqrt branch, K = 4098, M = 193; three WAIC chunks
           (1, 520, 37) x 70       33 contraction steps
  NORMAL_MODEL (4, 2, 37) x 50     M = 29
               (3, 2, 2500) x 21   M = 260: a tail longer than the 256 slots; under the hook the route that re-reads it
               (2, 2, 60001) x 3   M = 1040; a body of 118 962 values = 8 pieces, the last one ragged
  300 rows under a lowered block budget: three row groups, 128 + 128 + 44, for both kinds (LOGISTIC: the sub-target X + r0 d)"""
import functools

import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import psis, synth, waic

pytestmark = pytest.mark.gpu

ORC_MATH = dict(dot=lambda a, b: orc.dot(a, b, 1), exp=lambda x: orc.math_eval(0, x)[0], log=lambda x: orc.math_eval(1, x)[0],
                softplus=lambda x: orc.math_eval(3, x)[0])
CASES = [("logistic", (1, 3, 25), 5), ("logistic", (2, 70, 100), 130), ("logistic", (3, 5, 1366), 9), ("logistic", (1, 520, 37), 70),
         ("normal", (4, 2, 37), 50), ("normal", (3, 2, 2500), 21), ("normal", (2, 2, 60001), 3)]
_IDS = [f"{n}-{'x'.join(map(str, s))}-{r}rows" for n, s, r in CASES]
GROUP_CASES = [("normal", (2, 2, 50), 300), ("logistic", (1, 5, 40), 300)]
_KIND = {"logistic": (mcmc_amd.TARGET_LOGISTIC, waic.LOGISTIC), "normal": (mcmc_amd.TARGET_NORMAL_MODEL, waic.NORMAL_MODEL)}
_SUMMARY = ("elpd_loo", "p_loo", "lppd", "se_elpd_loo", "n_bad")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


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


def _target(name, d, n_rows, y=None):
    X, y0 = _problem(name, d, n_rows)
    return mcmc_amd.make_target(_KIND[name][0], d, X=X, y=y0 if y is None else y)


def _mirror(name, slab, n_rows, y=None):
    X, y0 = _problem(name, slab.shape[1], n_rows)
    ll = waic.loglik(_KIND[name][1], slab, y0 if y is None else y, X, math=ORC_MATH)
    return psis.psis_ref(ll, math=ORC_MATH)


@functools.lru_cache(maxsize=None)
def _reference(name, shape, n_rows):
    ref = _mirror(name, _slab(name, shape), n_rows)
    _frozen(*ref.values())
    return ref


def _summary(res):
    return np.array([res["summary"][k] for k in _SUMMARY])


def _assert_result(res, ref, what):
    for k in ("elpd_loo", "pareto_k", "lppd"):
        if res[k] is not None:
            _assert_same(res[k], ref[k], (what, k))
    if res["summary"] is not None:
        _assert_same(_summary(res), ref["summary"], (what, "summary"))


@pytest.mark.parametrize("name,shape,n_rows", CASES, ids=_IDS)
def test_every_output_is_the_mirror_bit_for_bit(name, shape, n_rows):
    ref = _reference(name, shape, n_rows)
    assert np.isfinite(ref["pareto_k"]).all() and np.isfinite(ref["elpd_loo"]).all()        # the fitted path is what is compared
    K = shape[0] * shape[2]
    plan = mcmc_amd.test_psis_plan(_KIND[name][0], shape[1], n_rows, shape[0], shape[2])
    assert plan["M"] == psis.tail_length(K) and plan["n_groups"] == 1 and plan["tail_route"] == 0
    res = mcmc_amd.draws_psis_loo(_target(name, shape[1], n_rows), _slab(name, shape))
    _assert_result(res, ref, (name, shape))
    assert res["summary"]["n_bad"] == np.count_nonzero(~(ref["pareto_k"] <= 0.7))


@pytest.mark.parametrize("name,shape,n_rows", GROUP_CASES, ids=["normal", "logistic"])
def test_row_groups_give_the_bits_of_one_group(name, shape, n_rows):
    K = shape[0] * shape[2]
    kind = _KIND[name][0]
    tgt, slab = _target(name, shape[1], n_rows), _slab(name, shape)
    ref = _reference(name, shape, n_rows)
    assert mcmc_amd.test_psis_plan(kind, shape[1], n_rows, shape[0], shape[2])["n_groups"] == 1
    one = mcmc_amd.draws_psis_loo(tgt, slab)
    _assert_result(one, ref, (name, "one group"))
    try:
        mcmc_amd.test_set_psis_ll_bytes(128 * K * 8 + 17)
        plan = mcmc_amd.test_psis_plan(kind, shape[1], n_rows, shape[0], shape[2])
        assert (plan["G"], plan["n_groups"], plan["last_rows"]) == (128, 3, 44)
        three = mcmc_amd.draws_psis_loo(tgt, slab)
    finally:
        mcmc_amd.test_set_psis_ll_bytes(0)
    _assert_result(three, ref, (name, "128 + 128 + 44"))


def test_the_tail_re_read_from_the_sorted_row_gives_the_bits_of_the_tail_in_lds():
    name, shape, n_rows = CASES[5]
    kind = _KIND[name][0]
    ref = _reference(name, shape, n_rows)
    try:
        mcmc_amd.test_set_psis_lds_tail(128)
        plan = mcmc_amd.test_psis_plan(kind, shape[1], n_rows, shape[0], shape[2])
        assert plan["M"] == 260 and plan["tail_route"] == 1 and plan["lds_bytes"] == 0
        res = mcmc_amd.draws_psis_loo(_target(name, shape[1], n_rows), _slab(name, shape))
    finally:
        mcmc_amd.test_set_psis_lds_tail(0)
    assert mcmc_amd.test_psis_plan(kind, shape[1], n_rows, shape[0], shape[2])["tail_route"] == 0
    _assert_result(res, ref, "the tail in device memory")


@pytest.mark.parametrize("name,shape,n_rows", [CASES[1], CASES[4]], ids=[_IDS[1], _IDS[4]])
def test_every_call_variant_gives_the_same_bits(name, shape, n_rows):
    import torch
    ref = _reference(name, shape, n_rows)
    slab = _slab(name, shape)
    n, d, C_ = shape
    tgt = _target(name, d, n_rows)
    outs_names = ("elpd_loo", "pareto_k", "lppd")
    # a host slab, each output alone (the other three NULL)
    for k in outs_names + ("summary",):
        res = mcmc_amd.draws_psis_loo(tgt, slab, want_elpd_loo=k == "elpd_loo", want_pareto_k=k == "pareto_k", want_lppd=k == "lppd", want_summary=k == "summary")
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
        for skip in (None,) + outs_names + ("summary",):
            outs = {k: torch.full((n_rows,), -7.0, dtype=torch.float64, device="cuda") for k in outs_names}
            if skip in outs:
                outs[skip] = None
            res = mcmc_amd.draws_psis_loo(target, dev, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, want_summary=skip != "summary", **outs)
            torch.cuda.synchronize()
            got = {k: (None if v is None else v.cpu().numpy()) for k, v in outs.items()}
            got["summary"] = res["summary"]
            assert (got["summary"] is None) == (skip == "summary")
            _assert_result(got, ref, ("device slab", what, "without", skip))
    assert np.array_equal(dev.cpu().numpy(), slab)                              # the slab is read only


def test_the_result_does_not_depend_on_the_stream_or_the_cached_workspace():
    import torch
    name, shape, n_rows = CASES[2]
    n, d, C_ = shape
    ref = _reference(name, shape, n_rows)
    tgt = _target(name, d, n_rows)
    dev = torch.from_numpy(np.array(_slab(name, shape))).cuda()

    def run(stream):
        outs = {k: torch.zeros(n_rows, dtype=torch.float64, device="cuda") for k in ("elpd_loo", "pareto_k", "lppd")}
        res = mcmc_amd.draws_psis_loo(tgt, dev, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=stream.cuda_stream, **outs)
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


@pytest.mark.parametrize("name,shape,n_rows", [CASES[1], CASES[4]], ids=[_IDS[1], _IDS[4]])
def test_lppd_is_waics_and_the_rest_depends_on_the_multiset_only(name, shape, n_rows):
    tgt, slab = _target(name, shape[1], n_rows), _slab(name, shape)
    res = mcmc_amd.draws_psis_loo(tgt, slab)
    _assert_same(res["lppd"], mcmc_amd.draws_waic(tgt, slab)["lppd"], "lppd")
    perm = np.random.default_rng(3).permutation(shape[2])
    shuffled = mcmc_amd.draws_psis_loo(tgt, np.ascontiguousarray(slab[:, :, perm])[::-1].copy())     # the chains permuted, and the draws reversed
    _assert_same(shuffled["elpd_loo"], res["elpd_loo"], "elpd_loo of the permuted slab")
    _assert_same(shuffled["pareto_k"], res["pareto_k"], "pareto_k of the permuted slab")
    assert shuffled["summary"]["elpd_loo"] == res["summary"]["elpd_loo"] and shuffled["summary"]["n_bad"] == res["summary"]["n_bad"]


@pytest.mark.parametrize("name,shape,n_rows", [CASES[1], CASES[4]], ids=[_IDS[1], _IDS[4]])
def test_ties_and_a_degenerate_tail(name, shape, n_rows):
    n, d, C_ = shape
    K = n * C_
    tgt = _target(name, d, n_rows)
    # every column equal: nothing can be fitted
    x = np.array(_slab(name, shape))
    x[:] = x[0, :, 0][None, :, None]
    res = mcmc_amd.draws_psis_loo(tgt, x)
    ref = _mirror(name, x, n_rows)
    assert (ref["pareto_k"] == np.inf).all() and np.isfinite(ref["elpd_loo"]).all()
    _assert_result(res, ref, "all columns equal")
    assert res["summary"]["n_bad"] == n_rows
    # a quarter of the columns duplicated: ties everywhere in the sorted row, and still a fit
    x = np.array(_slab(name, shape))
    q = C_ // 4
    x[:, :, q:2 * q] = x[:, :, 0:q]
    res = mcmc_amd.draws_psis_loo(tgt, x)
    ref = _mirror(name, x, n_rows)
    assert np.isfinite(ref["pareto_k"]).all()
    _assert_result(res, ref, "a quarter of the columns duplicated")


def test_non_finite_draws_make_their_rows_nan_and_the_call_succeeds():
    # LOGISTIC: X of mixed signs; a NaN column and a 1e308 column reach every row
    name, shape, n_rows = CASES[1]
    n, d, C_ = shape
    X, _ = _problem(name, d, n_rows)
    assert (X > 0).any(axis=1).all() and (X < 0).any(axis=1).all()
    x = np.array(_slab(name, shape))
    x[1, :, 5] = np.nan
    x[n - 1, :, 20] = 1e308
    res = mcmc_amd.draws_psis_loo(_target(name, d, n_rows), x)                  # returns: MI_OK
    ref = _mirror(name, x, n_rows)
    assert np.isnan(ref["elpd_loo"]).all() and np.isnan(ref["pareto_k"]).all()
    _assert_result(res, ref, "logistic")
    assert res["summary"]["n_bad"] == n_rows and np.isnan(res["summary"]["elpd_loo"])
    only = np.array(_slab(name, shape))
    only[n - 1, :, 20] = 1e308                                                   # the 1e308 column alone: ll of -1e307 or not finite, row by row
    res = mcmc_amd.draws_psis_loo(_target(name, d, n_rows), only)
    ref = _mirror(name, only, n_rows)
    assert not np.array_equal(_bits(ref["elpd_loo"]), _bits(_reference(name, shape, n_rows)["elpd_loo"]))
    _assert_result(res, ref, "logistic, 1e308 alone")
    # NORMAL_MODEL: a column with sigma = 0
    name, shape, n_rows = CASES[4]
    x = np.array(_slab(name, shape))
    x[2, 1, 7] = 0.0
    res = mcmc_amd.draws_psis_loo(_target(name, shape[1], n_rows), x)
    ref = _mirror(name, x, n_rows)
    assert np.isnan(ref["elpd_loo"]).all() and np.isnan(ref["pareto_k"]).all()
    _assert_result(res, ref, "normal, sigma = 0")


def test_an_influential_observation_has_the_largest_k():
    n_rows, shape = 21, (3, 2, 1366)
    rng = np.random.default_rng(21)
    y = 1.5 + 2.0 * rng.standard_normal(n_rows)
    y[13] = y.mean() + 8.0 * y.std(ddof=1)                                       # one observation 8 standard deviations out
    # draws of (mu, sigma) about their posterior given y
    s = y.std(ddof=1)
    x = np.empty(shape)
    x[:, 0, :] = y.mean() + s / np.sqrt(n_rows) * rng.standard_normal((shape[0], shape[2]))
    x[:, 1, :] = s * np.exp(rng.standard_normal((shape[0], shape[2])) / np.sqrt(2.0 * n_rows))
    tgt = mcmc_amd.make_target(mcmc_amd.TARGET_NORMAL_MODEL, 2, y=y)
    res = mcmc_amd.draws_psis_loo(tgt, x)
    ref = psis.psis_ref(waic.loglik(waic.NORMAL_MODEL, x, y, math=ORC_MATH), math=ORC_MATH)
    assert np.isfinite(ref["pareto_k"]).all() and int(np.argmax(ref["pareto_k"])) == 13
    _assert_result(res, ref, "outlier")
    assert int(np.argmax(res["pareto_k"])) == 13
    assert res["summary"]["n_bad"] == np.count_nonzero(~(ref["pareto_k"] <= 0.7))
    assert res["elpd_loo"][13] < res["lppd"][13]                                 # leaving it out costs predictive density
