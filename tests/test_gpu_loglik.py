"""GPU: mi_mcmc_loglik_waic and mi_mcmc_loglik_psis_loo -- WAIC and PSIS-LOO of a pointwise log-likelihood matrix that the caller supplies
(mcmc_amd/csrc/draws_loglik.hip in front of draws_rank.hip and draws_psis.hip) against the existing numpy mirrors of include/mi_mcmc.h, mcmc_amd/waic.py
(row_stats, summary) and mcmc_amd/psis.py (psis_ref), run over the CPU oracle's arithmetic as in test_gpu_draws_psis.py.  BIT FOR BIT: outputs are compared
as uint64 and any NaN matches any NaN; there is no tolerance in this file.  The matrices do not come from a target; for MI_LOGLIK_SLAB the device gets
np.transpose(mat, (1, 0, 2)) of the matrix [n_rows, n_keep, C] the mirror sees.

Which shape (n_rows, n_keep, C) reaches what (K = n_keep C samples, M the tail), each in both layouts:
  (5, 1, 25)       the smallest K; M = 5; one ragged chunk with 25 of the 64 slots used
  (7, 1, 2048)     exactly one full chunk
  (7, 1, 2049)     a second chunk of one column, whose shift is its only value
  (9, 3, 1366)     K = 4098: three chunks, the sqrt branch (M = 193), C odd; in the SLAB layout the chunks straddle t
  (3, 3, 2500)     M = 260, a tail longer than the 256 slots; under the hook the re-read tail route, with the same bits as the LDS route
  (3, 2, 60001)    K = 120 002: M = 1040; eight body pieces, the last one ragged
  (130, 2, 100)    the K div 5 branch; a ragged second block of 128 padded rows; C < 512, the sorter's flattened walk"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import psis, synth, waic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ORC_MATH = dict(dot=lambda a, b: orc.dot(a, b, 1), exp=lambda x: orc.math_eval(0, x)[0], log=lambda x: orc.math_eval(1, x)[0],
                softplus=lambda x: orc.math_eval(3, x)[0])
ROWS, SLAB = mcmc_amd.LOGLIK_ROWS, mcmc_amd.LOGLIK_SLAB
LAYOUTS = [ROWS, SLAB]
_LNAME = {ROWS: "rows", SLAB: "slab"}
SHAPES = [(5, 1, 25), (7, 1, 2048), (7, 1, 2049), (9, 3, 1366), (3, 3, 2500), (3, 2, 60001), (130, 2, 100)]
_IDS = ["x".join(map(str, s)) for s in SHAPES]
_WAIC_SUMMARY = ("elpd_waic", "p_waic", "lppd", "se_elpd")
_PSIS_SUMMARY = ("elpd_loo", "p_loo", "lppd", "se_elpd_loo", "n_bad")


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
def _matrix(shape):
    """ll [n_rows, n_keep, C], read-only: every row has a spread and a scale of its own"""
    R, n_keep, C_ = shape
    K = n_keep * C_
    rng = np.random.default_rng(R * 1000003 + K)
    a = rng.standard_normal((R, 1))
    s = 0.5 + rng.random((R, 1))
    z = rng.standard_normal((R, K))
    ll = -0.5 * ((a + z) / s) ** 2 - np.log(s)
    return _frozen(np.ascontiguousarray(ll.reshape(R, n_keep, C_)))[0]


def _laid_out(mat, layout):
    """what the device is handed: the matrix itself, or the slab [n_keep, n_rows, C]"""
    return mat if layout == ROWS else np.ascontiguousarray(np.transpose(mat, (1, 0, 2)))


def _mirror(mat):
    """the yardstick: dict of lppd, p_waic, waic_summary, elpd_loo, pareto_k, psis_summary of ll [n_rows, n_keep, C]"""
    lppd, p_waic = waic.row_stats(mat, math=ORC_MATH)
    ref = dict(lppd=lppd, p_waic=p_waic, waic_summary=waic.summary(lppd, p_waic))
    if mat.shape[1] * mat.shape[2] >= psis.K_MIN:
        p = psis.psis_ref(mat, math=ORC_MATH)
        _assert_same(p["lppd"], lppd, "the two mirrors' lppd")
        ref.update(elpd_loo=p["elpd_loo"], pareto_k=p["pareto_k"], psis_summary=p["summary"])
    return ref


@functools.lru_cache(maxsize=None)
def _reference(shape):
    ref = _mirror(_matrix(shape))
    _frozen(*ref.values())
    return ref


def _assert_waic(res, ref, what):
    for k in ("lppd", "p_waic"):
        if res[k] is not None:
            _assert_same(res[k], ref[k], (what, "waic", k))
    if res["summary"] is not None:
        _assert_same([res["summary"][k] for k in _WAIC_SUMMARY], ref["waic_summary"], (what, "waic summary"))


def _assert_psis(res, ref, what):
    for k in ("elpd_loo", "pareto_k", "lppd"):
        if res[k] is not None:
            _assert_same(res[k], ref[k], (what, "psis", k))
    if res["summary"] is not None:
        _assert_same([res["summary"][k] for k in _PSIS_SUMMARY], ref["psis_summary"], (what, "psis summary"))


def _both(mat, layout, ref, what):
    x = _laid_out(mat, layout)
    _assert_waic(mcmc_amd.loglik_waic(x, layout), ref, what)
    _assert_psis(mcmc_amd.loglik_psis_loo(x, layout), ref, what)


@pytest.mark.parametrize("layout", LAYOUTS, ids=_LNAME.get)
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_every_output_is_the_mirror_bit_for_bit(shape, layout):
    ref = _reference(shape)
    assert np.isfinite(ref["pareto_k"]).all() and np.isfinite(ref["elpd_loo"]).all()        # the fitted path is what is compared
    R, n_keep, C_ = shape
    K = n_keep * C_
    plan = mcmc_amd.test_loglik_plan(layout, R, n_keep, C_)
    assert plan["M"] == psis.tail_length(K) and plan["n_chunks"] == -(-K // 2048) and plan["sort_groups"] == 1 and plan["tail_route"] == 0
    mat = _matrix(shape)
    x = _laid_out(mat, layout)
    w = mcmc_amd.loglik_waic(x, layout)
    _assert_waic(w, ref, (shape, _LNAME[layout]))
    p = mcmc_amd.loglik_psis_loo(x, layout)
    _assert_psis(p, ref, (shape, _LNAME[layout]))
    _assert_same(p["lppd"], w["lppd"], "lppd of the two entries")
    assert p["summary"]["n_bad"] == np.count_nonzero(~(ref["pareto_k"] <= 0.7))


@pytest.mark.parametrize("layout", LAYOUTS, ids=_LNAME.get)
def test_the_tail_re_read_from_the_sorted_row_gives_the_bits_of_the_tail_in_lds(layout):
    shape = SHAPES[4]
    ref = _reference(shape)
    try:
        mcmc_amd.test_set_psis_lds_tail(128)
        plan = mcmc_amd.test_loglik_plan(layout, *shape)
        assert plan["M"] == 260 and plan["tail_route"] == 1
        res = mcmc_amd.loglik_psis_loo(_laid_out(_matrix(shape), layout), layout)
    finally:
        mcmc_amd.test_set_psis_lds_tail(0)
    assert mcmc_amd.test_loglik_plan(layout, *shape)["tail_route"] == 0
    _assert_psis(res, ref, "the tail in device memory")


@pytest.mark.parametrize("layout", LAYOUTS, ids=_LNAME.get)
def test_several_sort_groups_give_the_bits_of_one(layout):
    shape = (300, 2, 50)
    ref = _reference(shape)
    mat = _matrix(shape)
    lib = mcmc_amd.lib()
    assert mcmc_amd.test_loglik_plan(layout, *shape)["sort_groups"] == 1
    _both(mat, layout, ref, "one group")
    b = lib.mi_mcmc_test_rank_dim_bytes(1, 100, 0, 0)
    try:
        lib.mi_mcmc_test_set_rank_ws_bytes(128 * b + 17)
        plan = mcmc_amd.test_loglik_plan(layout, *shape)
        assert (plan["sort_rows"], plan["sort_groups"]) == (128, 3)                           # 128 + 128 + 44
        res = mcmc_amd.loglik_psis_loo(_laid_out(mat, layout), layout)
    finally:
        lib.mi_mcmc_test_set_rank_ws_bytes(0)
    _assert_psis(res, ref, "128 + 128 + 44")


def test_the_matrix_of_draws_waic_reproduces_the_two_built_in_entries():
    """loglik_out of mi_mcmc_draws_waic on a LOGISTIC slab stays on the device and is fed to the two new entries"""
    import torch
    n, d, C_, n_rows = 2, 70, 100, 130
    X, y = synth.logistic_problem(d, n_rows)
    tgt = mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, d, X=X, y=y)
    slab = torch.from_numpy(np.random.default_rng(n * 1000003 + d * 1009 + C_).standard_normal((n, d, C_))).cuda()
    st = torch.cuda.current_stream().cuda_stream
    new = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    ll, lppd, pw = new(n_rows, n, C_), new(n_rows), new(n_rows)
    w0 = mcmc_amd.draws_waic(tgt, slab, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, lppd=lppd, p_waic=pw, loglik=ll)
    elpd, pk, lppd2 = new(n_rows), new(n_rows), new(n_rows)
    p0 = mcmc_amd.draws_psis_loo(tgt, slab, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, elpd_loo=elpd, pareto_k=pk, lppd=lppd2)
    torch.cuda.synchronize()
    ref = dict(lppd=lppd.cpu().numpy(), p_waic=pw.cpu().numpy(), waic_summary=np.array([w0["summary"][k] for k in _WAIC_SUMMARY]),
               elpd_loo=elpd.cpu().numpy(), pareto_k=pk.cpu().numpy(), psis_summary=np.array([p0["summary"][k] for k in _PSIS_SUMMARY]))
    assert np.isfinite(ref["pareto_k"]).all() and np.isfinite(ref["p_waic"]).all()
    _assert_same(lppd2.cpu().numpy(), ref["lppd"], "the built-in entries' lppd")
    ll_before = ll.cpu().numpy()
    a, b = new(n_rows), new(n_rows)
    w = mcmc_amd.loglik_waic(ll, ROWS, n_rows=n_rows, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, lppd=a, p_waic=b)
    torch.cuda.synchronize()
    _assert_waic(dict(lppd=a.cpu().numpy(), p_waic=b.cpu().numpy(), summary=w["summary"]), ref, "draws_waic's matrix")
    e, k, l = new(n_rows), new(n_rows), new(n_rows)
    p = mcmc_amd.loglik_psis_loo(ll, ROWS, n_rows=n_rows, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, elpd_loo=e, pareto_k=k, lppd=l)
    _assert_psis(dict(elpd_loo=e.cpu().numpy(), pareto_k=k.cpu().numpy(), lppd=l.cpu().numpy(), summary=p["summary"]), ref, "draws_waic's matrix")
    assert np.array_equal(_bits(ll.cpu().numpy()), _bits(ll_before))                           # the matrix is read only


@pytest.fixture(scope="module")
def user_lib(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("ul") / "libuser_loglik.so")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-Wall", "-Werror", "-Wno-unused-function",
                           f"-I{ROOT}/include", "-shared", f"{ROOT}/examples/user_loglik.hip", f"-L{ROOT}/mcmc_amd", "-lmi_mcmc", f"-Wl,-rpath,{ROOT}/mcmc_amd",
                           "-o", out])
    mcmc_amd.lib()                                       # the engine first: the example resolves against the copy that is loaded
    return C.CDLL(out)


def test_the_example_librarys_matrix_reproduces_the_built_in_normal_model(user_lib):
    import torch
    n, C_, n_rows = 4, 37, 50
    rng = np.random.default_rng(n * 1000003 + 2 * 1009 + C_)
    x = rng.standard_normal((n, 2, C_))
    x[:, 1, :] = np.abs(x[:, 1, :]) + 0.5
    y = 1.5 + 2.0 * np.random.default_rng(n_rows).standard_normal(n_rows)
    tgt = mcmc_amd.make_target(mcmc_amd.TARGET_NORMAL_MODEL, 2, y=y)
    w0 = mcmc_amd.draws_waic(tgt, x, want_loglik=True)
    p0 = mcmc_amd.draws_psis_loo(tgt, x)
    ref = dict(lppd=w0["lppd"], p_waic=w0["p_waic"], waic_summary=np.array([w0["summary"][k] for k in _WAIC_SUMMARY]),
               elpd_loo=p0["elpd_loo"], pareto_k=p0["pareto_k"], psis_summary=np.array([p0["summary"][k] for k in _PSIS_SUMMARY]))
    assert np.isfinite(ref["pareto_k"]).all()
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    ll = torch.full((n, n_rows, C_), -7.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    u64 = C.c_uint64
    assert user_lib.user_loglik_normal(C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), u64(n), u64(C_), u64(n_rows), C.c_void_p(ll.data_ptr()), C.c_void_p(st)) == 0
    torch.cuda.synchronize()
    _assert_same(np.transpose(ll.cpu().numpy(), (1, 0, 2)), w0["loglik"], "the example's matrix against draws_waic's")        # a second producer of the same bits
    new = lambda: torch.full((n_rows,), -7.0, dtype=torch.float64, device="cuda")
    a, b = new(), new()
    w = mcmc_amd.loglik_waic(ll, SLAB, n_rows=n_rows, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, lppd=a, p_waic=b)
    torch.cuda.synchronize()
    _assert_waic(dict(lppd=a.cpu().numpy(), p_waic=b.cpu().numpy(), summary=w["summary"]), ref, "the example's matrix")
    e, k, l = new(), new(), new()
    p = mcmc_amd.loglik_psis_loo(ll, SLAB, n_rows=n_rows, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, elpd_loo=e, pareto_k=k, lppd=l)
    _assert_psis(dict(elpd_loo=e.cpu().numpy(), pareto_k=k.cpu().numpy(), lppd=l.cpu().numpy(), summary=p["summary"]), ref, "the example's matrix")
    # ... and the example's own end-to-end function
    ws, ls, kd = np.zeros(4), np.zeros(5), new()
    rc = user_lib.user_loglik_normal_compare(C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), u64(n), u64(C_), u64(n_rows), C.c_void_p(ws.ctypes.data),
                                             C.c_void_p(ls.ctypes.data), C.c_void_p(kd.data_ptr()), C.c_void_p(st))
    assert rc == 0, mcmc_amd.lib().mi_mcmc_last_error().decode()
    _assert_same(ws, ref["waic_summary"], "end to end, WAIC")
    _assert_same(ls, ref["psis_summary"], "end to end, LOO")
    _assert_same(kd.cpu().numpy(), ref["pareto_k"], "end to end, pareto_k")


@pytest.mark.parametrize("layout", LAYOUTS, ids=_LNAME.get)
def test_every_call_variant_gives_the_same_bits(layout):
    import torch
    shape = SHAPES[6]
    R, n_keep, C_ = shape
    ref = _reference(shape)
    x = _laid_out(_matrix(shape), layout)
    # a host matrix, each output alone
    for k in ("lppd", "p_waic", "summary"):
        res = mcmc_amd.loglik_waic(x, layout, want_lppd=k == "lppd", want_p_waic=k == "p_waic", want_summary=k == "summary")
        assert [j for j in res if res[j] is not None] == [k]
        _assert_waic(res, ref, ("host matrix, only", k))
    for k in ("elpd_loo", "pareto_k", "lppd", "summary"):
        res = mcmc_amd.loglik_psis_loo(x, layout, want_elpd_loo=k == "elpd_loo", want_pareto_k=k == "pareto_k", want_lppd=k == "lppd", want_summary=k == "summary")
        assert [j for j in res if res[j] is not None] == [k]
        _assert_psis(res, ref, ("host matrix, only", k))
    # a device matrix, every output NULL in turn
    dev = torch.from_numpy(np.array(x)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    kw = dict(n_rows=R, n_keep=n_keep, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st)
    new = lambda: torch.full((R,), -7.0, dtype=torch.float64, device="cuda")
    for skip in (None, "lppd", "p_waic", "summary"):
        outs = {k: (None if k == skip else new()) for k in ("lppd", "p_waic")}
        res = mcmc_amd.loglik_waic(dev, layout, want_summary=skip != "summary", **outs, **kw)
        torch.cuda.synchronize()                                                 # summary == NULL on a device matrix: the call returned after enqueueing
        got = {k: (None if v is None else v.cpu().numpy()) for k, v in outs.items()}
        got["summary"] = res["summary"]
        assert (got["summary"] is None) == (skip == "summary")
        _assert_waic(got, ref, ("device matrix without", skip))
    for skip in (None, "elpd_loo", "pareto_k", "lppd", "summary"):
        outs = {k: (None if k == skip else new()) for k in ("elpd_loo", "pareto_k", "lppd")}
        res = mcmc_amd.loglik_psis_loo(dev, layout, want_summary=skip != "summary", **outs, **kw)
        got = {k: (None if v is None else v.cpu().numpy()) for k, v in outs.items()}
        got["summary"] = res["summary"]
        _assert_psis(got, ref, ("device matrix without", skip))
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(x))                   # the matrix is read only


def test_the_result_does_not_depend_on_the_stream_or_the_cached_workspace():
    import torch
    shape, layout = SHAPES[3], SLAB
    R, n_keep, C_ = shape
    ref = _reference(shape)
    dev = torch.from_numpy(_laid_out(_matrix(shape), layout)).cuda()

    def run(stream):
        kw = dict(n_rows=R, n_keep=n_keep, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=stream.cuda_stream)
        wo = {k: torch.zeros(R, dtype=torch.float64, device="cuda") for k in ("lppd", "p_waic")}
        mcmc_amd.loglik_waic(dev, layout, want_summary=False, **wo, **kw)       # not waited for: the next call is on the same stream
        po = {k: torch.zeros(R, dtype=torch.float64, device="cuda") for k in ("elpd_loo", "pareto_k", "lppd")}
        res = mcmc_amd.loglik_psis_loo(dev, layout, **po, **kw)
        stream.synchronize()
        w = {k: v.cpu().numpy() for k, v in wo.items()}
        w["summary"] = None
        p = {k: v.cpu().numpy() for k, v in po.items()}
        p["summary"] = res["summary"]
        return w, p

    torch.cuda.synchronize()
    a = run(torch.cuda.Stream())
    b = run(torch.cuda.Stream())
    mcmc_amd.release_workspace()
    c = run(torch.cuda.current_stream())
    for (w, p), what in ((a, "stream 1"), (b, "stream 2"), (c, "after release_workspace")):
        _assert_waic(w, ref, what)
        _assert_psis(p, ref, what)


@pytest.mark.parametrize("layout", LAYOUTS, ids=_LNAME.get)
def test_a_constant_row_and_non_finite_rows_leave_the_other_rows_alone(layout):
    shape = (6, 2, 100)
    clean = _matrix(shape)
    ref_clean = _reference(shape)
    const = -1.5                                         # c + log(K) is exact (c is a multiple of log(K)'s last place), so the row's elpd is c itself
    bad = np.array(clean)
    bad[1] = const
    bad[2, 1, 7] = np.nan
    bad[3, 0, 0] = -np.inf                               # the first chunk's shift
    bad[3, 1, 50] = -np.inf
    bad[4, 0, 99] = 1e308
    ref = _mirror(bad)
    # what the mirror says by the IEEE rules
    assert ref["p_waic"][1] == 0.0 and ref["pareto_k"][1] == np.inf and ref["elpd_loo"][1] == const
    assert np.isnan(ref["elpd_loo"][2]) and np.isnan(ref["pareto_k"][2]) and np.isnan(ref["lppd"][2]) and np.isnan(ref["p_waic"][2])
    assert np.isnan(ref["elpd_loo"][3]) and np.isnan(ref["pareto_k"][3]) and np.isnan(ref["p_waic"][3])
    assert ref["lppd"][4] == np.inf
    for r in (0, 5):
        for k in ("lppd", "p_waic", "elpd_loo", "pareto_k"):
            assert _bits(ref[k])[r] == _bits(ref_clean[k])[r]
    x = _laid_out(bad, layout)
    w = mcmc_amd.loglik_waic(x, layout)                  # returns: MI_OK
    p = mcmc_amd.loglik_psis_loo(x, layout)
    _assert_waic(w, ref, "bad rows")
    _assert_psis(p, ref, "bad rows")
    assert p["summary"]["n_bad"] == np.count_nonzero(~(ref["pareto_k"] <= 0.7)) >= 3
    for r in (0, 5):                                     # the other rows' bits are those of a run without the bad rows
        for res, keys in ((w, ("lppd", "p_waic")), (p, ("elpd_loo", "pareto_k", "lppd"))):
            for k in keys:
                assert _bits(res[k])[r] == _bits(ref_clean[k])[r], (r, k)


@pytest.mark.parametrize("layout", LAYOUTS, ids=_LNAME.get)
def test_one_row_has_no_standard_error(layout):
    shape = (1, 2, 100)
    ref = _reference(shape)
    assert np.isnan(ref["waic_summary"][3]) and np.isnan(ref["psis_summary"][3]) and np.isfinite(ref["pareto_k"]).all()
    x = _laid_out(_matrix(shape), layout)
    w = mcmc_amd.loglik_waic(x, layout)
    p = mcmc_amd.loglik_psis_loo(x, layout)
    _assert_waic(w, ref, "one row")
    _assert_psis(p, ref, "one row")
    assert np.isnan(w["summary"]["se_elpd"]) and np.isnan(p["summary"]["se_elpd_loo"])
