"""No GPU: mi_mcmc_loglik_waic and mi_mcmc_loglik_psis_loo (WAIC and PSIS-LOO of a caller-supplied pointwise log-likelihood matrix) reject bad arguments
before any device call, in the order include/mi_mcmc.h states; the smallest K of each entry passes the checks as far as the device probe; and the plan of
a call (draws_loglik.hpp: chunks, fold grid, tail, sort groups, tail route, workspace) is the stated function of the shape, of where the matrix lives
and of the two budgets."""

import numpy as np
import pytest

import mcmc_amd
from mcmc_amd import psis

ROWS, SLAB = mcmc_amd.LOGLIK_ROWS, mcmc_amd.LOGLIK_SLAB
_OUT = [np.zeros(65537) for _ in range(4)]               # [n_rows] each (summary: 5), for the largest n_rows a call here can reach a device with


def _matrix(n_rows, K):
    """a matrix every row of which can be fitted, should the call reach a device"""
    rng = np.random.default_rng(n_rows * 1000003 + K)
    return -0.5 * rng.standard_normal((n_rows, K)) ** 2


_MAT = _matrix(5, 25)


def _rc(entry, mat=_MAT.ctypes.data, layout=ROWS, n_rows=5, n_keep=1, n_chains=25, outs=None):
    n_out = 3 if entry == "waic" else 4
    outs = (True,) * n_out if outs is None else outs
    assert len(outs) == n_out
    assert n_rows <= _OUT[0].size or n_rows > 1 << 20     # the outputs hold what a call that runs writes; the larger calls are refused before they write
    ptrs = [a.ctypes.data if on else None for a, on in zip(_OUT, outs)]
    fn = mcmc_amd.lib().mi_mcmc_loglik_waic if entry == "waic" else mcmc_amd.lib().mi_mcmc_loglik_psis_loo
    return fn(mat, layout, mcmc_amd.MEM_HOST, n_rows, n_keep, n_chains, *ptrs, None)


def _none(entry):
    return (False,) * (3 if entry == "waic" else 4)


# each case alone: (keyword arguments, what the message names)
_BAD = {
    "null_matrix": (dict(mat=None), "null matrix"),
    "all_outputs_null": (None, "all NULL"),
    "layout_is_2": (dict(layout=2), "layout = 2"),
    "layout_is_minus_1": (dict(layout=-1), "layout = -1"),
    "n_rows_is_0": (dict(n_rows=0), "n_rows must be positive"),
    "n_keep_past_32_bits": (dict(n_keep=1 << 32), "32 bits"),
    "n_chains_past_32_bits": (dict(n_chains=1 << 32), "32 bits"),
    "n_keep_is_0": (dict(n_keep=0), "K = n_keep * n_chains = 0, at least"),
    "n_chains_is_0": (dict(n_chains=0), "K = n_keep * n_chains = 0, at least"),
    "slab_65537_rows": (dict(layout=SLAB, n_rows=65537), "MI_LOGLIK_SLAB with n_rows = 65537"),
}


@pytest.mark.parametrize("entry", ["waic", "psis"])
@pytest.mark.parametrize("case", sorted(_BAD))
def test_bad_arguments_are_rejected_without_a_gpu(entry, case):
    kw, names = _BAD[case]
    kw = dict(outs=_none(entry)) if kw is None else kw
    assert _rc(entry, **kw) == mcmc_amd.MI_ERR_BAD_ARG
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("loglik_waic:" if entry == "waic" else "loglik_psis_loo:") and names in msg, msg


def test_too_few_and_too_many_samples():
    for entry, kw, names in (("waic", dict(n_keep=1, n_chains=1), "K = n_keep * n_chains = 1, at least 2"),
                             ("psis", dict(n_keep=4, n_chains=6), "K = n_keep * n_chains = 24, at least 25"),
                             ("psis", dict(n_keep=1 << 16, n_chains=1 << 16), "below 2^32")):
        assert _rc(entry, **kw) == mcmc_amd.MI_ERR_BAD_ARG
        msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
        assert names in msg, msg


@pytest.mark.parametrize("entry", ["waic", "psis"])
def test_a_call_that_fails_several_checks_reports_them_in_the_stated_order(entry):
    """every check fails at first; the faults are mended one by one, and each time the next check in the header's order speaks"""
    kw = dict(mat=None, outs=_none(entry), layout=7, n_rows=0, n_keep=1 << 32, n_chains=0)
    steps = [("null matrix", dict(mat=_MAT.ctypes.data)),
             ("all NULL", dict(outs=None)),
             ("layout = 7", dict(layout=SLAB)),
             ("n_rows must be positive", dict(n_rows=65537)),
             ("32 bits", dict(n_keep=1)),
             ("at least", dict(n_keep=1 << 16, n_chains=1 << 16))]           # K = 2^32
    if entry == "psis":
        steps.append(("below 2^32", dict(n_keep=1, n_chains=25)))
    steps.append(("MI_LOGLIK_SLAB with n_rows = 65537", None))
    for names, mend in steps:
        assert _rc(entry, **kw) == mcmc_amd.MI_ERR_BAD_ARG, names
        msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
        assert names in msg, (names, msg)
        if mend:
            kw.update(mend)


def test_the_smallest_K_passes_the_argument_checks_and_there_is_no_cpu_path():
    for name in ("mi_mcmc_loglik_waic", "mi_mcmc_loglik_psis_loo"):
        assert name in mcmc_amd.EXPORTS and hasattr(mcmc_amd.lib(), name)
    assert hasattr(mcmc_amd.lib(), "mi_mcmc_test_loglik_plan")
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.loglik_psis_loo(_matrix(5, 24))
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.loglik_waic(_matrix(5, 1))
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(ValueError):
        mcmc_amd.loglik_waic(_MAT, layout=2)
    if mcmc_amd.lib().mi_mcmc_device_count() == 0:
        two = _matrix(5, 2)
        assert _rc("waic", mat=two.ctypes.data, n_chains=2) == mcmc_amd.MI_ERR_NO_DEVICE       # K = 2: accepted as far as the device check
        assert _rc("psis") == mcmc_amd.MI_ERR_NO_DEVICE                                       # K = 25
        for layout in (ROWS, SLAB):
            for i in range(3):
                assert _rc("waic", layout=layout, outs=tuple(j == i for j in range(3))) == mcmc_amd.MI_ERR_NO_DEVICE
            for i in range(4):
                assert _rc("psis", layout=layout, outs=tuple(j == i for j in range(4))) == mcmc_amd.MI_ERR_NO_DEVICE


def test_the_row_bound_is_the_slab_layouts_alone():
    big = _matrix(65537, 25)
    for entry in ("waic", "psis"):
        assert _rc(entry, mat=big.ctypes.data, layout=SLAB, n_rows=65537) == mcmc_amd.MI_ERR_BAD_ARG
        assert _rc(entry, mat=big.ctypes.data, layout=SLAB, n_rows=65536) != mcmc_amd.MI_ERR_BAD_ARG
        rc = _rc(entry, mat=big.ctypes.data, layout=ROWS, n_rows=65537)
        assert rc == (mcmc_amd.MI_ERR_NO_DEVICE if mcmc_amd.lib().mi_mcmc_device_count() == 0 else mcmc_amd.MI_OK)


def test_what_fits_no_device_is_oom_not_bad_arg():
    # 2^38 + 1 rows; and 2^21 rows of 2^20 columns: 2^41 values.  The size guards come after the device probe
    want = mcmc_amd.MI_ERR_NO_DEVICE if mcmc_amd.lib().mi_mcmc_device_count() == 0 else mcmc_amd.MI_ERR_OOM
    assert _rc("waic", n_rows=(1 << 38) + 1) == want
    assert _rc("psis", n_rows=1 << 21, n_keep=1, n_chains=1 << 20) == want


def _ceil(a, b):
    return (a + b - 1) // b


def _align(b):
    return _ceil(b, 256) * 256


@pytest.mark.parametrize("n_keep,C_,n_chunks", [(1, 2048, 1), (1, 2049, 2), (3, 1366, 3), (1, 25, 1), (2, 60001, 59)])
def test_chunks_fold_grid_and_tail_are_the_stated_functions(n_keep, C_, n_chunks):
    K = n_keep * C_
    for n_rows in (1, 7, 130):
        plans = [mcmc_amd.test_loglik_plan(layout, n_rows, n_keep, C_, mat_host=False, psis=True) for layout in (ROWS, SLAB)]
        assert plans[0] == plans[1]                                            # one matrix, one plan
        p = plans[0]
        assert p["n_chunks"] == n_chunks == _ceil(K, 2048)
        assert p["fold_grid"] == _ceil(n_rows * n_chunks, 4)                  # a wave per (row, chunk), four waves per workgroup
        assert p["M"] == psis.tail_length(K) and p["m"] == psis.fit_points(p["M"])
        assert p["sort_rows"] == n_rows and p["sort_groups"] == 1 and p["tail_route"] == 0
        w = mcmc_amd.test_loglik_plan(ROWS, n_rows, n_keep, C_, mat_host=False, psis=False)
        assert (w["n_chunks"], w["fold_grid"]) == (p["n_chunks"], p["fold_grid"])
        assert (w["M"], w["m"], w["sort_rows"], w["sort_groups"], w["tail_route"]) == (0, 0, 0, 0, 0)
        # the workspace of the WAIC entry: lppd, p_waic [ldR], the partials [n_chunks][4][ldR]; a host matrix is staged whole behind them
        ldR = 128 * _ceil(n_rows, 128)
        assert w["ws_bytes"] == 2 * _align(8 * ldR) + _align(32 * n_chunks * ldR)
        for psis_entry, dev in ((False, w), (True, p)):
            host = mcmc_amd.test_loglik_plan(SLAB, n_rows, n_keep, C_, mat_host=True, psis=psis_entry)
            assert host["ws_bytes"] == dev["ws_bytes"] + _align(8 * n_rows * K)
        assert p["ws_bytes"] > w["ws_bytes"] + 16 * n_rows * K               # the sort's two key images


def test_the_measured_shape():
    p = mcmc_amd.test_loglik_plan(ROWS, 4096, 1, 65536, mat_host=False, psis=True)
    assert (p["n_chunks"], p["fold_grid"], p["M"], p["m"], p["tail_route"]) == (32, 32768, 768, 57, 0)
    assert p["sort_groups"] == _ceil(4096, p["sort_rows"]) and p["ws_bytes"] < (5 << 29)          # the sort's budget of 2 GiB and small change: no block of ll


def test_the_sort_groups_follow_the_rank_budget():
    lib = mcmc_amd.lib()
    n_rows, n_keep, C_ = 300, 2, 50
    try:
        for layout in (ROWS, SLAB):
            shape = (1, n_keep * C_) if layout == ROWS else (n_keep, C_)       # the slab the sorter sees
            b = lib.mi_mcmc_test_rank_dim_bytes(shape[0], shape[1], 0, 0)
            assert b == 16 * 100 + 1024 + 8192
            assert mcmc_amd.test_loglik_plan(layout, n_rows, n_keep, C_)["sort_groups"] == 1
            for budget, rows in ((128 * b, 128), (129 * b - 1, 128), (129 * b, 129), (1, 1), (300 * b, 300)):
                lib.mi_mcmc_test_set_rank_ws_bytes(budget)
                p = mcmc_amd.test_loglik_plan(layout, n_rows, n_keep, C_)
                assert (p["sort_rows"], p["sort_groups"]) == (rows, _ceil(n_rows, rows)), (layout, budget, p)
            lib.mi_mcmc_test_set_rank_ws_bytes(0)
    finally:
        lib.mi_mcmc_test_set_rank_ws_bytes(0)


def test_the_tail_route_on_both_sides_of_the_lds_capacity():
    assert psis.tail_length(7500) == 260
    try:
        for layout in (ROWS, SLAB):
            for cap, route in ((0, 0), (260, 0), (259, 1), (128, 1)):
                mcmc_amd.test_set_psis_lds_tail(cap)
                p = mcmc_amd.test_loglik_plan(layout, 3, 3, 2500)
                assert p["M"] == 260 and p["tail_route"] == route, (cap, p)
        mcmc_amd.test_set_psis_lds_tail(0)
        # ... and of the real one, 8 192 (K0 as in test_draws_psis_host.py)
        K0 = next(K for K in range(7456000, 7458000) if psis.tail_length(K) == 8192 and psis.tail_length(K + 1) == 8193)
        assert mcmc_amd.test_loglik_plan(ROWS, 1, 1, K0)["tail_route"] == 0 and mcmc_amd.test_loglik_plan(ROWS, 1, 1, K0 + 1)["tail_route"] == 1
    finally:
        mcmc_amd.test_set_psis_lds_tail(0)
