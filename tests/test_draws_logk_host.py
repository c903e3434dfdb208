"""No GPU: mi_mcmc_draws_log_kernel rejects bad arguments before any device call (MI_ERR_BAD_ARG / MI_ERR_UNSUPPORTED even where no device is visible -- a
call that reached the device probe would answer MI_ERR_NO_DEVICE there), and the plan of a call (draws_logk.hpp: grid, LDS, padded extents, workspace)
is the stated function of (kind, d, n_rows, n_keep, C) and of what is staged, at the shapes the GPU tests run and at the shapes the timing tool runs."""
import ctypes as C

import numpy as np
import pytest

import mcmc_amd

_X = np.zeros((2, 3, 4))
_OUT = np.zeros((2, 4))
_PREC = np.eye(3)
_ROWS = np.zeros((5, 3))
_Y = np.zeros(5)


def _target(kind=mcmc_amd.TARGET_GAUSS_DENSE, d=3, prec=_PREC, X=None, y=None, n_rows=None, struct_size=None):
    t = mcmc_amd.make_target(kind, d, prec=prec, X=X, y=y)
    if n_rows is not None:
        t.n_rows = n_rows
    if struct_size is not None:
        t.struct_size = struct_size
    return t


def _rc(target, slab=_X.ctypes.data, n_keep=2, n_chains=4, out=_OUT.ctypes.data):
    return mcmc_amd.lib().mi_mcmc_draws_log_kernel(None if target is None else C.byref(target), slab, mcmc_amd.MEM_HOST,
                                                  n_keep, n_chains, out, None)


_LOGIT = dict(kind=mcmc_amd.TARGET_LOGISTIC, prec=None, X=_ROWS, y=_Y)
_NORMAL = dict(kind=mcmc_amd.TARGET_NORMAL_MODEL, d=2, prec=None, y=_Y)
_BAD = {
    "null_target": (None, {}, "target"),
    "null_slab": ({}, dict(slab=None), "slab"),
    "null_out": ({}, dict(out=None), "out"),
    "struct_size": (dict(struct_size=3), {}, "struct_size"),
    "d_is_0": (dict(kind=mcmc_amd.TARGET_GAUSS_ISO, d=0, prec=None), {}, "d "),
    "n_keep_is_0": ({}, dict(n_keep=0), "K "),
    "n_chains_is_0": ({}, dict(n_chains=0), "K "),
    "n_keep_past_32_bits": ({}, dict(n_keep=1 << 32), "n_keep"),
    "n_chains_past_32_bits": ({}, dict(n_chains=1 << 32), "n_chains"),
    "d_past_65536": (dict(kind=mcmc_amd.TARGET_GAUSS_ISO, d=65537, prec=None), {}, "d = 65537"),
    "dense_without_prec": (dict(prec=None), {}, "prec"),
    "diag_without_prec": (dict(kind=mcmc_amd.TARGET_GAUSS_DIAG, prec=None), {}, "prec"),
    "logistic_without_X": (dict(_LOGIT, X=None, n_rows=5), {}, "logistic"),
    "logistic_without_y": (dict(_LOGIT, y=None), {}, "logistic"),
    "logistic_n_rows_is_0": (dict(_LOGIT, n_rows=0), {}, "n_rows"),
    "normal_model_without_y": (dict(_NORMAL, y=None, n_rows=5), {}, "NORMAL_MODEL"),
    "normal_model_n_rows_is_0": (dict(_NORMAL, n_rows=0), {}, "n_rows"),
    "normal_model_d_is_3": (dict(_NORMAL, d=3), {}, "d = 2"),
    "kind_is_0": (dict(kind=0), {}, "kind"),
    "kind_is_7": (dict(kind=7), {}, "kind"),
}


@pytest.mark.parametrize("case", sorted(_BAD))
def test_log_kernel_rejects_bad_arguments_without_a_gpu(case):
    tkw, kw, names = _BAD[case]
    target = None if tkw is None else _target(**tkw)
    assert _rc(target, **kw) == mcmc_amd.MI_ERR_BAD_ARG
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_log_kernel:") and names in msg, msg


def test_the_mixture_target_is_unsupported_without_a_gpu():
    t = _target(kind=mcmc_amd.TARGET_GAUSS_MIXTURE, prec=np.ones(5), X=_ROWS, y=_Y)
    assert _rc(t) == mcmc_amd.MI_ERR_UNSUPPORTED
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_log_kernel:") and "MIXTURE" in msg, msg


def test_front_end_raises_and_the_entry_is_exported():
    assert "mi_mcmc_draws_log_kernel" in mcmc_amd.EXPORTS and hasattr(mcmc_amd.lib(), "mi_mcmc_draws_log_kernel")
    assert hasattr(mcmc_amd.lib(), "mi_mcmc_test_logk_plan")
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_log_kernel(_target(prec=None), _X)
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(ValueError):
        mcmc_amd.draws_log_kernel(_target(), np.zeros((2, 4, 4)))          # the slab's d is not the target's
    with pytest.raises(ValueError):
        mcmc_amd.draws_log_kernel(_target(), 12345, n_keep=2, n_chains=4, mem=mcmc_amd.MEM_DEVICE)      # a device slab without a device out
    if mcmc_amd.lib().mi_mcmc_device_count() == 0:
        with pytest.raises(mcmc_amd.MiMcmcError) as e:                     # a valid call: no CPU path
            mcmc_amd.draws_log_kernel(_target(), _X)
        assert e.value.code == mcmc_amd.MI_ERR_NO_DEVICE


def _ceil(a, b):
    return (a + b - 1) // b


def _a256(n):
    return _ceil(n, 256) * 256


def _want_plan(kind, d, n_rows, n_keep, C_, slab_host, target_host):
    """draws_logk.hpp's statement, restated"""
    K = n_keep * C_
    product = kind in (mcmc_amd.TARGET_GAUSS_DENSE, mcmc_amd.TARGET_LOGISTIC)
    mat = {mcmc_amd.TARGET_GAUSS_ISO: 0, mcmc_amd.TARGET_GAUSS_DIAG: d, mcmc_amd.TARGET_GAUSS_DENSE: d * d, mcmc_amd.TARGET_LOGISTIC: n_rows * d,
           mcmc_amd.TARGET_NORMAL_MODEL: 0}[kind]
    yv = n_rows if kind in (mcmc_amd.TARGET_LOGISTIC, mcmc_amd.TARGET_NORMAL_MODEL) else 0
    w = dict(route=int(product), block=256)
    if product:
        rows = d if kind == mcmc_amd.TARGET_GAUSS_DENSE else n_rows
        w.update(grid=_ceil(K, 128), lds_bytes=2 * 32 * 144 * 8, Kp=16 * _ceil(d, 16), ldA=128 * _ceil(rows, 128), n_row_tiles=_ceil(rows, 128))
        pack = w["Kp"] * w["ldA"] * 8
    else:
        w.update(grid=_ceil(K, 256), lds_bytes=0, Kp=0, ldA=0, n_row_tiles=0)
        pack = 0
    ws = _a256(pack)
    if target_host:
        ws += _a256(mat * 8) + _a256(yv * 8)
    if slab_host:
        ws += _a256(K * d * 8) + _a256(K * 8)
    w["ws_bytes"] = max(ws, 256)
    return w


D, L = mcmc_amd.TARGET_GAUSS_DENSE, mcmc_amd.TARGET_LOGISTIC
# (kind, d, n_rows, n_keep, C): the GPU tests' shapes, then the timing tool's
PLAN_SHAPES = [(D, 1, 0, 1, 3), (D, 5, 0, 2, 7), (D, 17, 0, 3, 37), (D, 130, 0, 2, 333), (D, 520, 0, 1, 19), (D, 32, 0, 2, 7),
               (L, 3, 5, 2, 5), (L, 70, 130, 3, 37), (L, 520, 70, 1, 19), (L, 32, 16, 2, 5),
               (mcmc_amd.TARGET_GAUSS_ISO, 300, 0, 3, 37), (mcmc_amd.TARGET_GAUSS_DIAG, 300, 0, 3, 37), (mcmc_amd.TARGET_NORMAL_MODEL, 2, 50, 4, 37),
               (D, 128, 0, 100, 65536), (D, 1024, 0, 1, 65536), (L, 512, 1024, 1, 32768)]


@pytest.mark.parametrize("staged", [(True, True), (False, False), (False, True)], ids=["host", "device", "device_slab_host_target"])
@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_the_plan_is_the_stated_function_of_the_shape(shape, staged):
    got = mcmc_amd.test_logk_plan(*shape, slab_host=staged[0], target_host=staged[1])
    assert got == _want_plan(*shape, *staged)
    assert got == mcmc_amd.test_logk_plan(*shape, slab_host=staged[0], target_host=staged[1])        # nothing else enters


def test_the_product_grid_covers_every_column_once_and_fits_the_device_limits():
    for shape in PLAN_SHAPES:
        p = mcmc_amd.test_logk_plan(*shape)
        K = shape[3] * shape[4]
        per_wg = 128 if p["route"] else 256
        assert (p["grid"] - 1) * per_wg < K <= p["grid"] * per_wg
        assert p["grid"] < 2 ** 31 and p["lds_bytes"] <= 80 * 1024      # two workgroups of the product kernel share a CU's 160 KiB
