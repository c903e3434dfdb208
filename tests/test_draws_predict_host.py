"""No GPU: mi_mcmc_draws_predict rejects bad arguments before any device call (MI_ERR_BAD_ARG / MI_ERR_UNSUPPORTED even where no device is visible -- a
call that reached the device probe would answer MI_ERR_NO_DEVICE there), and mcmc_amd/predict.py, the numpy statement of the arithmetic, agrees with
plain numpy on a small problem, with the CPU oracle's generator, and with the truth: the replicates of a row are Bernoulli draws of its p.

The bounds.  p against 1 / (1 + exp(-X theta)): 1e-15 relative, as the issue sets it.  row_stats' mean and variance against np.mean / np.var(ddof=1):
1e-13 relative, as the issue sets it.  The replicate's frequency: |rep_freq_r - p_mean_r| <= 5 sqrt(sum_k p_rk (1 - p_rk)) / K, five standard deviations
of the sum of K independent Bernoulli(p_rk) draws -- the sum's own 5 sigma, not a chosen number."""
import ctypes as C

import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import predict, synth

_X = np.zeros((2, 3, 4))
_ROWS = np.zeros((5, 3))
_Y = np.zeros(5)
_NAMES = ("p_mean", "p_var", "rep_freq", "prob", "yrep", "t_rep", "ll_rep", "ll_obs", "summary")
_OUT = dict(p_mean=np.zeros(5), p_var=np.zeros(5), rep_freq=np.zeros(5), prob=np.zeros((5, 2, 4)), yrep=np.zeros((5, 2, 4)), t_rep=np.zeros((2, 4)),
            ll_rep=np.zeros((2, 4)), ll_obs=np.zeros((2, 4)), summary=np.zeros(4))
_ALL = frozenset(_NAMES)


def _target(kind=mcmc_amd.TARGET_LOGISTIC, d=3, prec=None, X=_ROWS, y=_Y, n_rows=None, struct_size=None):
    t = mcmc_amd.make_target(kind, d, prec=prec, X=X, y=y)
    if n_rows is not None:
        t.n_rows = n_rows
    if struct_size is not None:
        t.struct_size = struct_size
    return t


def _rc(target, slab=_X.ctypes.data, n_keep=2, n_chains=4, outs=_ALL):
    ptrs = [_OUT[k].ctypes.data if k in outs else None for k in _NAMES]
    return mcmc_amd.lib().mi_mcmc_draws_predict(None if target is None else C.byref(target), slab, mcmc_amd.MEM_HOST,
                                               n_keep, n_chains, 7, *[p for p in ptrs], None)


_BAD = {
    "null_target": (None, {}, "target"),
    "null_slab": ({}, dict(slab=None), "slab"),
    "all_outputs_null": ({}, dict(outs=frozenset()), "all nine outputs are NULL"),
    "struct_size": (dict(struct_size=3), {}, "struct_size"),
    "d_is_0": (dict(d=0), {}, "d "),
    "n_keep_is_0": ({}, dict(n_keep=0), "K "),
    "K_is_1": ({}, dict(n_keep=1, n_chains=1), "K = n_keep * n_chains = 1"),
    "n_keep_past_32_bits": ({}, dict(n_keep=1 << 32), "n_keep"),
    "n_chains_past_32_bits": ({}, dict(n_chains=1 << 32), "n_chains"),
    "d_past_65536": (dict(d=65537), {}, "d = 65537"),
    "logistic_without_X": (dict(X=None, n_rows=5), {}, "logistic"),
    "n_rows_is_0": (dict(n_rows=0), {}, "n_rows"),
    "n_rows_is_2_to_32": (dict(n_rows=1 << 32), {}, "n_rows = 4294967296"),
    "no_y_with_ll_obs": (dict(y=None), dict(outs=frozenset(["p_mean", "ll_obs"])), "target.y"),
    "no_y_with_summary": (dict(y=None), dict(outs=frozenset(["t_rep", "summary"])), "target.y"),
    "kind_is_0": (dict(kind=0), {}, "kind"),
    "kind_is_7": (dict(kind=7), {}, "kind"),
}


@pytest.mark.parametrize("case", sorted(_BAD))
def test_predict_rejects_bad_arguments_without_a_gpu(case):
    tkw, kw, names = _BAD[case]
    target = None if tkw is None else _target(**tkw)
    assert _rc(target, **kw) == mcmc_amd.MI_ERR_BAD_ARG
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_predict:") and names in msg, msg


@pytest.mark.parametrize("kind,kw,says", [(mcmc_amd.TARGET_GAUSS_ISO, {}, "no observations"), (mcmc_amd.TARGET_GAUSS_DIAG, dict(prec=np.ones(3)), "no observations"),
                                          (mcmc_amd.TARGET_GAUSS_DENSE, dict(prec=np.eye(3)), "no observations"),
                                          (mcmc_amd.TARGET_GAUSS_MIXTURE, dict(prec=np.ones(5)), "no observations"),
                                          (mcmc_amd.TARGET_NORMAL_MODEL, dict(d=2, X=None), "NORMAL_MODEL")], ids=["iso", "diag", "dense", "mixture", "normal_model"])
def test_the_other_targets_are_unsupported_without_a_gpu(kind, kw, says):
    assert _rc(_target(kind=kind, **kw)) == mcmc_amd.MI_ERR_UNSUPPORTED
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draws_predict:") and says in msg, msg


def test_the_entry_is_exported_and_the_version_stands():
    assert "mi_mcmc_draws_predict" in mcmc_amd.EXPORTS and hasattr(mcmc_amd.lib(), "mi_mcmc_draws_predict")
    assert mcmc_amd.lib().mi_mcmc_version() == 0x000600
    t = mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, 3, X=_ROWS)             # no outcomes: a target to predict at
    assert int(t.n_rows) == 5 and not t.y
    with pytest.raises(ValueError):
        mcmc_amd.draws_predict(_target(), np.zeros((2, 4, 4)))                 # the slab's d is not the target's
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_predict(t, _X, want_summary=True)
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    if mcmc_amd.lib().mi_mcmc_device_count() == 0:
        for k in _NAMES:                                                       # valid calls, each output alone: no CPU path
            assert _rc(_target(), outs=frozenset([k])) == mcmc_amd.MI_ERR_NO_DEVICE
        assert _rc(_target(y=None), outs=_ALL - {"ll_obs", "summary"}) == mcmc_amd.MI_ERR_NO_DEVICE


def _small():
    X, y = synth.logistic_problem(4, 30)
    slab = 0.7 * np.random.default_rng(11).standard_normal((5, 4, 90))         # K = 450
    return X, y, slab


def test_the_mirror_over_numpy_is_the_plain_formula():
    X, y, slab = _small()
    ref = predict.predict_ref(slab, X, y, seed=3)
    cols = slab.transpose(0, 2, 1).reshape(-1, 4)
    want = 1.0 / (1.0 + np.exp(-(X @ cols.T)))
    p = ref["prob"].reshape(30, -1)
    assert np.max(np.abs(p - want) / want) <= 1e-15
    assert np.max(np.abs(ref["p_mean"] - np.mean(p, axis=1)) / np.mean(p, axis=1)) <= 1e-13
    assert np.max(np.abs(ref["p_var"] - np.var(p, axis=1, ddof=1)) / np.var(p, axis=1, ddof=1)) <= 1e-13
    yr = ref["yrep"].reshape(30, -1)
    assert set(np.unique(yr)) <= {0.0, 1.0} and 0.0 < yr.mean() < 1.0
    assert np.array_equal(ref["t_rep"].ravel(), yr.sum(axis=0))
    assert np.array_equal(ref["rep_freq"], yr.sum(axis=1) / 450.0)            # (A / K) * K need not round back to A: the quotient itself is compared
    eta = X @ cols.T
    assert np.allclose(ref["ll_obs"].ravel(), (y[:, None] * eta - np.logaddexp(0.0, eta)).sum(axis=0), rtol=1e-13, atol=0.0)
    assert np.allclose(ref["ll_rep"].ravel(), (yr * eta - np.logaddexp(0.0, eta)).sum(axis=0), rtol=1e-13, atol=0.0)
    t_obs, ppp_t, ppp_dev, t_mean = ref["summary"]
    assert t_obs == y.sum() and ppp_t == np.mean(ref["t_rep"] >= t_obs) and ppp_dev == np.mean(ref["ll_rep"] <= ref["ll_obs"]) and t_mean == yr.sum() / 450.0
    # without outcomes: the same replicates and statistics, no ll_obs, no summary
    bare = predict.predict_ref(slab, X, None, seed=3)
    assert bare["ll_obs"] is None and bare["summary"] is None
    for k in ("prob", "yrep", "p_mean", "p_var", "rep_freq", "t_rep", "ll_rep"):
        assert np.array_equal(bare[k], ref[k]), k
    assert not np.array_equal(predict.predict_ref(slab, X, y, seed=4)["yrep"], ref["yrep"])


def test_a_nan_probability_replicates_a_zero_and_counts_as_false():
    assert np.array_equal(predict.yrep(np.array([np.nan, 0.0, 1.0, 0.5]), np.array([0.3, 0.3, 0.3, 0.5])), [0.0, 0.0, 1.0, 0.0])
    s = predict.summary(np.array([1.0, 0.0]), np.array([1.0, 2.0, 0.0]), np.array([np.nan, -1.0, -3.0]), np.array([-2.0, np.nan, -2.0]))
    assert np.array_equal(s, [1.0, 2.0 / 3.0, 1.0 / 3.0, 1.0])


def test_the_counter_layout_and_u01_are_the_oracles():
    """uniforms() with stream 1 (STREAM_UNIFORM) in place of 8, over the oracle's Philox block, is the oracle's own uniform(seed, chain, draw 0, slot):
    the counter layout and u01 written out in predict.py are det_math.hpp's.  A seed and a chain beyond 32 bits reach the key's and the counter's high words."""
    math = dict(predict.NUMPY_MATH, philox=lambda ctr, key: np.array([orc.philox(c, key) for c in ctr]))
    for seed in (0, 12345, (7 << 32) | 9):
        u = predict.uniforms(seed, 6, 9, math, stream=1)
        for r in range(6):
            for k in range(9):
                assert u[r, k].view(np.uint64) == np.float64(orc.uniform(seed, k, 0, r)).view(np.uint64), (seed, r, k)
        assert np.array_equal(u, predict.uniforms(seed, 6, 9, predict.NUMPY_MATH, stream=1))             # and numpy's Philox is the oracle's
    assert not np.array_equal(predict.uniforms(5, 6, 9), predict.uniforms(5, 6, 9, stream=1))            # stream 8 is another stream
    # a chain beyond 32 bits: its high bits go to the fourth counter word, above the stream
    ctr_seen = []
    predict.uniforms(1, 1, 1, dict(predict.NUMPY_MATH, philox=lambda ctr, key: (ctr_seen.append(np.array(ctr)), predict._philox_np(ctr, key))[1]))
    assert ctr_seen[0].tolist() == [[0, 0, 0, 8]]


def test_the_replicates_of_a_row_are_bernoulli_draws_of_its_p():
    """40 rows, K = 4000, seed 2024, the mirror alone.  For every row |rep_freq_r - p_mean_r| <= 5 sqrt(sum_k p_rk (1 - p_rk)) / K: the standard deviation of
    the sum of the row's K Bernoulli draws, five times.  With seed 2024 the mirror passes: the largest ratio of a row's deviation to ITS bound is 0.411 (2.1 sigma, row 29)."""
    X, _ = synth.logistic_problem(4, 40)
    slab = 0.8 * np.random.default_rng(5).standard_normal((20, 4, 200))
    K = 4000
    cols = slab.transpose(0, 2, 1).reshape(K, 4)
    eta = X @ cols.T                                                           # the statistics, not the bits, are under test: numpy's product will do
    p = predict.prob(slab, X, eta=eta).reshape(40, K)
    yr = predict.yrep(p, predict.uniforms(2024, 40, K))
    p_mean, _, rep_freq = predict.row_stats(p, yr)
    bound = 5.0 * np.sqrt(np.sum(p * (1.0 - p), axis=1)) / K
    ratio = np.abs(rep_freq - p_mean) / bound
    print(f"largest |rep_freq - p_mean| / bound = {ratio.max():.3f} (row {int(ratio.argmax())})")
    assert (bound > 0.0).all() and (ratio <= 1.0).all(), ratio
