"""GPU: mi_mcmc_draws_log_kernel -- out[t][c] = log K(x[t][:][c]) of every column of a slab [n_keep][d][C] (mcmc_amd/csrc/draws_logk.hip) against the CPU
oracle's orc_target_kernel in its plain orders (W = 4, one block), BIT FOR BIT: every output is compared as uint64 and any NaN matches any NaN; there is no
tolerance in this file.

The product kernel (DENSE, LOGISTIC) gives a workgroup 128 columns k = t * C + c, a wave 32 of them, and walks row tiles of 128 rows with the
contraction in steps of 16.  Which shape (n_keep, d, C) reaches what:
  DENSE    (1, 1, 3)       below every tile, K = 3 < 16: one MFMA column tile with 13 idle columns, three waves without a column
           (2, 5, 7)       K = 14, the tile spans both t
           (3, 17, 37)     a ragged contraction (17 = 16 + 1) and row block; K = 111: tiles that span t, a ragged last wave
           (2, 130, 333)   two row tiles (130 = 128 + 2), six workgroups of columns, an odd C: rows of the slab on both 8-byte alignments
           (1, 520, 19)    five row tiles, 33 contraction steps
           (2, 32, 7)      d a multiple of 16: a contraction of full steps only, no ragged last step
  LOGISTIC (2, 3, 5) with 5 rows, (3, 70, 37) with 130 rows (two row tiles, the second with 2 rows), (1, 520, 19) with 70 rows,
           (2, 32, 5) with 16 rows (full steps only)
  ISO, DIAG (3, 300, 37) and NORMAL_MODEL (4, 2, 37) with 50 observations: one lane per column."""
import functools

import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import synth

pytestmark = pytest.mark.gpu

DENSE_SHAPES = [(1, 1, 3), (2, 5, 7), (3, 17, 37), (2, 130, 333), (1, 520, 19), (2, 32, 7)]
LOGIT_SHAPES = [((2, 3, 5), 5), ((3, 70, 37), 130), ((1, 520, 19), 70), ((2, 32, 5), 16)]
_KIND = {"iso": (mcmc_amd.TARGET_GAUSS_ISO, orc.TARGET_ISO), "diag": (mcmc_amd.TARGET_GAUSS_DIAG, orc.TARGET_DIAG),
         "dense": (mcmc_amd.TARGET_GAUSS_DENSE, orc.TARGET_DENSE), "logistic": (mcmc_amd.TARGET_LOGISTIC, orc.TARGET_LOGISTIC),
         "normal": (mcmc_amd.TARGET_NORMAL_MODEL, orc.TARGET_NORMAL_MODEL)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """bit patterns; any NaN matches any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb]))


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _slab(shape, scale=1.0):
    rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2])
    return _frozen(rng.standard_normal(shape) * scale)[0]


@functools.lru_cache(maxsize=None)
def _problem(name, d, n_rows=0):
    """(prec, X, y) of a target, read-only"""
    if name == "iso":
        return None, None, None
    if name == "diag":
        return _frozen(synth.ill_conditioned_diag(d), None, None)
    if name == "dense":
        return _frozen(synth.dense_gaussian_precision(d), None, None)
    if name == "dense_nonsym":           # visibly non-symmetric: the oracle reads row i of the matrix as given
        rng = np.random.default_rng(d + 77)
        return _frozen(np.ascontiguousarray(np.eye(d) + np.triu(rng.standard_normal((d, d)), 1) + 0.01 * np.tril(rng.standard_normal((d, d)), -1)), None, None)
    if name == "logistic":
        X, y = synth.logistic_problem(d, n_rows)
        return _frozen(None, X, y)
    if name == "normal":
        return _frozen(None, None, 1.5 + 2.0 * np.random.default_rng(n_rows).standard_normal(n_rows))
    raise KeyError(name)


def _kind(name):
    return "dense" if name == "dense_nonsym" else name


def _oracle(name, slab, n_rows=0):
    """orc_target_kernel, value only, of every column"""
    n, d, C_ = slab.shape
    prec, X, y = _problem(name, d, n_rows)
    spec = orc.TargetSpec(_KIND[_kind(name)][1], d, prec=prec, X=X, y=y, W=4)
    out = np.empty((n, C_))
    for t in range(n):
        for c in range(C_):
            out[t, c] = spec.kernel(slab[t, :, c], want_grad=False)[0]
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, shape, n_rows=0):
    return _frozen(_oracle(name, _normal_slab(shape) if name == "normal" else _slab(shape), n_rows))[0]


@functools.lru_cache(maxsize=None)
def _normal_slab(shape):
    x = np.array(_slab(shape))
    x[:, 1, :] = np.abs(x[:, 1, :]) + 0.5            # sigma > 0
    return _frozen(x)[0]


def _target(name, d, n_rows=0):
    prec, X, y = _problem(name, d, n_rows)
    return mcmc_amd.make_target(_KIND[_kind(name)][0], d, prec=prec, X=X, y=y)


def _assert_same(got, want, what):
    bad = ~((np.isnan(got) & np.isnan(want)) | (_bits(got) == _bits(want)))
    assert got.shape == want.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dense_is_the_oracle_bit_for_bit(shape):
    got = mcmc_amd.draws_log_kernel(_target("dense", shape[1]), _slab(shape))
    _assert_same(got, _reference("dense", shape), shape)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("shape,n_rows", LOGIT_SHAPES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else f"{s}rows")
def test_logistic_is_the_oracle_bit_for_bit(shape, n_rows):
    got = mcmc_amd.draws_log_kernel(_target("logistic", shape[1], n_rows), _slab(shape))
    _assert_same(got, _reference("logistic", shape, n_rows), (shape, n_rows))
    assert np.isfinite(got).all()


@pytest.mark.parametrize("name", ["iso", "diag"])
def test_separable_gaussians_are_the_oracle_bit_for_bit(name):
    shape = (3, 300, 37)
    _assert_same(mcmc_amd.draws_log_kernel(_target(name, 300), _slab(shape)), _reference(name, shape), name)
    small = (2, 6, 5)                               # d = 6: the tail of the four chains (i = 4, 5) without a second full round
    _assert_same(mcmc_amd.draws_log_kernel(_target(name, 6), _slab(small)), _reference(name, small), name)


def test_normal_model_is_the_oracle_bit_for_bit():
    shape = (4, 2, 37)
    _assert_same(mcmc_amd.draws_log_kernel(_target("normal", 2, 50), _normal_slab(shape)), _reference("normal", shape, 50), shape)


def test_orientation_a_non_symmetric_matrix_is_read_row_by_row():
    shape = (3, 17, 37)
    P = _problem("dense_nonsym", 17)[0]
    assert np.abs(P - P.T).max() > 0.1
    got = mcmc_amd.draws_log_kernel(_target("dense_nonsym", 17), _slab(shape))
    _assert_same(got, _reference("dense_nonsym", shape), "row i of P as given")
    # ... and the transposed pack would have been seen: in fp64 the two orientations differ in most columns
    spec_t = orc.TargetSpec(orc.TARGET_DENSE, 17, prec=np.ascontiguousarray(P.T), W=4)
    other = np.array([[spec_t.kernel(_slab(shape)[t, :, c], want_grad=False)[0] for c in range(37)] for t in range(3)])
    assert (_bits(other) != _bits(got)).mean() > 0.5


_SPECIALS = [np.inf, -np.inf, np.nan, 1e200]


def _poisoned(shape):
    """the slab with single entries of a few columns replaced; returns (slab, the mask [n_keep][C] of touched columns)"""
    n, d, C_ = shape
    x = np.array(_slab(shape))
    rng = np.random.default_rng(99 + d)
    touched = np.zeros((n, C_), dtype=bool)
    for k, v in enumerate(_SPECIALS * 2):           # eight columns, each special twice: once in dimension 0, once in a later one
        t, c = int(rng.integers(n)), 4 * k + 1
        i = 0 if k < 4 else int(rng.integers(1, d))
        x[t, i, c] = v
        touched[t, c] = True
    # both infinities in one column: inf - inf inside a chain
    x[n - 1, 0, C_ - 1], x[n - 1, d - 1, C_ - 1] = np.inf, -np.inf
    touched[n - 1, C_ - 1] = True
    return x, touched


@pytest.mark.parametrize("name,shape,n_rows", [("dense", (3, 17, 37), 0), ("logistic", (3, 70, 37), 130)], ids=["dense", "logistic"])
def test_non_finite_samples_stay_in_their_own_column(name, shape, n_rows):
    x, touched = _poisoned(shape)
    got = mcmc_amd.draws_log_kernel(_target(name, shape[1], n_rows), x)
    want = _oracle(name, x, n_rows)
    _assert_same(got, want, "the touched columns included")                    # which are NaN, which +-inf, and every bit of the rest
    assert not np.isfinite(want[touched]).all()                                # the specials did something
    clean = _reference(name, shape, n_rows)
    assert np.array_equal(_bits(got)[~touched], _bits(clean)[~touched])        # every other column: the untouched run
    assert np.isfinite(got[~touched]).all()


def test_the_result_does_not_depend_on_the_call():
    import torch
    shape = (2, 130, 333)
    slab, want = _slab(shape), _reference("dense", shape)
    tgt = _target("dense", 130)
    first = mcmc_amd.draws_log_kernel(tgt, slab)
    _assert_same(first, want, "first call")
    _assert_same(mcmc_amd.draws_log_kernel(tgt, slab), first, "second call")
    # the slab and out on the device, on torch's current stream: the call only enqueues (the target's host arrays are read before it returns)
    dev = torch.from_numpy(np.array(slab)).cuda()
    out = torch.full((2, 333), -7.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    mcmc_amd.draws_log_kernel(tgt, dev, n_keep=2, n_chains=333, mem=mcmc_amd.MEM_DEVICE, stream=st, out=out)
    _assert_same(out.cpu().numpy(), first, "device slab")
    # ... and with the target on the device as well: nothing is staged, nothing is waited for
    P_dev = torch.from_numpy(np.array(_problem("dense", 130)[0])).cuda()
    tgt_dev = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, 130, prec=P_dev, mem=mcmc_amd.MEM_DEVICE)
    out2 = torch.full((2, 333), -7.0, dtype=torch.float64, device="cuda")
    mcmc_amd.draws_log_kernel(tgt_dev, dev, n_keep=2, n_chains=333, mem=mcmc_amd.MEM_DEVICE, stream=st, out=out2)
    _assert_same(out2.cpu().numpy(), first, "device slab, device target")
    assert np.array_equal(dev.cpu().numpy(), slab)                              # the slab is read only
    # [d][C] is the case n_keep = 1
    state = np.ascontiguousarray(slab[1])
    _assert_same(mcmc_amd.draws_log_kernel(tgt, state), first[1:2], "[d][C] as n_keep = 1")
    # the logistic target on the device, too
    lshape, rows = (3, 70, 37), 130
    X, y = _problem("logistic", 70, rows)[1:]
    X_dev, y_dev = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(y)).cuda()
    ltgt = mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, 70, X=X_dev, y=y_dev, mem=mcmc_amd.MEM_DEVICE)
    ltgt.n_rows = rows
    ldev = torch.from_numpy(np.array(_slab(lshape))).cuda()
    lout = torch.full((3, 37), -7.0, dtype=torch.float64, device="cuda")
    mcmc_amd.draws_log_kernel(ltgt, ldev, n_keep=3, n_chains=37, mem=mcmc_amd.MEM_DEVICE, stream=st, out=lout)
    _assert_same(lout.cpu().numpy(), _reference("logistic", lshape, rows), "logistic, all on the device")


def test_the_trace_is_a_slab_the_diagnostics_take():
    shape = (8, 130, 333)                           # the (2, 130, 333) slab extended to n_keep = 8 with fresh random rows
    slab = np.concatenate([_slab((2, 130, 333)), np.random.default_rng(8).standard_normal((6, 130, 333))])
    assert slab.shape == shape
    lp = mcmc_amd.draws_log_kernel(_target("dense", 130), slab)
    assert lp.shape == (8, 333)
    assert np.array_equal(_bits(lp[:2]), _bits(_reference("dense", (2, 130, 333))))       # a column's value depends on its own column only
    trace = lp.reshape(8, 1, 333)                   # [n_keep][1][C]: as it is
    s = mcmc_amd.draw_stats(trace)
    r = mcmc_amd.draw_stats_ranked(trace)
    for k in ("mean", "rhat", "ess"):
        assert s[k].shape == (1,) and np.isfinite(s[k]).all(), (k, s[k])
    for k in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail"):
        assert r[k].shape == (1,) and np.isfinite(r[k]).all(), (k, r[k])
