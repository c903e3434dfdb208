"""GPU: mi_mcmc_draws_rank_transform -- the exact average rank, or its normal score, of every retained sample of a slab [n_keep][d][C] among the retained
samples of its dimension (mcmc_amd/csrc/draws_rank.hip: a full radix sort of every dimension's keys and a two-level search) against
mcmc_amd/rank_stats.py, BIT FOR BIT: every output is compared as uint64, there is no tolerance in this file.

The sort works on a dimension's key image [S], key s = r * C + c of retained row r, in tiles of RANK_TILE = 16 384 keys (a count / scatter workgroup:
four waves, each a quarter of the tile in chunks of 64); the lookup keeps every 4 096th sorted key in LDS.  Which shape runs what:
  (1, 1, 1)       one key; with MI_RANK_SPLIT n_keep = 1 is MI_ERR_BAD_ARG, which is what the test asks there
  (7, 3, 45)      rows shorter than 512: the flattened 8-byte loads; odd n_keep, so the split drops the middle row
  (5, 3, 1001)    odd C past 512: the 16-byte body with a peeled head or tail, the alignment alternating from row to row
  (40, 2, 1)      C = 1: every row one key
  (2, 700, 3)     many dimensions of six keys: 700 workgroups of one ragged chunk
  (3, 2, 16385)   one key more than a tile per row: four tiles (three with the split), every tile boundary inside a row, so row pieces start on both
                  alignments; the last tile holds 3 keys (2 with the split): three of a scatter workgroup's four waves have nothing
  (9, 2, 40003)   22 tiles with a ragged last one: offsets over many tiles, 88 keys in the lookup's first level."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import mcmc_amd
from mcmc_amd import quantiles as Q
from mcmc_amd import rank_stats as R

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FF8000000000000
WHATS = ["average", "normal"]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]          # (split, fold)
_FLAG_ID = {(False, False): "plain", (True, False): "split", (False, True): "fold", (True, True): "split_fold"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _slab(shape):
    n, d, C_ = shape
    rng = np.random.default_rng(n * 1000003 + d * 1009 + C_)
    x = rng.standard_normal(shape) * np.exp(rng.uniform(-20.0, 20.0, (1, d, 1))) + rng.standard_normal((1, d, 1))
    x.setflags(write=False)
    return x


def _check(slab, what, split, fold, **kw):
    got = mcmc_amd.draws_rank_transform(slab, what, split=split, fold=fold, **kw)
    want = R.rank_transform_ref(slab, what, split=split, fold=fold)
    assert _same(got, want), (what, split, fold, int((_bits(got) != _bits(want)).sum()))
    return got


def _counts():
    so, pa = C.c_uint64(0), C.c_uint64(0)
    mcmc_amd.lib().mi_mcmc_test_rank_counts(C.byref(so), C.byref(pa))
    return so.value, pa.value


RAGGED = [(1, 1, 1), (7, 3, 45), (5, 3, 1001), (40, 2, 1), (2, 700, 3), (3, 2, 16385), (9, 2, 40003)]


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: _FLAG_ID[f])
@pytest.mark.parametrize("what", WHATS)
@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "x".join(map(str, s)))
def test_ragged_shapes(shape, what, flags):
    split, fold = flags
    slab = _slab(shape)
    if split and shape[0] < 2:                             # the header's rule: no halves of one draw
        with pytest.raises(mcmc_amd.MiMcmcError) as e:
            mcmc_amd.draws_rank_transform(slab, what, split=True, fold=fold)
        assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
        return
    got = _check(slab, what, split, fold)
    n, d, C_ = shape
    assert got.shape == ((n // 2, d, 2 * C_) if split else shape)
    if what == "average" and not fold:                     # a continuous slab: a permutation of 1 .. S in every dimension
        S = got.shape[0] * got.shape[2]
        assert np.array_equal(np.sort(got.transpose(1, 0, 2).reshape(d, S), axis=1), np.tile(np.arange(1.0, S + 1.0), (d, 1)))


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: _FLAG_ID[f])
@pytest.mark.parametrize("which", ["last_digits_decide", "first_digits_decide"])
def test_every_digit_decides(which, flags):
    """1 + k 2^-52: the six upper digits of the keys are constant, so six passes are skipped and the two lowest sort alone.  +- 2^e (1 + m) over the
    whole exponent range: every digit varies, all eight passes run."""
    n, d, C_ = 4, 2, 4096
    K = n * C_
    rng = np.random.default_rng(11)
    if which == "last_digits_decide":
        x = np.stack([1.0 + rng.permutation(K) * 2.0 ** -52 for _ in range(d)])
    else:
        e = rng.integers(-1074, 1024, (d, K))
        x = np.ldexp(1.0 + rng.random((d, K)), e) * rng.choice([-1.0, 1.0], (d, K))
        assert np.isfinite(x).all() and (x == 0).sum() < K // 100
    slab = np.ascontiguousarray(x.reshape(d, n, C_).transpose(1, 0, 2))
    split, fold = flags
    before = _counts()
    for what in WHATS:
        got = _check(slab, what, split, fold)
    sorts, passes = (b - a for a, b in zip(before, _counts()))
    assert sorts == (4 if fold else 2)                     # per call one sort of x, with fold another of |x - med|
    if which == "first_digits_decide":
        assert passes == 8 * sorts
    elif not fold:                                         # K = 2^14 keys 1 + k 2^-52 (the split keeps them all): 14 bits vary, two digits
        assert passes == 2 * sorts
    else:                                                  # |x - med| spreads over the exponents again: only the sorts of x skip six passes
        assert 2 * 2 + 2 <= passes <= 2 * 2 + 2 * 8
    if which == "last_digits_decide" and not split and not fold:
        got = mcmc_amd.draws_rank_transform(slab, "average")
        assert np.array_equal(got, (slab - 1.0) * 2.0 ** 52 + 1.0)                      # the value 1 + k 2^-52 has rank k + 1


TIES = (3, 5, 2049)


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: _FLAG_ID[f])
def test_ties_share_the_average_rank(flags):
    rng = np.random.default_rng(5)
    slab = rng.choice(np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0]), TIES)
    split, fold = flags
    r = _check(slab, "average", split, fold)
    _check(slab, "normal", split, fold)
    S = r.shape[0] * r.shape[2]
    assert ((2.0 * r).sum(axis=(0, 2)) == S * (S + 1.0)).all()                           # sum of R2, whatever the ties
    if not fold:                                           # -0.0 below +0.0: two different ranks
        v = R.retained(slab, split)
        neg, pos = r[(v == 0) & np.signbit(v)], r[(v == 0) & ~np.signbit(v)]
        assert neg.size and pos.size and neg.max() < pos.min()


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: _FLAG_ID[f])
def test_all_equal_slab(flags):
    split, fold = flags
    slab = np.full(TIES, -1.2345678901234567)
    r = _check(slab, "average", split, fold)
    S = r.shape[0] * r.shape[2]
    assert (r == (S + 1) / 2.0).all()
    z = _check(slab, "normal", split, fold)
    assert (_bits(z) == 0).all()                                                         # p = 0.5 exactly: +0.0


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: _FLAG_ID[f])
@pytest.mark.parametrize("what", WHATS)
def test_non_finite_samples(what, flags):
    split, fold = flags
    shape = (7, 3, 45)
    clean = np.array(_slab(shape))
    slab = clean.copy()
    rng = np.random.default_rng(9)
    flat = rng.permutation(7 * 45)[:12]
    t, c = flat // 45, flat % 45
    special = np.array([np.inf, -np.inf, np.inf, -np.inf, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float64)
    special[4:].view(np.uint64)[:] = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
                                      0xFFFFFFFFFFFFFFFF, 0x7FF8000000000123, 0xFFF4000000000000]
    slab[t, 1, c] = special
    assert np.isnan(slab[:, 1]).sum() == 8
    got = _check(slab, what, split, fold)
    base = _check(clean, what, split, fold)
    assert _same(got[:, [0, 2]], base[:, [0, 2]])                                        # the other dimensions do not see them
    v = R.retained(slab, split)[:, 1]
    g1 = got[:, 1]
    assert (_bits(g1[np.isnan(v)]) == NAN_BITS).all() and np.isnan(v).sum() >= 4
    # +-inf: a finite rank and score (folded too: with 8 NaNs and 2 +inf on top of 315 samples the median is finite, |inf - med| = inf)
    assert np.isfinite(g1[np.isinf(v)]).all() and np.isinf(v).any()
    assert np.isfinite(g1[~np.isnan(v)]).all()
    if what == "average" and not fold:                     # the NaNs sit on top: the others rank as they do among themselves
        assert np.array_equal(g1[~np.isnan(v)], R.average_ranks(v[~np.isnan(v)].reshape(1, 1, -1)).ravel())


def _set_budget(b):
    mcmc_amd.lib().mi_mcmc_test_set_rank_ws_bytes(b)


def _dim_bytes(n_keep, C_, flags):
    return mcmc_amd.lib().mi_mcmc_test_rank_dim_bytes(n_keep, C_, flags, 0)


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: _FLAG_ID[f])
def test_dimensions_processed_in_three_groups(flags):
    split, fold = flags
    shape = (7, 5, 45)
    slab = _slab(shape)
    whole = [_check(slab, what, split, fold) for what in WHATS]
    f = mcmc_amd.lib().mi_mcmc_test_rank_dims_per_group
    try:
        _set_budget(2 * _dim_bytes(7, 45, int(split) | 2 * int(fold)))
        assert f(7, 5, 45, int(split) | 2 * int(fold), 0) == 2     # groups of 2, 2, 1
        for what, w in zip(WHATS, whole):
            assert _same(mcmc_amd.draws_rank_transform(slab, what, split=split, fold=fold), w)
    finally:
        _set_budget(0)


def test_device_resident_on_another_stream():
    import torch
    shape = (5, 3, 1001)
    slab = _slab(shape)
    side = torch.cuda.Stream()
    dev = torch.from_numpy(np.array(slab)).cuda()
    torch.cuda.synchronize()
    for what, (split, fold) in itertools.product(WHATS, FLAGS):
        host = mcmc_amd.draws_rank_transform(slab, what, split=split, fold=fold)
        out = torch.full(host.shape, -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        mcmc_amd.draws_rank_transform(dev, what, split=split, fold=fold, n_keep=5, d=3, n_chains=1001, mem=mcmc_amd.MEM_DEVICE, stream=side.cuda_stream, out=out)
        assert _same(out.cpu().numpy(), host)              # (the call is blocking: the stream has finished)
    assert np.array_equal(dev.cpu().numpy(), slab)         # the slab is read only


def test_the_cached_workspace_holds_no_stale_counts():
    import torch
    big, small = (9, 2, 40003), (3, 17, 257)
    side = torch.cuda.Stream()
    dev_b, dev_s = torch.from_numpy(np.array(_slab(big))).cuda(), torch.from_numpy(np.array(_slab(small))).cuda()
    torch.cuda.synchronize()
    kw = dict(mem=mcmc_amd.MEM_DEVICE, stream=side.cuda_stream)
    out_b = torch.empty((4, 2, 80006), dtype=torch.float64, device="cuda")
    for what, (split, fold) in itertools.product(WHATS, [(True, True), (False, False)]):
        mcmc_amd.draws_rank_transform(dev_b, "normal", split=True, fold=True, n_keep=9, d=2, n_chains=40003, out=out_b, **kw)
        want = R.rank_transform_ref(_slab(small), what, split=split, fold=fold)
        out_s = torch.empty(want.shape, dtype=torch.float64, device="cuda")
        mcmc_amd.draws_rank_transform(dev_s, what, split=split, fold=fold, n_keep=3, d=17, n_chains=257, out=out_s, **kw)
        assert _same(out_s.cpu().numpy(), want)            # on the workspace the larger call left behind
    assert mcmc_amd.release_workspace() > 0
    want = R.rank_transform_ref(_slab(small), "average")
    assert _same(mcmc_amd.draws_rank_transform(_slab(small), "average"), want)           # a fresh workspace: whatever hipMalloc hands out


def test_ranks_agree_with_the_order_statistics():
    shape = (5, 3, 1001)
    slab = _slab(shape)
    r = mcmc_amd.draws_rank_transform(slab, "average")
    pooled_r = r.transpose(1, 0, 2).reshape(3, -1)
    pooled_x = slab.transpose(1, 0, 2).reshape(3, -1)
    ks = [0, 1, 17, 2502, 5003, 5004]
    os_ = mcmc_amd.draws_order_stats(slab, ks)
    for a, k in enumerate(ks):
        for i in range(3):
            at = np.flatnonzero(pooled_r[i] == k + 1.0)
            assert at.size == 1                                                          # continuous draws: every rank is unique
            assert _bits(pooled_x[i, at])[0] == _bits(os_[a, i : i + 1])[0]
