"""GPU: mi_mcmc_draws_order_stats / mi_mcmc_draws_quantiles -- exact pooled order statistics of a draws slab [n_keep][d][C] by radix selection
(draws_select.hip).  The result is an integer-defined quantity, so every comparison is BITWISE (the outputs viewed as uint64) against the numpy
statement mcmc_amd/quantiles.py; there is no tolerance anywhere in this file.

Shapes are the smallest at which each path of the kernel is taken: rows shorter than 512 are walked flattened with 8-byte loads, longer ones with
16-byte loads on the aligned body and a peeled head and tail (odd C: the alignment alternates from row to row); rows shorter than 16 384 share a
workgroup, longer ones are cut into pieces."""
import functools

import numpy as np
import pytest

import mcmc_amd
from mcmc_amd import quantiles as Q

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FF8000000000000


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ranks(K):
    return sorted({0, K - 1, K // 2, K // 3})


def _normal(shape, seed=None):
    n, d, C = shape
    rng = np.random.default_rng(n * 1000003 + d * 1009 + C if seed is None else seed)
    return rng.standard_normal(shape) * np.exp(rng.uniform(-3.0, 3.0, (1, d, 1))) + rng.uniform(-2.0, 2.0, (1, d, 1))


@functools.lru_cache(maxsize=None)
def _case(shape):
    """a slab with its sorted keys: shared by the tests, never modified"""
    slab = _normal(shape)
    ks = Q.sorted_keys(slab)
    slab.setflags(write=False)
    ks.setflags(write=False)
    return slab, ks


def _check_order_stats(slab, ranks, ks=None):
    got = mcmc_amd.draws_order_stats(slab, ranks)
    want = Q.order_stats_ref(slab, ranks, ks)
    bad = int((_bits(got) != _bits(want)).sum())
    print(f"{slab.shape}, {len(ranks)} ranks: {bad} of {want.size} order statistics differ")
    assert _same(got, want)
    return got


# the last two: C = 1001 is odd and past 512 (16 rows per workgroup on the 16-byte path, every other row starts 8 bytes off); C = 1 with many draws
RAGGED = [(1, 1, 1), (7, 3, 45), (5, 130, 130), (3, 17, 257), (2, 700, 3), (5, 3, 1001), (40, 2, 1)]


@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "x".join(map(str, s)))
def test_ragged_shapes(shape):
    slab, ks = _case(shape)
    _check_order_stats(slab, _ranks(shape[0] * shape[2]), ks)


def test_dimensions_processed_in_three_groups():
    """The group rule of draws_select.hpp: dims_per_group = min(d, max(1, min(2^28 / (n_ranks * 2048 + wg_per_dim * 1024), 2^22 / wg_per_dim))).  With
    32 ranks and K = 2 * 3 samples (one workgroup per dimension) that is 2^28 / 66 560 = 4 032 dimensions, so d = 2 * 4 032 + 5 = 8 069 is the smallest
    kind of shape that runs as three groups (4 032, 4 032 and a ragged last one of 5), each through all 17 launches on the same histograms."""
    assert (1 << 28) // (32 * 2048 + 1024) == 4032
    shape = (2, 8069, 3)
    slab, ks = _case(shape)
    ranks = [a % 6 for a in range(32)]
    _check_order_stats(slab, ranks, ks)


def test_many_workgroups_per_dimension():
    shape = (9, 3, 40003)                                 # K = 360 027 per dimension: 9 rows of 3 pieces of 13 335, 13 335 and 13 333
    slab, ks = _case(shape)
    _check_order_stats(slab, _ranks(9 * 40003), ks)


@pytest.mark.parametrize("which", ["last_digits_decide", "first_digits_decide"])
def test_every_round_decides(which):
    n, d, C = 4, 2, 4096
    K = n * C
    rng = np.random.default_rng(11)
    if which == "last_digits_decide":                    # 1 + k 2^-52: equal through 44 bits of the key, the answer is fixed in the last two digits
        x = np.stack([1.0 + rng.permutation(K) * 2.0 ** -52 for _ in range(d)])
    else:                                                # +- 2^e (1 + m) over the whole exponent range, subnormals included
        e = rng.integers(-1074, 1024, (d, K))
        x = np.ldexp(1.0 + rng.random((d, K)), e) * rng.choice([-1.0, 1.0], (d, K))
        assert np.isfinite(x).all() and (x == 0).sum() < K // 100
    slab = np.ascontiguousarray(x.reshape(d, n, C).transpose(1, 0, 2))
    ranks = _ranks(K) + [1, 2, 255, 256, 257, K - 2]
    got = _check_order_stats(slab, ranks)
    if which == "last_digits_decide":
        assert np.array_equal(got[:, 0], 1.0 + np.array(ranks) * 2.0 ** -52)


TIES = (3, 5, 2049)


def test_all_equal_slab():
    slab = np.full(TIES, -1.2345678901234567)
    got = _check_order_stats(slab, _ranks(3 * 2049))
    assert (got == -1.2345678901234567).all()
    got = _check_order_stats(np.full((7, 3, 45), 3.5), _ranks(7 * 45))
    assert (got == 3.5).all()


def test_few_distinct_values_and_the_sign_of_zero():
    rng = np.random.default_rng(12)
    slab = rng.choice(np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0]), TIES)
    K = 3 * 2049
    ranks = list(range(0, K, K // 29))[:30] + [K - 1, K // 2]
    got = _check_order_stats(slab, ranks)
    x = slab.transpose(1, 0, 2).reshape(TIES[1], K)
    n_neg = ((x < 0) | ((x == 0) & np.signbit(x))).sum(axis=1)       # how many samples sort at or below -0.0
    n_neg_nonzero = (x < 0).sum(axis=1)
    for a, r in enumerate(ranks):
        zero = got[a] == 0
        assert np.array_equal(zero, (r >= n_neg_nonzero) & (r < n_neg_nonzero + (x == 0).sum(axis=1)))
        assert np.array_equal(np.signbit(got[a])[zero], (r < n_neg)[zero])


def test_standard_normal_slab():
    slab = np.random.default_rng(13).standard_normal(TIES)            # round 1: two to four hot bins
    _check_order_stats(slab, _ranks(3 * 2049))


def test_non_finite_samples():
    shape = (3, 4, 1001)
    K = 3 * 1001
    rng = np.random.default_rng(14)
    slab = rng.standard_normal(shape)
    bits = slab.view(np.uint64)
    n_nan, n_pinf, n_ninf = K // 10, 7, 5
    for i in range(shape[1]):
        idx = rng.permutation(K)
        t, c = np.divmod(idx, 1001)
        nan = np.uint64(0x7FF0000000000000) | rng.integers(1, 1 << 52, n_nan, dtype=np.uint64) | (rng.integers(0, 2, n_nan, dtype=np.uint64) << np.uint64(63))
        bits[t[:n_nan], i, c[:n_nan]] = nan                  # quiet and signalling, both signs, any payload
        slab[t[n_nan:n_nan + n_pinf], i, c[n_nan:n_nan + n_pinf]] = np.inf
        slab[t[n_nan + n_pinf:n_nan + n_pinf + n_ninf], i, c[n_nan + n_pinf:n_nan + n_pinf + n_ninf]] = -np.inf
    assert np.isnan(slab).sum() == n_nan * shape[1]
    ranks = [0, n_ninf - 1, n_ninf, K // 2, K - n_nan - n_pinf - 1, K - n_nan - n_pinf, K - n_nan - 1, K - n_nan, K - n_nan + 1, K - 1]
    got = _check_order_stats(slab, ranks)
    assert (got[0] == -np.inf).all() and (got[1] == -np.inf).all() and np.isfinite(got[2:5]).all()
    assert (got[5] == np.inf).all() and (got[6] == np.inf).all()
    assert (_bits(got[7:]) == NAN_BITS).all()


@pytest.mark.parametrize("which", ["one", "thirty_two", "unsorted_with_repeats", "all_32_equal"])
def test_rank_lists(which):
    shape = (5, 130, 130)
    slab, ks = _case(shape)
    K = 5 * 130
    rng = np.random.default_rng(15)
    ranks = {"one": [K // 3], "thirty_two": [int(r) for r in np.linspace(0, K - 1, 32)],
             "unsorted_with_repeats": [K - 1, 3, K // 2, 3, 0, K - 1, 17, K // 2] + [int(r) for r in rng.integers(0, K, 9)],
             "all_32_equal": [K // 2] * 32}[which]
    _check_order_stats(slab, ranks, ks)


PROBS = [0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.95, 0.999, 1.0]


@pytest.mark.parametrize("shape", [(5, 130, 130), (9, 3, 40003)], ids=lambda s: "x".join(map(str, s)))
def test_quantiles(shape):
    slab, ks = _case(shape)
    got = mcmc_amd.draws_quantiles(slab, PROBS)
    want = Q.quantiles_ref(slab, PROBS, ks)
    print(f"{shape}: {int((_bits(got) != _bits(want)).sum())} of {want.size} quantiles differ")
    assert _same(got, want)


def test_host_and_device_slabs_and_the_cached_workspace():
    import torch
    big, small = (9, 3, 40003), (3, 17, 257)
    slab_b, ks_b = _case(big)
    slab_s, ks_s = _case(small)
    ranks_b, ranks_s = [int(r) for r in np.linspace(0, 9 * 40003 - 1, 32)], _ranks(3 * 257)
    want_b, want_s = Q.order_stats_ref(slab_b, ranks_b, ks_b), Q.order_stats_ref(slab_s, ranks_s, ks_s)
    side = torch.cuda.Stream()
    dev_b, dev_s = torch.from_numpy(slab_b.copy()).cuda(), torch.from_numpy(slab_s.copy()).cuda()
    torch.cuda.synchronize()
    kw = dict(mem=mcmc_amd.MEM_DEVICE, stream=side.cuda_stream)
    assert _same(mcmc_amd.draws_order_stats(slab_b, ranks_b), want_b)                    # a host slab, the default stream
    assert _same(mcmc_amd.draws_order_stats(dev_b, ranks_b, *big, **kw), want_b)         # a device slab, another stream: a large call ...
    assert _same(mcmc_amd.draws_order_stats(dev_s, ranks_s, *small, **kw), want_s)       # ... then a smaller one on its workspace: no stale counts
    assert _same(mcmc_amd.draws_quantiles(dev_s, PROBS, *small, **kw), Q.quantiles_ref(slab_s, PROBS, ks_s))
    assert mcmc_amd.release_workspace() > 0
    assert _same(mcmc_amd.draws_order_stats(dev_s, ranks_s, *small, **kw), want_s)       # a fresh workspace: whatever hipMalloc hands out
    assert _same(mcmc_amd.draws_order_stats(slab_s, ranks_s), want_s)


def test_quantiles_of_an_hmc_run_without_copying_the_draws():
    import torch
    from mcmc_amd import synth
    d, C, n_keep = 128, 2048, 6
    prec = torch.from_numpy(synth.dense_gaussian_precision(d)).cuda()
    theta = torch.from_numpy(np.ascontiguousarray(synth.initial_states(C, d, seed=3).T)).cuda()
    tgt = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=prec, mem=mcmc_amd.MEM_DEVICE)
    st = mcmc_amd.default_settings(rng_seed_value=1, n_burnin_draws=20, n_keep_draws=n_keep, n_leap_steps=16, step_size=0.25)
    draws = torch.zeros((n_keep, d, C), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    mcmc_amd.run("hmc", tgt, st, mcmc_amd.make_chains(theta, C, draws=draws, mem=mcmc_amd.MEM_DEVICE), stream=stream)
    probs = [0.05, 0.5, 0.95]
    got = mcmc_amd.draws_quantiles(draws, probs, n_keep, d, C, mem=mcmc_amd.MEM_DEVICE, stream=stream)
    host = draws.cpu().numpy()
    assert _same(got, Q.quantiles_ref(host, probs))
    assert (got[0] < got[1]).all() and (got[1] < got[2]).all() and np.isfinite(got).all()
