"""Shared by tests/test_nested_rhat_ref_cpu.py and tests/test_gpu_draws_nested.py: the shapes of the nested R-hat tests, their slabs, the mirror of
include/mi_mcmc.h (mcmc_amd/nested_rhat.py) and the bit comparison.  No GPU in here."""
import functools

import numpy as np

from mcmc_amd import nested_rhat

OUTPUTS = ("nrhat", "mean", "between", "within", "mcse_mean", "super_mean")
RANKED_OUTPUTS = ("nrhat", "nrhat_bulk", "nrhat_tail")
TILE = 256              # chains of one chain-moments workgroup
UNROLL = 8              # draws of one unrolled step of a column

# (N, d, C, M) and what each reaches; K = C / M.  Together: M in {1, 2, 3, 63, 64, 65, 130}, K in {2, 3, 8, 65, 130}, N in {1, 2, 3, 8, 9, 17, 130},
# d in {1, 3, 129}, C below, at and past whole chain tiles.
#   (1, 3, 128, 64)     the chains' state: no centred pass; M = 64 fills SUM64's lanes exactly once; K = 2, the smallest
#   (2, 1, 3, 1)        M = 1 (Bt = +0), one dimension, three chains: every sum shorter than its lanes or its unrolled step
#   (3, 129, 6, 2)      d = 129: the dimension fold's last workgroup holds one wave with work and three without
#   (17, 3, 195, 3)     K = 65: a second element in lane 0 of the dimension fold; two unrolled steps and one draw behind them; C below one tile
#   (130, 3, 126, 63)   sixteen unrolled steps and two draws behind them; M = 63 leaves SUM64's last lane empty
#   (1, 1, 130, 65)     M = 65: a second element in lane 0 of the superchain fold
#   (2, 3, 390, 130)    M = 130: three elements in lanes 0 and 1; two chain tiles, the second ragged; superchain 1 spans both
#   (17, 1, 4225, 65)   K = 65 with M = 65; 17 chain tiles, the last with 129 chains
#   (3, 3, 65, 1)       M = 1 with K = 65
#   (8, 3, 512, 64)     N = one unrolled step exactly, C = two whole tiles
#   (1, 129, 260, 130)  the state at d = 129, two tiles
#   (9, 3, 8320, 64)    K = 130: three elements per lane in the dimension fold; 33 tiles, the last with 128 chains
SHAPES = [(1, 3, 128, 64), (2, 1, 3, 1), (3, 129, 6, 2), (17, 3, 195, 3), (130, 3, 126, 63), (1, 1, 130, 65), (2, 3, 390, 130), (17, 1, 4225, 65),
          (3, 3, 65, 1), (8, 3, 512, 64), (1, 129, 260, 130), (9, 3, 8320, 64)]
# the ranked form: the state, a slab with K = 65, two tiles with M = 130, and five dimensions (one per group under the smallest budget)
RANKED_SHAPES = [(1, 3, 128, 64), (17, 3, 195, 3), (2, 3, 390, 130), (3, 5, 6, 2)]


def shape_id(s):
    return "x".join(map(str, s))


def slab(N, d, C, M):
    """chains that have not quite forgotten their superchain's start: unit noise, an offset per dimension, a smaller one per superchain"""
    rng = np.random.default_rng(100000 * N + 1000 * d + 10 * C + M)
    K = C // M
    x = rng.standard_normal((N, d, C)) + rng.uniform(-10.0, 10.0, d)[None, :, None]
    x += 0.3 * np.repeat(rng.standard_normal((d, K)), M, axis=1)[None]
    return np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def frozen_slab(shape):
    x = slab(*shape)
    x.setflags(write=False)
    return x


def _frozen(res):
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference(shape):
    """the mirror of frozen_slab(shape): computed once, shared, read-only"""
    return _frozen(nested_rhat.nested_ref(frozen_slab(shape), shape[3]))


@functools.lru_cache(maxsize=None)
def ranked_reference(shape):
    return _frozen(nested_rhat.nested_ranked_ref(frozen_slab(shape), shape[3]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, want, what):
    """bit patterns; any NaN matches any NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((np.isnan(got) & np.isnan(want)) | (bits(got) == bits(want)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def assert_is_the_mirror(got, ref, what, names=OUTPUTS):
    """a device result (dict; an output that was not asked for is None) against the mirror's: every output there is, bit for bit"""
    for k in names:
        if got[k] is not None:
            assert_same(got[k], ref[k], (what, k))
