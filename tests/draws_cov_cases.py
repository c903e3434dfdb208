"""Shared by tests/test_covariance_ref_cpu.py, tests/test_gpu_draws_cov.py and tests/test_gpu_mass_adapt_dense.py: the shapes of the covariance tests,
their slabs, the mirror of include/mi_mcmc.h (mcmc_amd/covariance.py) over the CPU oracle's fma chain, and the bit comparison.  No GPU in here."""
import functools

import numpy as np

import orc
from mcmc_amd import covariance

# d below one MFMA tile / the smallest K; d just past 128 (2 x 2 output tiles, a mirrored off-diagonal one) with a ragged C; the same with chunks
# that span slabs; many slabs of an odd width; more than one chunk per tile and more than one mean group; d = 1
SHAPES = [(1, 5, 2), (1, 130, 333), (3, 130, 333), (7, 17, 1001), (1, 200, 20000), (2, 1, 4097)]
# (n_keep, d, C) and what each reaches (the plan values are derived by hand in tests/test_covariance_ref_cpu.py):
#   (2, 300, 401)     T = 3: tiles (1,0), (2,0), (2,1), the last tile row with 44 rows; two chunks, the second with 290 samples (a ragged last step); the
#                     chunk boundary 512 inside slab t = 1
#   (1, 385, 77)      T = 4: six tiles below the diagonal; a last tile row of ONE row; one ragged chunk
#   (40, 3, 7)        C < 16: every step of the contraction and of the mean crosses slabs
#   (600, 2, 1)       C = 1; two chunks
#   (1, 3, 5000)      two mean groups of 2560: the eight-deep unrolled loads, then their tail; 10 chunks
#   (1, 520, 512)     T = 5, 15 tiles; K = KC exactly: full steps only
#   (1, 2, 600000)    K > 512 * 1024: the one shape here whose KC (592) is not the floor of 512; 1014 chunks, 147 mean groups
NEW_SHAPES = [(2, 300, 401), (1, 385, 77), (40, 3, 7), (600, 2, 1), (1, 3, 5000), (1, 520, 512), (1, 2, 600000)]
SAMPLED = {(1, 200, 20000), (1, 520, 512)}        # the mirror runs on sampled elements of every tile; everywhere else on the full matrix
TILE = 128

ORC_MATH = dict(dot=lambda a, b: orc.dot(a, b, 1))


def shape_id(s):
    return "x".join(map(str, s))


def slab(n_keep, d, C):
    rng = np.random.default_rng(1000 * n_keep + 10 * d + C)
    K = n_keep * C
    A = rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)
    x = A @ rng.standard_normal((d, K)) + rng.uniform(-10.0, 10.0, d)[:, None]          # [d][K], k = t C + c
    return np.ascontiguousarray(x.reshape(d, n_keep, C).transpose(1, 0, 2))


@functools.lru_cache(maxsize=None)
def frozen_slab(shape):
    x = slab(*shape)
    x.setflags(write=False)
    return x


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, want, what):
    """bit patterns; any NaN matches any NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((np.isnan(got) & np.isnan(want)) | (bits(got) == bits(want)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def tiles(d):
    T = (d + TILE - 1) // TILE
    return [(ti, tj) for ti in range(T) for tj in range(ti + 1)]


def sample_elements(d, seed=0, n_interior=4):
    """(i, j) with j <= i from EVERY tile with tj <= ti: its four corners (clipped to d; on the diagonal to j <= i) and n_interior random elements.
    Every element of a shape passes through all of the shape's chunks, so a shape with n_chunks >= 2 has that count in every sampled element."""
    rng = np.random.default_rng(seed)
    out = []
    for ti, tj in tiles(d):
        r0, r1 = ti * TILE, min(d, (ti + 1) * TILE) - 1
        c0, c1 = tj * TILE, min(d, (tj + 1) * TILE) - 1
        picked = dict.fromkeys((i, min(j, i)) for i in (r0, r1) for j in (c0, c1))
        n_tile = (r1 - r0 + 1) * (r1 - r0 + 2) // 2 if ti == tj else (r1 - r0 + 1) * (c1 - c0 + 1)
        want = min(n_tile, len(picked) + n_interior)                     # n_interior FURTHER elements, where the tile has that many
        while len(picked) < want:
            i, j = int(rng.integers(r0, r1 + 1)), int(rng.integers(c0, c1 + 1))
            picked[(max(i, j), min(i, j)) if ti == tj else (i, j)] = None
        out += list(picked)
    return out


def mirror(x, shape_key=None):
    """dict(mean [d], and cov [d, d] or elements {(i, j): value}) of a slab in the header's order, over the oracle's fma chain"""
    d = x.shape[-2]
    sampled = shape_key in SAMPLED or d > 400
    res = dict(mean=covariance.mean_ref(x), cov=None, elements=None)
    if sampled:
        res["elements"] = covariance.covariance_ref(x, math=ORC_MATH, elements=sample_elements(d))
    else:
        res["cov"] = covariance.covariance_ref(x, math=ORC_MATH)
        res["cov"].setflags(write=False)
    res["mean"].setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference(shape):
    """the mirror of frozen_slab(shape): computed once, shared, read-only"""
    return mirror(frozen_slab(shape), shape)


def assert_is_the_mirror(mean, cov, ref, what):
    """a device (mean, cov) against mirror(): every element the mirror has, bit for bit; either output may be None"""
    if mean is not None:
        assert_same(mean, ref["mean"], (what, "mean"))
    if cov is None:
        return
    if ref["cov"] is not None:
        assert_same(cov, ref["cov"], (what, "cov"))
    else:
        ij = np.array(list(ref["elements"]))
        want = np.array(list(ref["elements"].values()))
        assert_same(cov[ij[:, 0], ij[:, 1]], want, (what, "cov, sampled (i, j)"))
        assert_same(cov[ij[:, 1], ij[:, 0]], want, (what, "cov, sampled (j, i)"))
