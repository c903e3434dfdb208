"""CPU: the host arithmetic of mcmc::nuts on the matrix-product route (mcmc_amd/csrc/gemm_nuts.hpp) -- the tick ceiling of the host loop, the workspace per
chain and the split of a call's chains into ranges -- through the test hooks of mi_mcmc_probes.h.  Plain functions: no device."""

import pytest

import mcmc_amd

SEARCH_TICKS = 4096


def _points(j):
    """distinct points of a depth-j doubling's trajectory"""
    return 1 + j * (j + 1) // 2


@pytest.mark.parametrize("D", range(1, 11))
def test_tick_ceiling(D):
    """INIT, the search's allowance (a fresh run only), and per draw: the evaluation at prev_draw, one re-evaluation per doubling that is not the last, every point of
    every doubling"""
    per_draw = 1 + (D - 1) + sum(_points(j) for j in range(D))
    for n in (0, 1, 7, 2000):
        assert mcmc_amd.test_gemm_nuts_tick_ceiling(D, n, search=False) == 1 + n * per_draw
        assert mcmc_amd.test_gemm_nuts_tick_ceiling(D, n, search=True) == 1 + SEARCH_TICKS + 1 + n * per_draw
    assert sum(_points(j) for j in range(10)) == 175      # (max_tree_depth 10: 1023 leaves on 175 points)


@pytest.mark.parametrize("d,n_rows", [(513, 0), (1024, 0), (1100, 0), (513, 40), (700, 300), (1024, 4096)])
@pytest.mark.parametrize("D", [1, 4, 10])
def test_workspace_per_chain(d, n_rows, D):
    """11 fixed vectors and 2 (theta, p) record vectors per point of the deepest doubling, of d padded to 16; the logistic target's two row-term vectors; the scalars of
    the chain's four lanes; the column words"""
    dK, nK = (d + 15) // 16 * 16, (n_rows + 15) // 16 * 16
    want = ((11 + 2 * _points(D - 1)) * dK + 2 * nK + 4 * 184 + 3) * 8
    assert mcmc_amd.test_gemm_nuts_chain_bytes(d, n_rows, D) == want
    if (d, n_rows, D) == (1024, 0, 10):
        assert 0.8e6 < want < 0.9e6
    # what does not depend on the chains: P^T [dK][dM], resp. X^T [dK][nM] and X [nK][dM] (M: padded to 128), and the counters
    dM, nM = (d + 127) // 128 * 128, (n_rows + 127) // 128 * 128
    assert mcmc_amd.test_gemm_nuts_fixed_bytes(d, n_rows) == ((dK * nM + nK * dM if n_rows else dK * dM) + 32) * 8


def test_range_split_in_multiples_of_128():
    cb, fb = 1000, 5000
    f = mcmc_amd.test_gemm_nuts_range_chains
    assert f(300, cb, fb, fb + 384 * cb) == 384            # everything fits: the chains padded to the tile
    assert f(300, cb, fb, fb + 10**9) == 384
    assert f(300, cb, fb, fb + 383 * cb) == 256            # two tiles fit: 256 + 44
    assert f(300, cb, fb, fb + 128 * cb) == 128            # three ranges
    assert f(300, cb, fb, fb + 128 * cb - 1) == 0          # not even one range: the call stays literal
    assert f(300, cb, fb, fb - 1) == 0 and f(300, cb, fb, 0) == 0
    assert f(1, cb, fb, fb + 128 * cb) == 128 and f(1, cb, fb, fb + 127 * cb) == 0
    for C in (1, 127, 128, 129, 300, 65536):
        for tiles in range(0, 8):
            r = f(C, cb, fb, fb + tiles * 128 * cb + 77)
            assert r % 128 == 0 and r == min(tiles * 128, (C + 127) // 128 * 128)
            if r:
                n_ranges = (C + r - 1) // r
                assert (n_ranges - 1) * r < C <= n_ranges * r
