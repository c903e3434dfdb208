"""CPU: the host arithmetic of mcmc::nuts with settings.vals_bound on the matrix-product route (mcmc_amd/csrc/gemm_nuts.hpp) -- the workspace per chain with bounds
(one vector of padded d more: theta of the last point next to x = inv_transform(theta), which the products read) and the split of a call's chains into ranges under
it -- through the test hooks of mi_mcmc_probes.h.  Plain functions: no device."""

import pytest

import mcmc_amd

SHAPES = [(513, 0), (1024, 0), (1100, 0), (513, 40), (700, 300), (1024, 4096)]


def _points(j):
    """distinct points of a depth-j doubling's trajectory"""
    return 1 + j * (j + 1) // 2


def _pad(n, m):
    return (n + m - 1) // m * m


@pytest.mark.parametrize("d,n_rows", SHAPES)
@pytest.mark.parametrize("D", [1, 4, 10])
def test_bounded_workspace_per_chain_is_the_documented_rule(d, n_rows, D):
    """include/mi_mcmc.h: 12 fixed vectors (the unbounded 11 and theta of the last point) and 2 (theta, p) record vectors per point of the deepest doubling, of d
    padded to 16; the logistic target's two row-term vectors; the scalars of the chain's four lanes; the column words"""
    dK, nK = _pad(d, 16), _pad(n_rows, 16)
    want = ((12 + 2 * _points(D - 1)) * dK + 2 * nK + 4 * 184 + 3) * 8
    assert mcmc_amd.test_gemm_nuts_bounded_chain_bytes(d, n_rows, D) == want


@pytest.mark.parametrize("d,n_rows", SHAPES)
@pytest.mark.parametrize("D", [1, 4, 10])
def test_bounds_cost_whole_padded_vectors_and_the_old_hook_keeps_its_values(d, n_rows, D):
    dK, nK = _pad(d, 16), _pad(n_rows, 16)
    plain = mcmc_amd.test_gemm_nuts_chain_bytes(d, n_rows, D)
    assert plain == ((11 + 2 * _points(D - 1)) * dK + 2 * nK + 4 * 184 + 3) * 8          # tests/test_gemm_nuts_host.py's figure, unchanged
    extra = mcmc_amd.test_gemm_nuts_bounded_chain_bytes(d, n_rows, D) - plain
    assert extra > 0 and extra % (dK * 8) == 0 and extra // (dK * 8) == 1
    # what does not depend on the chains does not depend on the bounds either: one figure
    dM, nM = _pad(d, 128), _pad(n_rows, 128)
    assert mcmc_amd.test_gemm_nuts_fixed_bytes(d, n_rows) == ((dK * nM + nK * dM if n_rows else dK * dM) + 32) * 8


@pytest.mark.parametrize("d,n_rows,D", [(700, 0, 4), (1024, 4096, 6)])
def test_range_split_with_the_bounded_figure(d, n_rows, D):
    cb, fb = mcmc_amd.test_gemm_nuts_bounded_chain_bytes(d, n_rows, D), mcmc_amd.test_gemm_nuts_fixed_bytes(d, n_rows)
    plain = mcmc_amd.test_gemm_nuts_chain_bytes(d, n_rows, D)
    f = mcmc_amd.test_gemm_nuts_range_chains
    assert f(300, cb, fb, fb + 384 * cb) == 384            # everything fits: the chains padded to the tile
    assert f(300, cb, fb, fb + 384 * cb - 1) == 256
    assert f(300, cb, fb, fb + 128 * cb + cb // 2) == 128  # three ranges
    assert f(300, cb, fb, fb + 128 * cb - 1) == 0          # not even one range: the call stays on the literal kernel
    assert f(300, cb, fb, fb + 127 * cb) == 0
    # a budget that holds one range of unbounded chains exactly does not hold one of bounded chains
    assert f(300, plain, fb, fb + 128 * plain) == 128 and f(300, cb, fb, fb + 128 * plain) == 0
    for C in (1, 129, 300, 65536):
        for tiles in range(0, 6):
            r = f(C, cb, fb, fb + tiles * 128 * cb + 77)
            assert r == min(tiles * 128, _pad(C, 128))
