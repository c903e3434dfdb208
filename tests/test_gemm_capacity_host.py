"""CPU: the host arithmetic of the capacity condition of hmc / mala / rwmh on the matrix-product route (mcmc_amd/csrc/mi_mcmc.hip: gemm_fits, gemm_need_bytes) through the
test hook mi_mcmc_test_gemm_need_bytes of mi_mcmc_probes.h -- what a call needs next to the memory there is.  Plain functions: no device."""

import pytest

import mcmc_amd

PLAIN, DENSE_M, BOUNDED = mcmc_amd.GEMM_PLAIN, mcmc_amd.GEMM_DENSE_M, mcmc_amd.GEMM_BOUNDED


def _up(x, m):
    return (x + m - 1) // m * m


def _ws_bytes(d, n_rows, C, variant):
    """gemm_ws_bytes (gemm_samplers.hip: gemm_carve): the packed matrices | six state vectors | two row-term vectors | prevE, kprev, nacc | the draw counter | a dense
    precond_mat's three matrices and four vectors, or vals_bound's three vectors; d padded to 16 (K) and 128 (M), the chains to 128"""
    dK, dM, nK, nM, Cp = _up(d, 16), _up(d, 128), _up(n_rows, 16), _up(n_rows, 128), _up(C, 128)
    doubles = (dK * nM + nK * dM if n_rows else dK * dM) + 6 * dK * Cp + 2 * nK * Cp + 3 * Cp + 32
    if variant == DENSE_M:
        doubles += 3 * dK * dM + 4 * dK * Cp
    if variant == BOUNDED:
        doubles += 3 * dK * Cp
    return doubles * 8


def _replay_bytes(d, n_rows, C):
    """behind the route's own: the non-finite flags, the target's matrix transposed for the literal replay, and its work areas (literal.hpp: lit_work_doubles) for at
    most 512 workgroups"""
    n = n_rows if n_rows else d
    return _up((C + 1) * 4, 256) + (_up(d * max(d, n), 32) + min(C, 512) * (19 * (d + 8) + 2 * (n + 8))) * 8


def _uploads(d, variant):
    """next to the workspace: 1 MiB for the tables and the target's d x d matrix; with a dense precond_mat the replay's four transposed d x d matrices"""
    return (4 if variant == DENSE_M else 1) * d * d * 8 + (1 << 20)


SHAPES = [(513, 0, 1), (513, 0, 1025), (520, 0, 33), (513, 40, 1025), (700, 300, 300), (1024, 0, 65536), (1024, 4096, 600), (3840, 0, 128)]


@pytest.mark.parametrize("d,n_rows,C", SHAPES)
@pytest.mark.parametrize("variant", [PLAIN, DENSE_M, BOUNDED])
def test_need_is_the_workspace_plus_the_documented_extras(d, n_rows, C, variant):
    own = _up(_ws_bytes(d, n_rows, C, variant), 256)
    with_replay = own + _replay_bytes(d, n_rows, C) + _uploads(d, variant)
    assert mcmc_amd.test_gemm_need_bytes(d, n_rows, C, variant, replay=True) == with_replay
    # rwmh has no replay; a dense precond_mat (hmc, mala) always has one
    assert mcmc_amd.test_gemm_need_bytes(d, n_rows, C, variant, replay=False) == (with_replay if variant == DENSE_M else own + _uploads(d, variant))


def test_need_grows_with_chains_dimension_and_variant():
    f = mcmc_amd.test_gemm_need_bytes
    for variant in (PLAIN, DENSE_M, BOUNDED):
        for replay in (False, True):
            by_c = [f(600, 0, C, variant, replay) for C in (1, 127, 128, 129, 300, 1025, 65536)]
            assert by_c == sorted(by_c) and by_c[2] < by_c[3] < by_c[4] < by_c[5] < by_c[6]      # a chain tile more is strictly more
            by_d = [f(d, 0, 300, variant, replay) for d in (513, 528, 529, 640, 1024, 3840)]
            assert by_d == sorted(by_d) and len(set(by_d)) == len(by_d)
            by_n = [f(600, n, 300, variant, replay) for n in (16, 17, 300, 4096)]                # (rows padded to 16 and to 128)
            assert by_n == sorted(by_n) and len(set(by_n)) == len(by_n)
    for d, n_rows, C in SHAPES:
        for replay in (False, True):
            assert f(d, n_rows, C, PLAIN, replay) < f(d, n_rows, C, BOUNDED, replay) < f(d, n_rows, C, DENSE_M, replay)
        assert f(d, n_rows, C, PLAIN, False) < f(d, n_rows, C, PLAIN, True)
    # the benchmarked size of the route -- d = 1024, 65 536 chains -- needs 3.3 GB: far inside the device, so the condition never moves such a call
    assert 3.2e9 < f(1024, 0, 65536, PLAIN, True) < 3.4e9
