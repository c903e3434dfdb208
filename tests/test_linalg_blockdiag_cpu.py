"""CPU: the reference that tests/test_gpu_linalg.py uses near the capacity edge (d = 3 840, where orc_inv of the whole matrix costs minutes) is the
oracle's: for a block-diagonal matrix, orc_inv / orc_chol_lower of the whole equal the block-diagonal of orc_inv / orc_chol_lower of the blocks, bit
for bit and including the signs of the zeros outside the blocks.

Why: at step c the rows outside the pivot's block hold f = a[r][c] == 0 and are skipped, and an exact zero never wins the pivot search against the
block's own non-zero column (strict >), so every block sees exactly the operations of its own factorisation.  The zeros outside the blocks are only
ever divided by a pivot and combined as 0 - f * 0: they keep the sign +0.0 as long as every PIVOT IS POSITIVE (0.0 / negative = -0.0).  SPD blocks
that do not swap rows, and the general block of linalg_cases.pivoting_block (swaps at most steps, positive pivots by construction) satisfy that;
the last test shows a block with a negative pivot leaving -0.0 outside the blocks, i.e. where the property ends -- such blocks are not used."""
import numpy as np

from linalg_cases import block_diag, blockwise, orc_chol, orc_inv, pivoting_block, same, spd


def _spd_blocks():
    return [spd(64, 1), spd(71, 2), spd(65, 3)]              # d = 200


def test_inverse_of_a_block_diagonal_spd_matrix_is_the_blockwise_inverse():
    blocks = _spd_blocks()
    M = block_diag(blocks)
    assert M.shape == (200, 200)
    assert same(orc_inv(M), blockwise(orc_inv, blocks))


def test_cholesky_of_a_block_diagonal_spd_matrix_is_the_blockwise_cholesky():
    blocks = _spd_blocks()
    assert same(orc_chol(block_diag(blocks)), blockwise(orc_chol, blocks))


def test_inverse_with_a_general_block_that_pivots():
    G = pivoting_block(71, 4)
    assert not np.array_equal(G, G.T)
    assert (np.abs(G).argmax(axis=0) != np.arange(71)).sum() > 60      # the largest entry of most columns is off the diagonal: rows swap
    blocks = [spd(64, 1), G, spd(65, 3)]
    assert same(orc_inv(block_diag(blocks)), blockwise(orc_inv, blocks))


def test_where_the_property_ends_a_negative_pivot_leaves_negative_zeros_outside_the_block():
    blocks = [spd(64, 1), -spd(71, 2), spd(65, 3)]
    whole, ref = orc_inv(block_diag(blocks)), blockwise(orc_inv, blocks)
    assert np.array_equal(whole, ref)                        # the values agree (-0.0 == 0.0) ...
    assert np.signbit(whole[64:135, :64]).any() and not np.signbit(ref[64:135, :64]).any()      # ... the signs of the zeros do not


def test_a_matrix_beyond_the_staging_budget_runs_on_the_calling_thread_and_equals_the_oracle():
    """mi_mcmc_mat_inverse / mi_mcmc_mat_cholesky_lower beyond the (lowered) staging budget: the host loops -- no device is asked for, so this runs
    anywhere; the oracle's bits, also where the elimination pivots, and the memo answers the repeated call"""
    import mcmc_amd
    mcmc_amd.test_set_linalg_stage_bytes(1024)              # INV needs 16 d bytes, CHOL_LOWER 8 d: d = 130 is beyond both
    try:
        for M in (spd(130, 5), spd(130, 6, 1e4), pivoting_block(200, 7)):
            n0, v0 = mcmc_amd.test_linalg_computed(), mcmc_amd.test_linalg_computed_on_device()
            assert same(mcmc_amd.mat_inverse(M), orc_inv(M)) and same(mcmc_amd.mat_inverse(M), orc_inv(M))
            assert mcmc_amd.test_linalg_computed() - n0 == 1 and mcmc_amd.test_linalg_computed_on_device() == v0
        M = spd(130, 5)
        assert same(mcmc_amd.mat_cholesky_lower(M), orc_chol(M))
    finally:
        mcmc_amd.test_set_linalg_stage_bytes(0)
