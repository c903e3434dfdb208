"""GPU: INV / CHOL_LOWER of a dense precond_mat on the device (mcmc_amd/csrc/linalg_device.hip through mi_mcmc_mat_inverse /
mi_mcmc_mat_cholesky_lower) against the oracle's orc_inv / orc_chol_lower (ref: src/hmc.cpp:58-59, src/mala.cpp:58,
include/stats/dmvnorm.hpp:36-41): every element bit for bit -- random SPD matrices, ill-conditioned ones, matrices whose elimination has to
pivot (also on ties and across NaN), singular / non-SPD input (inf / NaN out, as the reference's unvalidated calls give), sizes around the
64-dimension switch between the calling thread's loops and the device, and sizes that do not divide the grid.

Beyond d = 512 (a dense precond_mat of the matrix-product route, up to d = 3 840): sizes with several row strides per thread, the capacity edge
itself against the block-wise oracle (tests/test_linalg_blockdiag_cpu.py), pivot ties / NaN / inf / zeros placed across the strides, lanes and waves
of the pivot search, late non-positive and zero pivots of CHOL_LOWER, the host loops that serve a matrix beyond the staging budget (through the test
hook that lowers the budget), the routing edge of hmc / mala / nuts / rwmh at that budget, and the two-entry memo."""
import contextlib
import time

import numpy as np
import pytest

import mcmc_amd
import orc
from linalg_cases import block_diag, block_sizes, blockwise, orc_chol, orc_inv, pivoting_block, same, spd


_orc_inv, _orc_chol, _spd, _same = orc_inv, orc_chol, spd, same      # (tests/linalg_cases.py: shared with the CPU test of the block-wise reference)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 65, 100, 128, 255, 256, 300, 512])
def test_device_inverse_and_cholesky_equal_the_oracle_bitwise_on_spd_matrices(d):
    M = _spd(d, d)
    assert _same(mcmc_amd.mat_inverse(M), _orc_inv(M))
    assert _same(mcmc_amd.mat_cholesky_lower(M), _orc_chol(M))
    assert np.abs(mcmc_amd.mat_inverse(M) @ M - np.eye(d)).max() < 1e-8          # ... and it IS the inverse


@pytest.mark.gpu
@pytest.mark.parametrize("d,cond", [(96, 1e3), (200, 1e5), (512, 1e4)])
def test_ill_conditioned_matrices_whose_elimination_pivots(d, cond):
    M = _spd(d, 7 * d, cond)
    assert (np.abs(M).argmax(axis=0) != np.arange(d)).any()    # columns whose diagonal entry is not the largest: rows swap
    assert _same(mcmc_amd.mat_inverse(M), _orc_inv(M))
    assert _same(mcmc_amd.mat_cholesky_lower(M), _orc_chol(M))


@pytest.mark.gpu
def test_general_matrices_pivot_ties_nan_and_singular_input():
    rng = np.random.default_rng(5)
    d = 130
    G = rng.standard_normal((d, d))                             # not symmetric: INV does not care, pivots everywhere
    assert _same(mcmc_amd.mat_inverse(G), _orc_inv(G))
    T = np.round(rng.standard_normal((d, d)) * 2.0)             # small integers: exact ties in the pivot search (the FIRST largest wins), zeros skipped
    T += np.eye(d) * 3
    assert _same(mcmc_amd.mat_inverse(T), _orc_inv(T))
    N = _spd(d, 11)
    N[40, 3] = np.nan                                           # a NaN below the diagonal never wins the pivot search, then poisons what it touches
    assert _same(mcmc_amd.mat_inverse(N), _orc_inv(N))
    N2 = _spd(d, 12)
    N2[5, 5] = np.nan                                           # a NaN ON the diagonal stays the pivot
    assert _same(mcmc_amd.mat_inverse(N2), _orc_inv(N2))
    S = _spd(d, 13)
    S[:, 9] = 0.0; S[9, :] = 0.0                                # singular: division by a zero pivot, inf / NaN entries, no error
    assert _same(mcmc_amd.mat_inverse(S), _orc_inv(S))
    Q = -_spd(d, 14)                                            # not positive definite: sqrt of a negative number
    assert _same(mcmc_amd.mat_cholesky_lower(Q), _orc_chol(Q))
    assert np.isnan(mcmc_amd.mat_cholesky_lower(Q)).any()


@pytest.mark.gpu
def test_small_matrices_stay_on_the_calling_thread_and_agree_too():
    for d in (1, 2, 7, 63):
        M = _spd(d, 100 + d)
        assert _same(mcmc_amd.mat_inverse(M), _orc_inv(M)) and _same(mcmc_amd.mat_cholesky_lower(M), _orc_chol(M))


@pytest.mark.gpu
def test_device_factorisation_time_at_d512():
    """the host's Gauss-Jordan was 89 ms at d = 512 inside every blocking call with a dense precond_mat."""
    M = _spd(512, 3)
    mcmc_amd.mat_inverse(_spd(512, 4)); mcmc_amd.mat_cholesky_lower(_spd(512, 4))      # code-object load (another matrix: M is not memoised)
    t0 = time.perf_counter(); mcmc_amd.mat_inverse(M); t_inv = time.perf_counter() - t0
    t0 = time.perf_counter(); mcmc_amd.mat_cholesky_lower(M); t_chol = time.perf_counter() - t0
    print(f"d = 512: INV {t_inv * 1e3:.1f} ms, CHOL_LOWER {t_chol * 1e3:.1f} ms (device, incl. upload / download)")
    assert t_inv < 0.040 and t_chol < 0.040


# ---------------------------------------------------------------------------------------------------------------------------------------------
# beyond d = 512

@pytest.mark.gpu
@pytest.mark.parametrize("d", [513, 777, 1100])
def test_spd_matrices_beyond_d512_equal_the_oracle_bitwise(d):
    """no multiple of the 256 threads or the 64 workgroups, more than one row stride per thread everywhere (oracle: ~1.5 s at d = 1 100)"""
    M = _spd(d, d)
    assert _same(mcmc_amd.mat_inverse(M), _orc_inv(M))
    assert _same(mcmc_amd.mat_cholesky_lower(M), _orc_chol(M))


@pytest.mark.gpu
def test_ill_conditioned_matrix_beyond_d512_whose_elimination_pivots():
    d = 777
    M = _spd(d, 7 * d, 1e4)
    assert (np.abs(M).argmax(axis=0) != np.arange(d)).any()    # columns whose diagonal entry is not the largest: rows swap
    assert _same(mcmc_amd.mat_inverse(M), _orc_inv(M))
    assert _same(mcmc_amd.mat_cholesky_lower(M), _orc_chol(M))


def _edge_blocks(d, general):
    sizes = block_sizes(d)
    blocks = [_spd(n, 1000 + i) for i, n in enumerate(sizes)]
    if general:
        i = sizes.index(300)
        blocks[i] = pivoting_block(300, 5)                      # one general block that swaps rows (positive pivots: see the CPU test)
    return sizes, blocks


def _capacity_edge(d):
    """block-diagonal with ragged blocks (127, 128, 129, 300 repeated, a remainder) against the per-block oracle -- the oracle's bits for the whole
    matrix, tests/test_linalg_blockdiag_cpu.py -- and the residual |Ainv M - I|_inf within 8 x that of numpy's own inverse of the same matrix.  The three
    factorisations ran the DEVICE kernels (counted: the host loops return the same bits, and on a block-diagonal matrix, whose rows outside the pivot's
    block they skip, they take about as long, so neither the bits nor the time would show a quiet drop to them at the edge)"""
    n_dev0 = mcmc_amd.test_linalg_computed_on_device()
    sizes, blocks = _edge_blocks(d, general=True)
    assert sum(sizes) == d and len(set(sizes)) >= 4
    M = block_diag(blocks)
    t0 = time.perf_counter(); ref = blockwise(_orc_inv, blocks); t_orc = time.perf_counter() - t0
    t0 = time.perf_counter(); Ainv = mcmc_amd.mat_inverse(M); t_inv = time.perf_counter() - t0
    assert _same(Ainv, ref)
    eye = np.eye(d)
    res = np.linalg.norm(Ainv @ M - eye, np.inf)
    res_np = np.linalg.norm(np.linalg.inv(M) @ M - eye, np.inf)
    print(f"d = {d}: INV {t_inv:.2f} s (device), per-block oracle {t_orc:.2f} s; |Ainv M - I|_inf {res:.3e}, numpy's inverse {res_np:.3e}, ratio {res / res_np:.2f}")
    assert res <= 8.0 * res_np
    sizes, blocks = _edge_blocks(d, general=False)
    M = block_diag(blocks)
    t0 = time.perf_counter(); L = mcmc_amd.mat_cholesky_lower(M); t_chol = time.perf_counter() - t0
    assert _same(L, blockwise(_orc_chol, blocks))
    Ainv = mcmc_amd.mat_inverse(M)
    assert _same(Ainv, blockwise(_orc_inv, blocks))
    res = np.linalg.norm(Ainv @ M - eye, np.inf)
    res_np = np.linalg.norm(np.linalg.inv(M) @ M - eye, np.inf)
    print(f"d = {d}: CHOL_LOWER {t_chol:.2f} s (device); SPD blocks: |Ainv M - I|_inf {res:.3e}, numpy's inverse {res_np:.3e}, ratio {res / res_np:.2f}")
    assert res <= 8.0 * res_np
    assert mcmc_amd.test_linalg_computed_on_device() - n_dev0 == 3          # INV (general block), CHOL_LOWER, INV (SPD blocks)


@pytest.mark.gpu
def test_the_capacity_edge_d3840_against_the_blockwise_oracle():
    """d = 3 840: the scaled pivot rows fill the 60 KB staging budget exactly, each of the 64 workgroups owns 60 rows.
    Measured on an MI355X: INV 2.10 s, CHOL_LOWER 0.33 s on the device (upload / download included), the per-block oracle 0.03 s, the whole test 5.9 s
    (the rest: assembling the matrices, numpy's inverse and two products).  Residual |Ainv M - I|_inf 2.50e-14 against 1.22e-14 of numpy's inverse:
    ratio 2.05 of the 8 allowed (d = 2 049: 1.66 / 1.73)."""
    _capacity_edge(3840)


@pytest.mark.gpu
def test_d2049_against_the_blockwise_oracle():
    """one past a multiple of the 256 threads: the ninth row stride of every scan holds one element"""
    _capacity_edge(2049)


# ---- the pivot search: a strided scan of 256 threads (r = c + tid, c + tid + 256, ...), a shuffle reduction over the 64 lanes of a wave, a pass over
# the 4 waves.  "The FIRST index of the largest magnitude wins" in all three; d = 600: three strides at c < 88.

def _tie_matrix(c, r1, r2, seed, d=600, above=None):
    """small integers (exact arithmetic at the step that matters); column c holds its largest magnitude at rows r1 < r2 (with opposite signs) and nowhere
    else.  For c > 0 the leading c x c block is decoupled (zeros beside and below it), so rows >= c reach step c as they are in the input: the tie is
    there BEFORE any elimination, and the assertion on the input is an assertion on what the search sees.
    above = (r0, value), r0 < c: the rows above c are coupled to the columns from c on again, under a leading block 2 I (steps < c halve their own row,
    exactly, and eliminate nothing), and row r0 holds `value` / 2 > 40 in column c when step c searches: the scan starts AT the diagonal, a larger
    magnitude above it is not a candidate."""
    rng = np.random.default_rng(seed)
    T = np.clip(np.round(rng.standard_normal((d, d)) * 2.0), -6.0, 6.0)
    T += np.eye(d) * 3
    T[c:, :c] = 0.0; T[:c, c:] = 0.0
    T[r1, c] = 40.0; T[r2, c] = -40.0
    if above is not None:
        r0, value = above
        assert r0 < c and abs(value) / 2.0 > 40.0
        T[:c, c:] = np.clip(np.round(rng.standard_normal((c, d - c)) * 2.0), -6.0, 6.0)
        T[:c, :c] = 2.0 * np.eye(c)
        T[r0, c] = value
    col = np.abs(T[c:, c])
    assert np.array_equal(np.flatnonzero(col == col.max()) + c, [r1, r2])
    return T


def _place(c, r):
    o = r - c
    return dict(stride=o // 256, wave=(o % 256) // 64, lane=o % 64, thread=o % 256)


TIES = {  # name: (c, r1, r2)
    "lanes_of_one_wave": (0, 70, 100), "lanes_of_one_wave_c37": (37, 37 + 70, 37 + 100),
    "waves_same_stride": (0, 10, 200), "waves_same_stride_c37": (37, 37 + 10, 37 + 200),
    "wave3_stride0_vs_thread0_stride1": (0, 250, 256), "wave3_stride0_vs_thread0_stride1_c37": (37, 37 + 250, 37 + 256),
    "stride1_vs_stride2": (0, 300, 520), "stride1_vs_stride2_c37": (37, 37 + 300, 37 + 520),
    "one_thread_stride0_vs_stride1": (0, 5, 261), "diagonal_vs_last_row": (0, 0, 599),
    "larger_value_above_the_diagonal_c37": (37, 37 + 250, 37 + 256),
}
ABOVE = {"larger_value_above_the_diagonal_c37": (5, -1000.0)}      # row 5 < c = 37: 500 in column 37 at step 37, against the tie of 40s below


def _check_placement(name, c, r1, r2):
    a, b = _place(c, r1), _place(c, r2)
    if name.startswith("lanes_of_one_wave"):
        assert a["stride"] == b["stride"] == 0 and a["wave"] == b["wave"] and a["lane"] != b["lane"]
    elif name.startswith("waves_same_stride"):
        assert a["stride"] == b["stride"] == 0 and a["wave"] != b["wave"]
    elif name.startswith("wave3_stride0"):
        assert (a["stride"], a["wave"]) == (0, 3) and (b["stride"], b["thread"]) == (1, 0)
    elif name.startswith("stride1_vs_stride2"):
        assert a["stride"] == 1 and b["stride"] == 2 and a["thread"] != b["thread"]
    elif name == "one_thread_stride0_vs_stride1":
        assert a["thread"] == b["thread"] and (a["stride"], b["stride"]) == (0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TIES))
def test_pivot_ties_across_lanes_waves_and_strides(name):
    c, r1, r2 = TIES[name]
    _check_placement(name, c, r1, r2)
    T = _tie_matrix(c, r1, r2, seed=len(name), above=ABOVE.get(name))
    want = _orc_inv(T)
    assert np.isfinite(want).all()
    assert _same(mcmc_amd.mat_inverse(T), want)


def _negative_zero_last_pivot(d, seed, zero):
    """The LAST pivot is `zero` (+0.0 or -0.0) and its sign shows in the result: column d - 1 is zero, row d - 1 holds one entry (2, under the decoupled
    M[0][0] = 4), so step 0 leaves Ainv[d-1][0] = -0.5 and M[d-1][d-1] = zero - 2 * 0 keeps its sign; the steps between skip the row (f == 0); the last
    one divides (-0.5, 0, ..., 1) by the pivot: +-inf at both ends.  (A signed-zero pivot at an earlier step leaves 0 / 0 = NaN in its row, which the
    later steps spread over the whole row -- nothing of the sign survives.)"""
    Z = _spd(d, seed)
    Z[0, :] = 0.0; Z[:, 0] = 0.0; Z[0, 0] = 4.0
    Z[d - 1, :] = 0.0; Z[:, d - 1] = 0.0; Z[d - 1, 0] = 2.0; Z[d - 1, d - 1] = zero
    return Z


def _nan_inf_zero_cases(d=600):
    """(name, matrix) for INV at d = 600: what must never win, what must stay, ties of infinities and of zeros"""
    out = []
    # NaN below the diagonal in second / third-stride rows: never wins; its row is NaN from then on.  The columns of those rows are zero off the
    # diagonal, so that the NaN rows -- pivot rows at their own steps -- touch nobody else (f == 0) and the other rows stay finite and comparable
    N = _spd(d, 21)
    for r, c in ((300, 0), (400, 3), (599, 2)):
        N[:r, r] = 0.0; N[r + 1:, r] = 0.0; N[r, c] = np.nan
    out.append(("nan_below_in_later_strides", N))
    # NaN ON the diagonal, larger finite values in the later strides: the diagonal stays, rows 5, 305, 560 turn NaN (decoupled as above), the rest stays finite
    N2 = _spd(d, 22)
    N2[:, [5, 305, 560]] = 0.0
    N2[5, 5] = np.nan; N2[305, 5] = 100.0; N2[560, 5] = -200.0; N2[305, 305] = 1.0; N2[560, 560] = 1.0
    out.append(("nan_on_the_diagonal_larger_values_later", N2))
    # +inf and -inf tie in magnitude.  Whichever wins, the other row is f * 0 = NaN from then on and becomes a pivot row later: the oracle's output is NaN
    # throughout, and so must the device's be -- the case checks that the search terminates on them and nothing finite is invented
    for k, (r1, r2) in enumerate([(250, 256), (300, 520), (70, 100)]):
        I = _spd(d, 23 + k); I[r1, 0] = np.inf; I[r2, 0] = -np.inf
        out.append((f"inf_tie_{r1}_{r2}", I))
    Z = _spd(d, 27); Z[:, 300] = 0.0; Z[300, :] = 0.0; Z[:, 599] = 0.0; Z[599, :] = 0.0      # columns that are zero from the diagonal down: every candidate ties at 0, the diagonal (0 / 0) is taken
    out.append(("zero_columns", Z))
    Z0 = _spd(d, 28); Z0[:, 0] = 0.0                                                 # ... at c = 0, with three strides of zeros
    out.append(("zero_column_0", Z0))
    Zp = _negative_zero_last_pivot(d, 29, 0.0)
    Zm = _negative_zero_last_pivot(d, 29, -0.0)
    assert np.array_equal(Zp, Zm) and not _same(_orc_inv(Zm), _orc_inv(Zp))          # the sign of the zero shows in the oracle's output
    out.append(("negative_zero_pivot", Zm))
    # -0.0 candidates in other lanes, waves and strides (offsets 10, 256, 299 from c = 300) tie with the +0.0 diagonal: the diagonal stays (any of those
    # rows as the pivot row would be divided by -0.0 into infinities)
    Zn = _spd(d, 30); Zn[:, 300] = 0.0; Zn[300, :] = 0.0; Zn[310, 300] = -0.0; Zn[556, 300] = -0.0; Zn[599, 300] = -0.0
    out.append(("negative_zero_candidates_below", Zn))
    Zt = np.clip(np.round(np.random.default_rng(31).standard_normal((d, d)) * 2.0), -6.0, 6.0) + np.eye(d) * 3      # integers: many exact ties and exact zeros in every column
    out.append(("integer_matrix", Zt))
    return out


@pytest.mark.gpu
def test_nan_inf_and_zero_pivot_candidates_across_strides():
    for name, M in _nan_inf_zero_cases():
        want = _orc_inv(M)
        if not name.startswith("inf_tie"):
            assert (~np.isnan(want)).mean() > 0.99, name     # the comparison still has something to compare
        assert _same(mcmc_amd.mat_inverse(M), want), name


# ---- CHOL_LOWER beyond one stride (d = 600)

def _chol_cases(d=600):
    out = []
    for k in (300, 599):                     # SPD made non-positive at ONE late pivot: the oracle's output is NaN from (k, k) on and finite before
        M = _spd(d, 40 + k)
        L = _orc_chol(M)
        M[k, k] -= 1.5 * L[k, k] * L[k, k]
        Lo = _orc_chol(M)
        assert np.isnan(Lo[k, k]) and not np.isnan(Lo[:, :k]).any() and not np.isnan(Lo[:k]).any(), k
        out.append((f"non_positive_pivot_{k}", M))
    # an exactly zero pivot: A = L0 L0' in small integers (every operation of the factorisation is exact and returns L0), then A[k][k] lowered by L0[k][k]^2
    rng = np.random.default_rng(44)
    L0 = np.tril(np.clip(np.round(rng.standard_normal((d, d))), -2.0, 2.0), -1) + np.diag(rng.integers(1, 4, d).astype(float))
    A = L0 @ L0.T
    assert np.array_equal(_orc_chol(A), L0)
    k = 300
    A[k, k] -= L0[k, k] ** 2
    Lo = _orc_chol(A)
    assert Lo[k, k] == 0.0 and np.isnan(Lo[k + 1:, k]).any() and np.isinf(Lo[k + 1:, k]).any() and np.array_equal(Lo[:, :k], L0[:, :k])      # 0 / 0 and x / 0 below it
    out.append(("zero_pivot_300", A))
    # NaN and garbage in the strict upper triangle: CHOL_LOWER reads the lower triangle only -- the oracle too (checked here first)
    M = _spd(d, 45)
    U = M.copy()
    iu = np.triu_indices(d, 1)
    U[iu] = rng.standard_normal(iu[0].size) * 1e6
    U[0, 1] = np.nan; U[299, 300] = np.nan; U[10, 599] = np.inf; U[598, 599] = -np.inf
    assert _same(_orc_chol(U), _orc_chol(M))
    out.append(("garbage_above_the_diagonal", U))
    return out


@pytest.mark.gpu
def test_cholesky_late_non_positive_and_zero_pivots_and_an_ignored_upper_triangle():
    for name, M in _chol_cases():
        assert _same(mcmc_amd.mat_cholesky_lower(M), _orc_chol(M)), name


# ---- beyond the staging budget: the host loops (the test hook lowers the budget, so that d of a few hundred runs what d > 3 840 / 7 680 runs)

@contextlib.contextmanager
def _stage_bytes(n):
    mcmc_amd.test_set_linalg_stage_bytes(n)
    try:
        yield
    finally:
        mcmc_amd.test_set_linalg_stage_bytes(0)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [130, 300, 600])
def test_beyond_the_staging_budget_spd_and_ill_conditioned(d):
    """1 024 bytes: INV needs 16 d, CHOL_LOWER 8 d -- both beyond it from d = 129 on.  The same calls with the real budget run the device kernels and
    return the same bits (results do not depend on the hook; the memo is emptied when it moves, which the count of computed factorisations shows)."""
    M, P = _spd(d, 3 * d), _spd(d, 5 * d, 1e4)
    assert (np.abs(P).argmax(axis=0) != np.arange(d)).any()
    want = [_orc_inv(M), _orc_chol(M), _orc_inv(P), _orc_chol(P)]
    run = lambda: [mcmc_amd.mat_inverse(M), mcmc_amd.mat_cholesky_lower(M), mcmc_amd.mat_inverse(P), mcmc_amd.mat_cholesky_lower(P)]
    n0, v0 = mcmc_amd.test_linalg_computed(), mcmc_amd.test_linalg_computed_on_device()
    with _stage_bytes(1024):
        host = run()
    n1, v1 = mcmc_amd.test_linalg_computed(), mcmc_amd.test_linalg_computed_on_device()
    dev = run()
    n2, v2 = mcmc_amd.test_linalg_computed(), mcmc_amd.test_linalg_computed_on_device()
    assert (n1 - n0, n2 - n1) == (4, 4)                         # nothing of the other setting came back from the memo
    assert (v1 - v0, v2 - v1) == (0, 4)                         # ... the host loops under the hook, the device kernels without it
    for h, g, w in zip(host, dev, want):
        assert _same(h, w) and _same(g, w)


@pytest.mark.gpu
def test_the_staging_budget_is_inclusive_and_counted_per_operation():
    """2 080 bytes: INV (16 d bytes) fits up to d = 130 and CHOL_LOWER (8 d) up to d = 260, exactly as d = 3 840 / 7 680 fit the real 61 440 -- the
    matrix that fills the budget runs the device kernels, one dimension more the host loops; the same bits on both sides"""
    with _stage_bytes(2080):
        for fn, ref, d_fits in ((mcmc_amd.mat_inverse, _orc_inv, 130), (mcmc_amd.mat_cholesky_lower, _orc_chol, 260)):
            for d, on_device in ((d_fits, 1), (d_fits + 1, 0)):
                M = _spd(d, 9 * d)
                n0, v0 = mcmc_amd.test_linalg_computed(), mcmc_amd.test_linalg_computed_on_device()
                assert _same(fn(M), ref(M)), (fn.__name__, d)
                assert (mcmc_amd.test_linalg_computed() - n0, mcmc_amd.test_linalg_computed_on_device() - v0) == (1, on_device), (fn.__name__, d)


@pytest.mark.gpu
def test_beyond_the_staging_budget_pivot_ties_nan_and_singular_input():
    """the battery of test_general_matrices_pivot_ties_nan_and_singular_input (d = 130), the d = 600 batteries above and tie placements, on the host loops"""
    rng = np.random.default_rng(5)
    d = 130
    G = rng.standard_normal((d, d))
    T = np.round(rng.standard_normal((d, d)) * 2.0) + np.eye(d) * 3
    N = _spd(d, 11); N[40, 3] = np.nan
    N2 = _spd(d, 12); N2[5, 5] = np.nan
    S = _spd(d, 13); S[:, 9] = 0.0; S[9, :] = 0.0
    Q = -_spd(d, 14)
    with _stage_bytes(1024):
        for name, M in [("G", G), ("T", T), ("N", N), ("N2", N2), ("S", S)] + _nan_inf_zero_cases():
            assert _same(mcmc_amd.mat_inverse(M), _orc_inv(M)), name
        for name in ("wave3_stride0_vs_thread0_stride1", "stride1_vs_stride2_c37"):
            c, r1, r2 = TIES[name]
            M = _tie_matrix(c, r1, r2, seed=len(name))
            assert _same(mcmc_amd.mat_inverse(M), _orc_inv(M)), name
        assert _same(mcmc_amd.mat_cholesky_lower(Q), _orc_chol(Q)) and np.isnan(mcmc_amd.mat_cholesky_lower(Q)).any()
        for name, M in _chol_cases():
            assert _same(mcmc_amd.mat_cholesky_lower(M), _orc_chol(M)), name


# ---- the routing edge through the samplers: hmc / mala with a dense precond_mat beyond d = 512 ride the matrix-product route while INV(M) runs on the
# device; a matrix beyond the staging budget stays on the literal kernel (whose preparation calls the same INV: the host loops).  d = 520 needs 8 320 bytes.

from test_gpu_parity_gemm_dense_m import ALGO, MIXED, _problem, dense_mass      # noqa: E402  (the shapes of that file)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["hmc", "mala"])
@pytest.mark.parametrize("target", ["dense", "logit"])
def test_routing_edge_a_dense_precond_mat_beyond_the_budget_runs_on_the_literal_kernel(algo, target):
    d, N, C, burn, keep = 520, 64, 33, 2, 4
    kind, tkw, spec, init = _problem(target, d, N, C)
    M = dense_mass(d, d + 1)
    eps = MIXED[(target, algo)]
    st = mcmc_amd.default_settings(rng_seed_value=7, n_burnin_draws=burn, n_keep_draws=keep, n_leap_steps=3, step_size=eps, precond_mat=M)
    s = orc.make_settings(seed=7, n_burnin=burn, n_keep=keep, n_leap=3, step=eps, W=4, hoist=1, precond=M)
    o_draws, o = orc.run_many(ALGO[algo], spec, init, s)
    print(f"{algo} {target}: oracle accepts {int(o['n_accept'].sum())} of {keep * C} kept draws")
    assert 0 < o["n_accept"].sum() < keep * C <= 6 * C           # accepts AND rejects among the kept draws (n_accept counts those)
    with _stage_bytes(8192):
        l_draws, l = mcmc_amd.sample(algo, kind, init, st, **tkw)
        kern = mcmc_amd.last_kernel()
    assert kern.startswith("literal_kernel<"), kern
    assert np.array_equal(l["n_accept"], o["n_accept"]) and np.array_equal(l_draws, o_draws) and np.array_equal(l["theta"], o_draws[-1])
    g_draws, g = mcmc_amd.sample(algo, kind, init, st, **tkw)
    kern = mcmc_amd.last_kernel()
    assert kern.startswith("gemm_step_kernel<") and "dense precond_mat" in kern, kern
    assert np.array_equal(g["n_accept"], o["n_accept"]) and np.array_equal(g_draws, o_draws) and np.array_equal(g["theta"], o_draws[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["nuts", "rwmh"])
def test_routing_edge_nuts_and_rwmh_with_a_matrix_beyond_the_budget(algo):
    """their dense precond_mat / cov_mat beyond d = 512 is the literal kernel's either way; what moves is where its preparation factorises.  d = 520:
    INV stages 8 320 bytes, CHOL_LOWER 4 160 -- at 8 192 INV alone runs the host loops, at 4 096 both do (nothing on the device), at 0 neither"""
    d, C = 520, 6
    kind, tkw, spec, init = _problem("dense", d, 0, C)
    M = dense_mass(d, d + 1)
    eps = 0.05 if algo == "nuts" else 0.01
    st = mcmc_amd.default_settings(rng_seed_value=3, n_burnin_draws=1, n_keep_draws=3, step_size=eps, n_adapt_draws=0, max_tree_depth=3, precond_mat=M)
    s = orc.make_settings(seed=3, n_burnin=1, n_keep=3, step=eps, n_adapt=0, max_depth=3, W=4, hoist=1, precond=M)
    o_draws, o = orc.run_many(orc.ALGO_NUTS if algo == "nuts" else orc.ALGO_RWMH, spec, init, s)
    assert np.all(np.isfinite(o_draws)) and o["n_accept"].sum() > 0
    for budget in (8192, 4096, 0):
        with _stage_bytes(budget):                               # (every change of the budget empties the memo: each pass factorises anew)
            n0, v0 = mcmc_amd.test_linalg_computed(), mcmc_amd.test_linalg_computed_on_device()
            g_draws, g = mcmc_amd.sample(algo, kind, init, st, **tkw)
            kern = mcmc_amd.last_kernel()
            n, v = mcmc_amd.test_linalg_computed() - n0, mcmc_amd.test_linalg_computed_on_device() - v0
        assert kern.startswith("literal_kernel<"), kern
        assert np.array_equal(g["n_accept"], o["n_accept"]) and np.array_equal(g_draws, o_draws), budget
        print(f"{algo}, budget {budget}: {n} factorisations computed, {v} of them on the device")
        assert n > 0 and (v == 0 if budget == 4096 else v == n if budget == 0 else 0 < v < n), (budget, n, v)


# ---- the memo: two entries per thread and per operation, keyed by the whole matrix, the entry NOT used last is replaced

@pytest.mark.gpu
@pytest.mark.parametrize("op", ["inverse", "cholesky_lower"])
def test_memo_sequences_hits_and_evictions(op):
    fn, ref = (mcmc_amd.mat_inverse, _orc_inv) if op == "inverse" else (mcmc_amd.mat_cholesky_lower, _orc_chol)
    d = 96
    mats = {k: _spd(d, 60 + i) for i, k in enumerate("ABCDEF")}
    want = {k: ref(m) for k, m in mats.items()}
    assert all(not np.array_equal(want[a], want[b]) for a in mats for b in mats if a < b)
    mcmc_amd.release_workspace()
    # A B A C B A D A, then E F E A: computed (not a hit) exactly where the matrix is new or its entry was the one not used last when another came in --
    # C replaces B (A was used last), B then replaces A, A replaces C, D replaces B and A is still there, ...
    order    = "A B A C B A D A E F E A".split()
    computed = [1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 0, 1]
    for i, (k, c) in enumerate(zip(order, computed)):
        n0 = mcmc_amd.test_linalg_computed()
        assert _same(fn(mats[k]), want[k]), (i, k)
        assert mcmc_amd.test_linalg_computed() - n0 == c, (i, k)


@pytest.mark.gpu
def test_memo_keys_near_misses_nan_and_release():
    d = 96
    A = _spd(d, 70)
    B = A.copy(); B[50, 17] = np.nextafter(B[50, 17], np.inf)              # one element, one ulp
    for M in (A, B, A, B):
        assert _same(mcmc_amd.mat_inverse(M), _orc_inv(M)) and _same(mcmc_amd.mat_cholesky_lower(M), _orc_chol(M))
    assert not np.array_equal(_orc_inv(A), _orc_inv(B))
    Zp, Zm = _negative_zero_last_pivot(d, 71, 0.0), _negative_zero_last_pivot(d, 71, -0.0)                                      # the sign of one zero (== compares them equal; the key is the bytes)
    assert np.array_equal(Zp, Zm) and not _same(_orc_inv(Zp), _orc_inv(Zm))
    for M in (Zp, Zm, Zp, Zm):
        assert _same(mcmc_amd.mat_inverse(M), _orc_inv(M))
    N = _spd(d, 72); N[40, 3] = np.nan                                    # a NaN in the key (NaN != NaN; the bytes are equal): twice, the second from the memo
    n0 = mcmc_amd.test_linalg_computed()
    for _ in range(2):
        assert _same(mcmc_amd.mat_inverse(N), _orc_inv(N))
    assert mcmc_amd.test_linalg_computed() - n0 == 1
    mcmc_amd.release_workspace(all_streams=True)                          # empties the memo: computed again, and still right
    assert _same(mcmc_amd.mat_inverse(N), _orc_inv(N)) and _same(mcmc_amd.mat_inverse(A), _orc_inv(A))
    assert mcmc_amd.test_linalg_computed() - n0 == 3


@pytest.mark.gpu
def test_mala_runs_continued_alternately_with_two_masses():
    """mala asks for INV(M) and INV(eps^2 M) per call; two runs with different masses, each cut into two calls and interleaved, push four matrices through
    the two entries: every piece equals the run in one piece (the shape of test_dense_precond_mat_continues_a_run)"""
    d, C = 520, 33
    kind, tkw, _, init = _problem("dense", d, 0, C)
    Ms = [dense_mass(d, d + 1), dense_mass(d, d + 2)]
    S = lambda M, keep: mcmc_amd.default_settings(rng_seed_value=8, n_burnin_draws=0, n_keep_draws=keep, n_leap_steps=3, step_size=MIXED[("dense", "mala")], precond_mat=M)
    whole = [mcmc_amd.sample("mala", kind, init, S(M, 6), **tkw) for M in Ms]
    assert "dense precond_mat" in mcmc_amd.last_kernel()
    assert not np.array_equal(whole[0][0], whole[1][0])
    first = [mcmc_amd.sample("mala", kind, init, S(M, 2), **tkw) for M in Ms]
    second = [mcmc_amd.sample("mala", kind, np.ascontiguousarray(first[i][1]["theta"].T), S(M, 4), draw0=2, **tkw) for i, M in enumerate(Ms)]
    for i in range(2):
        assert 0 < whole[i][1]["n_accept"].sum()
        assert np.array_equal(whole[i][0], np.concatenate([first[i][0], second[i][0]]))
        assert np.array_equal(whole[i][1]["n_accept"], first[i][1]["n_accept"] + second[i][1]["n_accept"])
