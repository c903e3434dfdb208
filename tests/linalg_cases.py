"""Matrices and references shared by the INV / CHOL_LOWER tests (tests/test_gpu_linalg.py on the device, tests/test_linalg_blockdiag_cpu.py on the
oracle alone): the oracle's orc_inv / orc_chol_lower, the bitwise comparison, SPD and pivoting blocks, block-diagonal assembly and the per-block
reference that stands in for the oracle where the whole matrix would cost it minutes (d = 3 840: 2 d^3 operations on one core)."""
import ctypes as C

import numpy as np

import orc


def orc_inv(A):
    d = A.shape[0]
    out = np.empty((d, d))
    orc.lib().orc_inv(orc._p(np.ascontiguousarray(A)), C.c_size_t(d), orc._p(out))
    return out


def orc_chol(A):
    d = A.shape[0]
    out = np.empty((d, d))
    orc.lib().orc_chol_lower(orc._p(np.ascontiguousarray(A)), C.c_size_t(d), orc._p(out))
    return out


def spd(d, seed, cond=None):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    M = A @ A.T + np.diag(rng.uniform(0.3, 3.0, d))
    if cond is not None:                     # D M D with D log-spaced: still SPD, condition number ~ cond^2 x M's
        D = np.logspace(0.0, -np.log10(cond), d)
        rng.shuffle(D)
        M = D[:, None] * M * D[None, :]
    return M


def same(a, b):
    """bit for bit, signed zeros included; NaN equals NaN (its sign / payload is the hardware's, x86 and gfx950 differ, and nothing reads it)"""
    fin = ~np.isnan(a)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[fin]), np.signbit(b[fin]))


def pivoting_block(n, seed):
    """A general (non-symmetric) n x n block whose elimination swaps rows at most steps and whose pivots are all POSITIVE: a strictly
    column-diagonally-dominant matrix with a positive diagonal, its rows permuted.  Column dominance survives every elimination step (the Schur
    complement of such a matrix is one again, and its diagonal stays positive), so step c picks the row that holds the original diagonal entry
    of column c.  Positive pivots matter for the block-diagonal property below: the zeros outside the block stay +0.0 when divided by them."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    np.fill_diagonal(G, 0.0)
    G[np.diag_indices(n)] = np.abs(G).sum(axis=0) + rng.uniform(0.5, 2.0, n)
    return np.ascontiguousarray(G[rng.permutation(n)])


def block_sizes(d, pattern=(127, 128, 129, 300)):
    """the pattern repeated while it fits, one ragged block for what is left"""
    sizes, i = [], 0
    while sum(sizes) + pattern[i % len(pattern)] <= d:
        sizes.append(pattern[i % len(pattern)]); i += 1
    if sum(sizes) < d:
        sizes.append(d - sum(sizes))
    return sizes


def block_diag(blocks):
    d = sum(b.shape[0] for b in blocks)
    M = np.zeros((d, d))
    o = 0
    for b in blocks:
        n = b.shape[0]
        M[o:o + n, o:o + n] = b
        o += n
    return M


def blockwise(fn, blocks):
    """block-diagonal of fn(block): the reference of fn(block_diag(blocks)) that tests/test_linalg_blockdiag_cpu.py shows to be the oracle's bits"""
    return block_diag([fn(b) for b in blocks])
