"""CPU: mcmc_amd/covariance.py, the numpy statement of mi_mcmc_draws_covariance's definition (include/mi_mcmc.h), is tied to exact arithmetic here, so
that "device == mirror bit for bit" (tests/test_gpu_draws_cov.py) plus "mirror within derived bounds of exact" is the whole accuracy argument.

 - plan() gives the header's G, seg, T, P, KC, n_chunks on a table derived by hand below (every shape of the GPU tests is in it).
 - On the well-behaved inputs of the GPU tests the mirror (dot = the oracle's fma chain) stays inside the bounds of tests/test_gpu_draws_cov.py against
   a two-pass np.longdouble reference.
 - On hard inputs -- a mean 1e8 to 3e14 spreads away, scales over 300 decades -- it stays inside the EXTENDED bound (derivation at the test).
 - The mirror tells orders apart: its bits differ from the fma-free dot, from one unchunked chain, and (three chunks or more) from the chunk partials
   added in descending order.
 - A NaN and a +inf sample reach their own mean, row and column and nothing else."""
import functools

import numpy as np
import pytest

import draws_cov_cases as cases
from mcmc_amd import covariance

ALL_SHAPES = cases.SHAPES + cases.NEW_SHAPES

# (n_keep, d, C): (K, G, seg, T, P, KC, n_chunks), by hand from the header's rules
#   G0 = min(max(1, 4096 // d), ceil(K / 4096)); seg = 256 ceil(ceil(K / G0) / 256); G = ceil(K / seg)
#   T = ceil(d / 128); P = T (T + 1) / 2; n = max(1, 1024 // P); KC = max(512, 16 ceil(ceil(K / n) / 16)); n_chunks = ceil(K / KC)
PLAN_TABLE = {
    (1, 5, 2): (2, 1, 256, 1, 1, 512, 1),                 # G0 = min(819, 1); ceil(2 / 1024) = 1 -> 16 -> the floor 512
    (1, 130, 333): (333, 1, 512, 2, 3, 512, 1),           # 333 -> two lanes-rounds of 256; n = 341
    (3, 130, 333): (999, 1, 1024, 2, 3, 512, 2),          # ceil(999 / 341) = 3 -> 16 -> 512; 999 = 512 + 487
    (7, 17, 1001): (7007, 2, 3584, 1, 1, 512, 14),        # G0 = min(240, 2); ceil(7007 / 2) = 3504 -> 14 * 256; 7007 = 13 * 512 + 351
    (1, 200, 20000): (20000, 5, 4096, 2, 3, 512, 40),     # G0 = min(20, 5); 4000 -> 16 * 256; 4 * 4096 < 20000; ceil(20000 / 341) = 59 -> 64 -> 512
    (2, 1, 4097): (8194, 3, 2816, 1, 1, 512, 17),         # G0 = min(4096, 3); ceil(8194 / 3) = 2732 -> 11 * 256; 8194 = 16 * 512 + 2
    (2, 300, 401): (802, 1, 1024, 3, 6, 512, 2),          # n = 170; 802 = 512 + 290
    (1, 385, 77): (77, 1, 256, 4, 10, 512, 1),
    (40, 3, 7): (280, 1, 512, 1, 1, 512, 1),
    (600, 2, 1): (600, 1, 768, 1, 1, 512, 2),
    (1, 3, 5000): (5000, 2, 2560, 1, 1, 512, 10),         # G0 = min(1365, 2); 2500 -> 10 * 256; 5000 = 9 * 512 + 392
    (1, 520, 512): (512, 1, 512, 5, 15, 512, 1),          # n = 68
    (1, 2, 600000): (600000, 147, 4096, 1, 1, 592, 1014),  # G0 = min(2048, 147); ceil(600000 / 147) = 4082 -> 4096; 146 * 4096 < 600000;
                                                          # ceil(600000 / 1024) = 586 -> 37 * 16 = 592; 1013 * 592 = 599696
    (1, 24, 200): (200, 1, 256, 1, 1, 512, 1),            # the dense mass adaptation's starting states
    (1, 130, 3000): (3000, 1, 3072, 2, 3, 512, 6),
    (1, 520, 2000): (2000, 1, 2048, 5, 15, 512, 4),       # ceil(2000 / 68) = 30 -> 32 -> 512
    (50, 520, 2000): (100000, 7, 14336, 5, 15, 1472, 68),  # G0 = min(7, 25): d limits the groups; ceil(1e5 / 7) = 14286 -> 56 * 256; 6 * 14336 < 1e5;
                                                          # ceil(1e5 / 68) = 1471 -> 92 * 16 = 1472; 67 * 1472 = 98624
    (1, 1, 1000000): (1000000, 245, 4096, 1, 1, 992, 1009),  # ceil(1e6 / 4096) = 245; 4082 -> 4096; ceil(1e6 / 1024) = 977 -> 62 * 16; 1008 * 992 = 999936
    (1, 5000, 3): (3, 1, 256, 40, 820, 512, 1),           # 4096 // d = 0 -> 1; n = 1024 // 820 = 1
    (1, 6000, 9000): (9000, 1, 9216, 47, 1128, 9008, 1),  # P > 1024: n = max(1, 0) = 1; KC = 16 ceil(9000 / 16) = 9008: one chunk
}


def test_plan_is_the_headers_rule_on_a_table_derived_by_hand():
    for s in ALL_SHAPES:
        assert s in PLAN_TABLE, s
    for s, want in PLAN_TABLE.items():
        p = covariance.plan(*s)
        assert (p["K"], p["G"], p["seg"], p["T"], p["P"], p["KC"], p["n_chunks"]) == want, (s, p, want)
        assert (p["G"] - 1) * p["seg"] < p["K"] <= p["G"] * p["seg"] and p["KC"] % 16 == 0 and (p["n_chunks"] - 1) * p["KC"] < p["K"]
    with pytest.raises(ValueError):
        covariance.plan(1, 3, 1)


def _exact(x, pairs=None):
    """two-pass np.longdouble reference of a slab: mu [d], e [d][K] (about mu), and cov -- [d][d], or the values at `pairs`.  Every row is first
    shifted by its own first sample (an exact subtraction of two doubles in the wider format wherever the spread is below 2^11 times the value, and
    what keeps the reference's own mean error out of e at |mean| / sd = 1e14)."""
    X = covariance.samples(x).astype(np.longdouble)
    d, K = X.shape
    x0 = X[:, :1]
    sh = X - x0
    m = sh.sum(axis=1) / K
    e = sh - m[:, None]
    mu = x0[:, 0] + m
    if pairs is None:
        return mu, e, (e @ e.T) / (K - 1)
    return mu, e, np.array([(e[i] * e[j]).sum() / (K - 1) for i, j in pairs])


def _bounds(x, e, pairs=None):
    """the bounds of tests/test_gpu_draws_cov.py: (K + 64) 2^-52 sum_k |e_ik e_jk| / (K - 1) and (K + 2) 2^-53 mean_k |x_ik|, sums in float64"""
    X = covariance.samples(x)
    K = X.shape[1]
    ea = np.abs(e).astype(np.float64)
    if pairs is None:
        cb = (K + 64) * 2.0 ** -52 * (ea @ ea.T) / (K - 1)
    else:
        cb = np.array([(K + 64) * 2.0 ** -52 * (ea[i] * ea[j]).sum() / (K - 1) for i, j in pairs])
    return cb, (K + 2) * 2.0 ** -53 * np.abs(X).mean(axis=1)


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_the_mirror_meets_the_gpu_tests_bounds_on_their_inputs(shape):
    x = cases.frozen_slab(shape)
    ref = cases.reference(shape)
    pairs = None if ref["cov"] is not None else list(ref["elements"])
    got = ref["cov"] if pairs is None else np.array(list(ref["elements"].values()))
    mu, e, exact = _exact(x, pairs)
    cb, mb = _bounds(x, e, pairs)
    rc = float((np.abs(got.astype(np.longdouble) - exact) / cb).max())
    rm = float((np.abs(ref["mean"].astype(np.longdouble) - mu) / mb).max())
    print(f"(n_keep, d, C) = {shape}: mirror worst |cov - exact| / bound {rc:.4f}, worst |mean - mu| / bound {rm:.4f}")
    assert np.isfinite(got).all() and np.isfinite(ref["mean"]).all()
    assert rc <= 1.0 and rm <= 1.0


HARD = [(1e8, -3, 3), (1e8, -6, 6), (-3e12, -2, 2), (0.0, -150, 150)]


@pytest.mark.parametrize("offset,lo,hi", HARD, ids=[f"offset{o:g}_scales1e{a}to1e{b}" for o, a, b in HARD])
def test_the_mirror_meets_the_extended_bound_on_hard_inputs(offset, lo, hi):
    """x_ik = scale_i N(0, 1) + offset, shape (3, 130, 333), full matrix.  The bound of the well-behaved inputs treats the mean's error as negligible;
    here it is not (at offset 1e8 the mirror alone exceeds that bound many times over).  DERIVATION of the bound asserted here: let the computed mean
    be mu' = mu + delta, |delta_i| <= mean_bound_i = (K + 2) 2^-53 mean_k |x_ik| (K - 1 additions and one division, each within 2^-53 relative of
    partial sums that sum_k |x_ik| bounds).  The kernel centres about mu', and exactly
        sum_k (e_ik - delta_i) (e_jk - delta_j) = sum_k e_ik e_jk + K delta_i delta_j          (the cross terms vanish: sum_k e_ik = 0)
    so the mean's error moves cov_ij by K / (K - 1) delta_i delta_j and by nothing at first order.  The rounding of the centring and of the fma chain
    is what cov_bound_ij = (K + 64) 2^-52 sum_k |e_ik e_jk| / (K - 1) already holds (twice gamma_K; the sum of magnitudes about mu and about mu' differ
    at relative order delta / sd, far inside the factor 2).  Hence
        |cov_ij - exact_ij| <= cov_bound_ij + K / (K - 1) mean_bound_i mean_bound_j."""
    shape = (3, 130, 333)
    n_keep, d, C = shape
    K = n_keep * C
    rng = np.random.default_rng(7)
    scale = np.logspace(lo, hi, d)
    X = scale[:, None] * rng.standard_normal((d, K)) + offset
    x = np.ascontiguousarray(X.reshape(d, n_keep, C).transpose(1, 0, 2))
    mean = covariance.mean_ref(x)
    cov = covariance.covariance_ref(x, math=cases.ORC_MATH)
    mu, e, exact = _exact(x)
    cb, mb = _bounds(x, e)
    ext = cb + K / (K - 1) * mb[:, None] * mb[None, :]
    err = np.abs(cov.astype(np.longdouble) - exact)
    rc, rm = float((err / ext).max()), float((np.abs(mean.astype(np.longdouble) - mu) / mb).max())
    print(f"offset {offset:g}, scales 1e{lo} .. 1e{hi}: mirror worst |cov - exact| / extended bound {rc:.4f} (against the plain bound: "
          f"{float((err / cb).max()):.3g}), worst |mean - mu| / bound {rm:.4f}")
    assert np.isfinite(cov).all() and np.isfinite(mean).all()
    assert rc <= 1.0 and rm <= 1.0
    assert np.array_equal(cov, cov.T)


def _pairs_of(shape):
    d = shape[1]
    if d > 200 or shape in cases.SAMPLED:
        return cases.sample_elements(d, seed=1, n_interior=24)
    return [(i, j) for i in range(d) for j in range(i + 1)]


@functools.lru_cache(maxsize=None)
def _order_shares(shape):
    """shares of the elements whose bits change when (a) the dot loses its fma, (b) the chunk partials are added in descending q, (c) the chunking is
    dropped (one chain over all K)"""
    x = cases.frozen_slab(shape)
    e = covariance.centred(x)
    K = e.shape[1]
    p = covariance.plan(*shape)
    bounds = covariance.chunk_bounds(K, p["KC"])
    assert len(bounds) == p["n_chunks"]
    fma, plain = cases.ORC_MATH["dot"], covariance.NUMPY_MATH["dot"]
    pairs = _pairs_of(shape)
    base = np.array([covariance.element(e[i], e[j], bounds, fma) for i, j in pairs])
    a = np.array([covariance.element(e[i], e[j], bounds, plain) for i, j in pairs])
    b = np.array([covariance.element(e[i], e[j], bounds[::-1], fma) for i, j in pairs])
    c = np.array([covariance.element(e[i], e[j], [(0, K)], fma) for i, j in pairs])
    n = len(pairs)
    shares = [float((cases.bits(v) != cases.bits(base)).sum()) / n for v in (a, b, c)]
    # (b'), for a shape with ONE element: the share of the cyclic merges q = s, s + 1, .., n - 1, 0, .., s - 1 (s = 1 .. n - 1) that change its bits
    rot = [covariance.element(e[0], e[0], bounds[s:] + bounds[:s], fma) for s in range(1, len(bounds))] if n == 1 else []
    shares.append(float(np.mean([cases.bits(v)[0] != cases.bits(base)[0] for v in rot])) if rot else None)
    return p["n_chunks"], n, shares


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=cases.shape_id)
def test_the_mirror_can_tell_orders_apart(shape):
    """Bit equality with the mirror means something only if another order gives other bits.  Two partials have ONE order of addition (from +0,
    (0 + a) + b = (0 + b) + a exactly), so the descending merge must equal the ascending one at two chunks and can differ from three on; what tells a
    two-chunk shape's merge apart is the unchunked chain.  (2, 1, 4097) has ONE element, and the 17 partials of this input happen to round to the
    same double when added downwards (measured here: so do 127 of 200 random orders of them); there the 16 cyclic merges stand in, and some must differ."""
    n_chunks, n, (no_fma, descending, unchunked, cyclic) = _order_shares(shape)
    print(f"(n_keep, d, C) = {shape}, {n_chunks} chunks, {n} elements: bits differ from the fma-free dot in {no_fma:.3f}, from the descending merge in "
          f"{descending:.3f}, from one unchunked chain in {unchunked:.3f}" + ("" if cyclic is None else f"; {cyclic:.3f} of the cyclic merges differ"))
    if n_chunks == 1:
        assert descending == 0.0 and unchunked == 0.0
    elif n_chunks == 2:
        assert no_fma > 0.0 and unchunked > 0.0 and descending == 0.0
    else:
        assert no_fma > 0.0 and unchunked > 0.0
        assert descending > 0.0 if n > 1 else descending + cyclic > 0.0


def test_non_finite_samples_reach_their_own_mean_row_and_column_only():
    shape = (3, 130, 333)
    ref = cases.reference(shape)
    x = np.array(cases.frozen_slab(shape))
    i_nan, i_inf = 7, 100
    x[1, i_nan, 5] = np.nan
    x[2, i_inf, 300] = np.inf
    got = cases.mirror(x)
    bad = np.zeros(shape[1], dtype=bool)
    bad[[i_nan, i_inf]] = True
    touched = bad[:, None] | bad[None, :]
    assert np.array_equal(~np.isfinite(got["mean"]), bad) and np.isnan(got["mean"][i_nan]) and got["mean"][i_inf] == np.inf
    assert np.array_equal(np.isnan(got["cov"]), touched)                 # inf - inf in the centring: the +inf row is NaN too
    assert np.array_equal(cases.bits(got["cov"])[~touched], cases.bits(ref["cov"])[~touched])
    assert np.array_equal(cases.bits(got["mean"])[~bad], cases.bits(ref["mean"])[~bad])


def test_restricted_elements_are_the_full_matrix_elements():
    shape = (3, 130, 333)
    ref = cases.reference(shape)
    pairs = cases.sample_elements(shape[1])
    assert {(i // 128, j // 128) for i, j in pairs} == {(0, 0), (1, 0), (1, 1)} and all(j <= i for i, j in pairs)
    assert {(0, 0), (127, 0), (127, 127), (128, 0), (129, 127), (128, 128), (129, 129), (129, 128)} <= set(pairs)
    got = covariance.covariance_ref(cases.frozen_slab(shape), math=cases.ORC_MATH, elements=pairs)
    assert list(got) == pairs
    assert all(cases.bits(got[p])[()] == cases.bits(ref["cov"][p])[()] for p in pairs)
    with pytest.raises(ValueError):
        covariance.covariance_ref(cases.frozen_slab(shape), elements=[(3, 5)])
