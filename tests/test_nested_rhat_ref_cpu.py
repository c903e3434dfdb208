"""No GPU: mcmc_amd/nested_rhat.py, the numpy statement of mi_mcmc_draw_stats_nested (include/mi_mcmc.h), against exact arithmetic.

EXACT INPUTS.  Where every operation is exact -- N, M, K powers of two and x = (N - 1)(M - 1)(K - 1) times small integers, so that the three divisions by
n - 1 are exact too -- mean, between, within and super_mean ARE the rationals (fractions.Fraction), and nrhat, mcse_mean their correctly rounded roots.

DERIVED BOUNDS, against a two-pass computation in np.longdouble, every dimension of every case.  u = 2^-53.  A value that passes through p additions
and one division carries a relative error of at most (p + 1) u to first order; a SUM64 of n elements has depth(n) = ceil(n / 64) - 1 + 6 additions
(the addition to +0.0 is exact), a sequential sum of N draws N - 1.  All bounds below are TWICE the first-order ones (u2 = 2^-52 in place of u), which
covers the second-order terms.  With bars for exact values:
  a (chain mean)           err_a    <= N u2 mean_t |x|
  A_k (superchain mean)    err_A    <= (N + depth(M) + 1) u2 mean_{t,m} |x|
  mean                     err_mean <= (N + depth(M) + depth(K) + 2) u2 mean_{t,c} |x|
  a sum of squared deviations sum_j (y_j - c)^2 / (n - 1) of computed y_j, c with errors err_y_j, err_c, summed with p additions:
      eta_j = err_y_j + err_c + u2 |ybar_j - cbar|                              (the two inputs' errors and the subtraction's rounding)
      err  <= [sum_j eta_j (2 |ybar_j - cbar| + eta_j) + (p + 3) u2 sum_j (ybar_j - cbar)^2] / (n - 1)       (square, sum, division)
  v, Bt_k, between         that rule over the draws (p = N - 1), the members (p = depth(M)) and the superchains (p = depth(K))
  Wt_k = SUM64(v) / M      err <= mean_m err_v + (depth(M) + 1) u2 Wtbar_k;    w_k: err_Bt + err_Wt + u2 wbar_k
  within                   err <= mean_k err_w + (depth(K) + 1) u2 withinbar
  nrhat = sqrt(1 + b / w)  err <= (err_b / wbar + bbar err_w / wbar^2) / (2 nrhatbar) + 3 u2 nrhatbar
  mcse_mean = sqrt(b / K)  err <= err_b / (2 sqrt(K bbar)) + 2 u2 mcsebar
These are a few 1e-16 relative for mean and within, and grow for between only as far as the offsets of the dimensions cancel (|mean| / sd of the
superchain means ~ 100 here: <= 1e-12 relative), while one member read twice or one superchain mislabelled moves between and within by percents.

M = 1 IDENTITY.  nrhat^2 = Rhat^2 + 1 / N with Rhat^2 = (N - 1) / N + B / W of a plain two-pass numpy computation, to twice 2 nrhat err_nrhat (numpy's own
sums are no deeper than the mirror's) + 8 u2 nrhat^2.

SENSITIVITY.  Bit equality with the mirror means something only if another order gives other bits: four wrong mirrors are counted on the listed shapes.

STATISTICS.  For K superchains of M independent stationary members of variance s^2 and N = 1, between is (s^2 / M) chi^2_{K-1} / (K - 1) and within
estimates s^2 with K (M - 1) degrees of freedom, so (nrhat^2 - 1) M is a chi^2_{K-1} / (K - 1) variable up to within's relative error.  Its tails
by Wilson-Hilferty give the bounds used below; offsets of unit variance per superchain move nrhat^2 - 1 from about 1 / M to about 1 + 1 / M."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import draws_nested_cases as cases
from mcmc_amd import nested_rhat as NR

U2 = 2.0 ** -52
LD = np.longdouble


def _depth(n):
    return (n + 63) // 64 - 1 + 6


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# exact inputs


def _exact_rationals(x, M):
    N, d, C = x.shape
    K = C // M
    out = dict(mean=[], between=[], within=[], super_mean=[])
    for i in range(d):
        col = [[Fraction(float(x[t, i, c])) for t in range(N)] for c in range(C)]
        a = [sum(v) / N for v in col]
        var = [sum((y - m) ** 2 for y in v) / (N - 1) if N > 1 else Fraction(0) for v, m in zip(col, a)]
        A, w = [], []
        for k in range(K):
            am, vm = a[k * M:(k + 1) * M], var[k * M:(k + 1) * M]
            Ak = sum(am) / M
            Bt = sum((y - Ak) ** 2 for y in am) / (M - 1) if M > 1 else Fraction(0)
            A.append(Ak)
            w.append(Bt + sum(vm) / M)
        mean = sum(A) / K
        out["mean"].append(mean)
        out["between"].append(sum((y - mean) ** 2 for y in A) / (K - 1))
        out["within"].append(sum(w) / K)
        out["super_mean"].append(A)
    return out


@pytest.mark.parametrize("N,M,K", [(4, 4, 4), (4, 128, 64), (1, 4, 2), (2, 1, 4), (1, 64, 128)], ids=lambda v: str(v))
def test_on_exact_inputs_the_outputs_are_the_rationals(N, M, K):
    d = 2
    scale = max(N - 1, 1) * max(M - 1, 1) * (K - 1)
    rng = np.random.default_rng(N + 10 * M + 1000 * K)
    x = (scale * rng.integers(-8, 9, size=(N, d, K * M))).astype(np.float64)
    got = NR.nested_ref(x, M)
    want = _exact_rationals(x, M)
    for i in range(d):
        for name in ("mean", "between", "within"):
            assert Fraction(float(got[name][i])) == want[name][i], (name, i, got[name][i], float(want[name][i]))
        assert [Fraction(float(v)) for v in got["super_mean"][:, i]] == want["super_mean"][i]
        b, w = want["between"][i], want["within"][i]
        assert w > 0 and b >= 0
        # the roots: correctly rounded from exact operands wherever 1 + b / w and b / K are doubles themselves, which the next lines check
        r1, r2 = 1 + b / w, b / K
        if Fraction(float(r1)) == r1:
            assert got["nrhat"][i] == math.sqrt(float(r1))
        if Fraction(float(r2)) == r2:
            assert got["mcse_mean"][i] == math.sqrt(float(r2))
        assert abs(got["nrhat"][i] - math.sqrt(float(r1))) <= 4 * U2 * got["nrhat"][i]
        assert abs(got["mcse_mean"][i] - math.sqrt(float(r2))) <= 4 * U2 * got["mcse_mean"][i]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# derived bounds


def _sq_dev(ybar, cbar, err_y, err_c, p, n, axis):
    """(exact sum of squared deviations / (n - 1), its bound) along `axis` by the docstring's rule"""
    dev = np.abs(ybar - cbar)
    eta = err_y + err_c + U2 * dev
    s = (dev * dev).sum(axis=axis)
    return s / (n - 1), ((eta * (2 * dev + eta)).sum(axis=axis) + (p + 3) * U2 * s) / (n - 1)


def exact_with_bounds(x, M):
    """dict name -> (exact value in longdouble, bound) for every output of nested_ref"""
    N, d, C = x.shape
    K = C // M
    xl = np.asarray(x, dtype=LD).transpose(1, 2, 0).reshape(d, K, M, N)
    ax = np.abs(xl)
    a = xl.sum(axis=3) / N                                            # [d, K, M]
    err_a = N * U2 * ax.mean(axis=3)
    if N > 1:
        v, err_v = _sq_dev(xl, a[..., None], 0.0, err_a[..., None], N - 1, N, 3)
    else:
        v, err_v = np.zeros_like(a), np.zeros_like(a)
    A = a.sum(axis=2) / M                                             # [d, K]
    err_A = (N + _depth(M) + 1) * U2 * ax.mean(axis=(2, 3))
    if M > 1:
        Bt, err_Bt = _sq_dev(a, A[..., None], err_a, err_A[..., None], _depth(M), M, 2)
    else:
        Bt, err_Bt = np.zeros_like(A), np.zeros_like(A)
    Wt = v.sum(axis=2) / M
    err_Wt = err_v.mean(axis=2) + (_depth(M) + 1) * U2 * Wt
    w = Bt + Wt
    err_w = err_Bt + err_Wt + U2 * w
    mean = A.sum(axis=1) / K
    err_mean = (N + _depth(M) + _depth(K) + 2) * U2 * ax.mean(axis=(1, 2, 3))
    between, err_b = _sq_dev(A, mean[:, None], err_A, err_mean[:, None], _depth(K), K, 1)
    within = w.sum(axis=1) / K
    err_within = err_w.mean(axis=1) + (_depth(K) + 1) * U2 * within
    nrhat = np.sqrt(1 + between / within)
    err_nrhat = (err_b / within + between * err_within / within ** 2) / (2 * nrhat) + 3 * U2 * nrhat
    mcse = np.sqrt(between / K)
    err_mcse = err_b / (2 * np.sqrt(K * between)) + 2 * U2 * mcse
    return dict(mean=(mean, err_mean), between=(between, err_b), within=(within, err_within), nrhat=(nrhat, err_nrhat), mcse_mean=(mcse, err_mcse),
                super_mean=(A.T, err_A.T))


BOUND_SHAPES = [(1, 3, 128, 64), (17, 3, 195, 3), (130, 3, 126, 63), (2, 3, 390, 130), (3, 3, 65, 1), (17, 1, 4225, 65), (9, 3, 8320, 64)]


@pytest.mark.parametrize("shape", BOUND_SHAPES, ids=cases.shape_id)
def test_the_mirror_meets_the_derived_bounds_in_every_output(shape):
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than a double here: the exact reference needs the 80-bit format"
    x, got = cases.frozen_slab(shape), cases.reference(shape)
    ref = exact_with_bounds(x, shape[3])
    line = []
    for name in cases.OUTPUTS:
        exact, bound = ref[name]
        err = np.abs(got[name].astype(LD) - exact)
        line.append(f"{name} {float((err / bound).max()):.3f} (bound / |value| <= {float((bound / np.abs(exact)).max()):.1e})")
        assert np.isfinite(got[name]).all()
        assert (err <= bound).all(), (name, float((err / bound).max()))
    print(f"(N, d, C, M) = {shape}: worst |mirror - exact| / bound: " + ", ".join(line))


def test_with_one_chain_per_superchain_it_is_the_classic_rhat_plus_1_over_N():
    N, d, C = 17, 3, 65
    x = cases.slab(N, d, C, 1)
    got = NR.nested_ref(x, 1)
    m = x.mean(axis=0)
    W = x.var(axis=0, ddof=1).mean(axis=1)
    B = m.var(axis=1, ddof=1)
    rhat2 = (N - 1) / N + B / W
    _, err_nrhat = exact_with_bounds(x, 1)["nrhat"]
    bound = 2 * (2 * got["nrhat"] * err_nrhat.astype(np.float64)) + 8 * U2 * got["nrhat"] ** 2
    diff = np.abs(got["nrhat"] ** 2 - (rhat2 + 1.0 / N))
    print(f"M = 1 at (17, 3, 65): |nrhat^2 - (Rhat^2 + 1 / N)| = {diff.max():.2e}, bound {bound.min():.2e}")
    assert (diff <= bound).all() and (bound < 1e-12).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# sensitivity of the mirror


_SUM64 = NR.sum64


def _sum64_tree_upwards(u):
    """SUM64 with the tree's levels in the other order: h = 1, 2, .., 32 (r[s] += r[s + h] for the s that are multiples of 2 h)"""
    u = np.asarray(u, dtype=np.float64)
    n = u.shape[-1]
    r = np.zeros(u.shape[:-1] + (64,))
    for j in range((n + 63) // 64):
        blk = u[..., 64 * j:64 * (j + 1)]
        r[..., :blk.shape[-1]] = r[..., :blk.shape[-1]] + blk
    h = 1
    while h <= 32:
        r[..., ::2 * h] = r[..., ::2 * h] + r[..., h::2 * h]
        h *= 2
    return r[..., 0]


def _sum64_blocked_lanes(u):
    """SUM64 with lane s holding the CONSECUTIVE elements [s q, (s + 1) q), q = ceil(n / 64), instead of the strided ones"""
    u = np.asarray(u, dtype=np.float64)
    n = u.shape[-1]
    q = (n + 63) // 64
    pad = np.zeros(u.shape[:-1] + (64 * q,))
    pad[..., :n] = u
    return _SUM64(np.ascontiguousarray(pad.reshape(u.shape[:-1] + (64, q)).swapaxes(-1, -2)).reshape(u.shape[:-1] + (64 * q,)))


def _sum64_from_first(u):
    """SUM64 whose lanes start from their first element, not from +0.0"""
    u = np.asarray(u, dtype=np.float64)
    n = u.shape[-1]
    r = np.zeros(u.shape[:-1] + (64,))
    r[..., :min(n, 64)] = u[..., :64]
    for j in range(1, (n + 63) // 64):
        blk = u[..., 64 * j:64 * (j + 1)]
        r[..., :blk.shape[-1]] = r[..., :blk.shape[-1]] + blk
    h = 32
    while h >= 1:
        r[..., :h] = r[..., :h] + r[..., h:2 * h]
        h //= 2
    return r[..., 0]


def _with_sum64(fn, x, M):
    keep = NR.sum64
    NR.sum64 = fn
    try:
        return NR.nested_ref(x, M)
    finally:
        NR.sum64 = keep


def _changed(a, b):
    """elements of mean, between and within whose bits differ"""
    return sum(int((cases.bits(a[k]) != cases.bits(b[k])).sum()) for k in ("mean", "between", "within"))


@functools.lru_cache(maxsize=None)
def _wrong_mirrors(shape):
    N, d, C, M = shape
    K = C // M
    x, base = cases.frozen_slab(shape), cases.reference(shape)
    upwards = _changed(_with_sum64(_sum64_tree_upwards, x, M), base)
    blocked = _changed(_with_sum64(_sum64_blocked_lanes, x, M), base)
    twice = np.array(x)
    twice[:, :, 1] = twice[:, :, 0]                                  # member 1 of superchain 0 is member 0 read again
    twice = _changed(NR.nested_ref(twice, M), base)
    modk = np.ascontiguousarray(np.array(x).reshape(N, d, M, K).swapaxes(2, 3).reshape(N, d, C))      # chain c taken as member c / K of superchain c mod K
    modk = _changed(NR.nested_ref(modk, M), base)
    return dict(upwards=upwards, blocked=blocked, twice=twice, modk=modk, n=3 * d)


@pytest.mark.parametrize("shape", [(17, 3, 195, 3), (130, 3, 126, 63), (2, 3, 390, 130), (9, 3, 8320, 64), (17, 1, 4225, 65)], ids=cases.shape_id)
def test_the_mirror_can_tell_orders_and_labels_apart(shape):
    """Another tree order changes bits wherever a fold has more than two elements, another assignment of elements to lanes wherever a fold has more
    than 64; a member read twice and the superchain label c mod K change values."""
    N, d, C, M = shape
    got = _wrong_mirrors(shape)
    print(f"(N, d, C, M) = {shape}: of {got['n']} values of mean, between and within the bits change in {got['upwards']} with the tree taken upwards, "
          f"{got['blocked']} with consecutive elements per lane, {got['twice']} with a member read twice, {got['modk']} with k = c mod K")
    assert got["upwards"] > 0
    assert got["blocked"] > 0 if max(M, C // M) > 64 else got["blocked"] == 0        # one element per lane: both assignments are the same
    assert got["twice"] >= 2 * d                                     # between and within of every dimension at the least
    assert got["modk"] >= 2 * d


def test_a_fold_not_started_from_plus_zero_is_told_apart_by_minus_zero():
    """x + (+0.0) is x bit for bit unless x = -0.0, so only -0.0 can tell: elements of -0.0 sum to +0.0 from +0.0 and to -0.0 from the first of them.
    A chain mean IS -0.0 where the two draws are the smallest negative subnormal and 0: their sum halves to a tie that rounds to even."""
    minus_zero = np.full(70, -0.0)
    assert cases.bits(NR.sum64(minus_zero)) == 0 and cases.bits(_sum64_from_first(minus_zero)) == 1 << 63
    x = cases.slab(2, 3, 128, 64)
    x[0, 1, :], x[1, 1, :] = -5e-324, 0.0
    a, v = NR.chain_moments(x)
    assert (cases.bits(a)[1] == 1 << 63).all() and not cases.bits(v)[1].any()
    good, wrong = NR.nested_ref(x, 64), _with_sum64(_sum64_from_first, x, 64)
    assert cases.bits(good["mean"])[1] == 0 and cases.bits(good["super_mean"])[:, 1].tolist() == [0, 0]
    assert cases.bits(wrong["super_mean"])[:, 1].tolist() == [1 << 63] * 2            # M = 64 leaves no lane at its +0.0
    for i in (0, 2):
        assert all(cases.bits(good[k])[i] == cases.bits(wrong[k])[i] for k in ("mean", "between", "within"))
    a, v = NR.chain_moments(np.full((3, 1, 4), -0.0))
    assert not cases.bits(a).any() and not cases.bits(v).any()                  # the draws' own sums start from +0.0 as well


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# what the number means


def _chi2_upper(dof, z):
    """Wilson-Hilferty: the value that a chi^2_dof / dof variable exceeds with the upper-tail probability of a standard normal at z"""
    c = 2.0 / (9.0 * dof)
    return (1.0 - c + z * math.sqrt(c)) ** 3


def test_iid_chains_read_one_over_M_and_superchain_offsets_read_far_above():
    """K = M = 64, N = 1, d = 128 iid normal: (nrhat^2 - 1) M is chi^2_63 / 63 over a within with 64 * 63 degrees of freedom (sd 2.2 %).  z = 6 has
    an upper tail of 1e-9 per dimension; the within's own 6 sd are 14 %.  The mean over 128 dimensions has sd sqrt(2 / 63 / 128) = 0.016."""
    K = M = 64
    d = 128
    x = np.random.default_rng(7).standard_normal((1, d, K * M))
    r = NR.nested_ref(x, M)
    stat = (r["nrhat"] ** 2 - 1.0) * M
    hi = _chi2_upper(K - 1, 6.0) * 1.14
    lo = _chi2_upper(K - 1, -6.0) / 1.14
    print(f"iid, K = M = 64, N = 1, d = 128: (nrhat^2 - 1) M has mean {stat.mean():.3f}, min {stat.min():.3f}, max {stat.max():.3f}; bounds {lo:.3f} .. {hi:.3f}")
    assert (stat < hi).all() and (stat > lo).all()
    assert abs(stat.mean() - 1.0) < 6 * 0.016 + 0.02
    assert np.allclose(r["mcse_mean"], np.sqrt(r["between"] / K), rtol=1e-15)
    assert (np.abs(r["mean"]) < 6.0 / math.sqrt(K * M)).all()

    # unit offsets per superchain, d = 4, M = 16, K = 64: between ~ 1 + 1 / M, within ~ 1, so nrhat^2 - 1 ~ (1 + 1 / 16) chi^2_63 / 63
    d, M, K = 4, 16, 64
    rng = np.random.default_rng(8)
    base = rng.standard_normal((1, d, K * M))
    off = NR.superchain_init(rng.standard_normal((d, K)), M)
    clean, shifted = NR.nested_ref(base, M)["nrhat"], NR.nested_ref(base + off[None], M)["nrhat"]
    print(f"offsets of unit variance per superchain, d = 4, M = 16: nrhat {shifted.round(3).tolist()} against {clean.round(3).tolist()} without")
    assert (clean < math.sqrt(1.0 + hi / M)).all()
    assert (shifted ** 2 - 1.0 > (1.0 + 1.0 / M) * lo).all() and (shifted ** 2 - 1.0 < (1.0 + 1.0 / M) * hi).all()
    assert (shifted > clean + 0.2).all()


def test_superchain_init_is_np_repeat_along_the_chains():
    pts = np.arange(6.0).reshape(2, 3)
    out = NR.superchain_init(pts, 4)
    assert out.shape == (2, 12) and out.flags["C_CONTIGUOUS"]
    for c in range(12):
        assert np.array_equal(out[:, c], pts[:, c // 4])


def test_non_finite_samples_stay_in_their_dimension():
    shape = (17, 3, 195, 3)
    x = np.array(cases.frozen_slab(shape))
    x[3, 0, 100] = np.nan
    x[5, 2, 7] = np.inf
    got, clean = NR.nested_ref(x, 3), cases.reference(shape)
    assert all(np.isnan(got[k][0]) for k in ("nrhat", "mean", "between", "within", "mcse_mean"))
    assert got["mean"][2] == np.inf and np.isnan(got["between"][2]) and np.isnan(got["nrhat"][2])
    for k in ("nrhat", "mean", "between", "within", "mcse_mean"):
        assert cases.bits(got[k])[1] == cases.bits(clean[k])[1]
    assert np.array_equal(cases.bits(got["super_mean"][:, 1]), cases.bits(clean["super_mean"][:, 1]))
    assert np.isnan(got["super_mean"][100 // 3, 0]) and np.isfinite(np.delete(got["super_mean"][:, 0], 100 // 3)).all()


def test_chain_moments_and_the_state_as_a_2d_array():
    x = cases.slab(1, 3, 128, 64)
    a, v = NR.chain_moments(x[0])
    assert np.array_equal(a, x[0] + 0.0) and not v.any()
    r2, r3 = NR.nested_ref(x[0], 64), NR.nested_ref(x, 64)
    for k in cases.OUTPUTS:
        assert np.array_equal(cases.bits(r2[k]), cases.bits(r3[k]))
    with pytest.raises(ValueError):
        NR.nested_ref(x, 3)
    with pytest.raises(ValueError):
        NR.nested_ref(x, 128)
    with pytest.raises(ValueError):
        NR.nested_ref(x, 1)
