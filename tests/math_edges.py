"""Fixed input tables at the edges of the deterministic math functions, the Philox + Box-Muller generator and the fp64 MFMA tile, shared by
tests/test_math_edges_cpu.py (oracle against mpmath) and tests/test_gpu_math_edges.py (device against oracle, bit for bit).  Plain numpy, no GPU,
no randomness that is not seeded here; every function returns the same array on every call."""
import math
from fractions import Fraction

import numpy as np

NAN, INF = float("nan"), float("inf")
TINY = 5e-324                                   # the smallest subnormal, 2^-1074
DBL_MAX = 1.7976931348623157e308
EXP_HI, EXP_LO = 709.782712893384, -745.2       # det_exp: +inf above, 0 below
LOG_SWITCH = float.fromhex("0x1.6a09e667f3bcdp+0")   # det_log: mantissas above it are halved
LN2 = math.log(2.0)


def nbr(x, k):
    """x moved by k units in the last place (k of either sign), for a finite x that does not cross zero on the way"""
    a = np.array([x], dtype=np.float64)
    i = a.view(np.int64)
    i += (k if x > 0 or (x == 0 and not math.copysign(1, x) < 0) else -k)
    return float(a[0])


def around(x, n):
    """x and its n neighbours on each side"""
    return [nbr(x, k) for k in range(-n, n + 1)]


def _arr(vals):
    return np.array(vals, dtype=np.float64)


def exp_table():
    v = [NAN, INF, -INF, 0.0, -0.0, TINY, -TINY, 2.0 ** -54, -2.0 ** -54]
    v += around(EXP_HI, 3) + around(EXP_LO, 3)
    for k in range(-1075, 1025):                # rint(x / ln2) at its integers and at its ties
        for x in [k * LN2] + around((k + 0.5) * LN2, 1):
            if EXP_LO <= x <= EXP_HI:
                v.append(x)
    v += list(np.linspace(-745.2, -708.39, 1000))          # subnormal results
    return _arr(v)


def log_table():
    v = [NAN, INF, -INF, 0.0, -0.0, -1.0, DBL_MAX]
    v += [math.ldexp(1.0, k) for k in range(-1074, 1024)]
    for e in (-1022, -600, -1, 0, 1, 700, 1022):
        v += [math.ldexp(m, e) for m in around(LOG_SWITCH, 4)]
    v += [nbr(1.0, k) for k in range(-40, 41) if k != 0]
    v += [math.ldexp(float(m), -1074) for m in (1, 2, 3, 7, 1023, 2 ** 30 + 1, 2 ** 51 + 12345)]
    return _arr(v)


def sincos_table():
    """u in [0, 1) only: the octant edges k/8 with two neighbours on each side that stay inside the domain"""
    v = [0.0, TINY, 2 * TINY, 2.0 ** -53, 1.0 - 2.0 ** -53, nbr(1.0 - 2.0 ** -53, -1)]
    for k in range(1, 8):
        v += around(k / 8.0, 2)
    return _arr(v)


def logistic_table():
    """softplus and sigmoid"""
    v = [NAN, INF, -INF, 0.0, -0.0, 1e-300, -1e-300]
    pos = list(np.round(np.arange(36.5, 36.9001, 0.01), 2)) + [40.0, 708.0, 708.5, 709.0, 709.5, 709.78, 709.79, 710.0, 745.0, 745.1, 745.13, 745.14,
                                                                745.2, 800.0]
    v += pos + [-x for x in pos]
    v += list(np.linspace(-745.0, 745.0, 3001))
    return _arr(v)


def norm_ppf_table():
    v = [0.0, -0.0, -TINY, -1.0, -INF, 1.0, nbr(1.0, 1), 2.0, INF, NAN, 0.5, nbr(0.5, -1), nbr(0.5, 1)]
    v += around(0.075, 4) + around(0.925, 4)                       # |p - 0.5| = 0.425: centre <-> tails
    v += around(math.exp(-25.0), 4) + around(1.0 - math.exp(-25.0), 4)   # r = 5: the two tail branches
    v += [TINY, 2.0 ** -53, 1.0 - 2.0 ** -53]
    for S in (1, 2, 3, 1000):                                      # the normal-score grid of the rank-normalised statistics
        v += [(R - 0.375) / (S + 0.25) for R in range(1, S + 1)]
    for S in (10 ** 6, 10 ** 9):
        v += [(1 - 0.375) / (S + 0.25), (S - 0.375) / (S + 0.25)]
    return _arr(v)


# det_pow(x, y) is exp(y * log(x)) and nothing else: these pairs give NaN (0 * inf), where IEEE pow gives 1
POW_NAN_BY_DEFINITION = [(0.0, 0.0), (INF, 0.0), (1.0, INF)]


def pow_table():
    """(x, y): the dual-averaging schedule it^-kappa, and the specials; the last len(POW_NAN_BY_DEFINITION) pairs are those of that list"""
    x, y = [], []
    for kappa in (0.75, 0.5, 1.0):
        for it in list(range(1, 65)) + [10 ** 3, 10 ** 6, 2 ** 31]:
            x.append(float(it)), y.append(-kappa)
    for a in (TINY, 1e-300, 0.5, 1.0, 2.0, 1e300, DBL_MAX):
        x.append(a), y.append(0.0)
        x.append(a), y.append(-0.0)
    for b in (-0.75, 0.5, 1.0, 1e300, -1e300, TINY):
        x.append(1.0), y.append(b)
    x += [0.0, INF, NAN, 2.0, NAN]
    y += [-0.75, -0.75, -0.75, NAN, NAN]
    for a, b in POW_NAN_BY_DEFINITION:
        x.append(a), y.append(b)
    return _arr(x), _arr(y)


def rng_cases():
    """(seed, chain, draw, stream, d)"""
    M64 = 2 ** 64 - 1
    return [(1, 0, 0, 0, 128), (2 ** 40 + 7, 2 ** 33 + 5, 17, 0, 37), (99, 65535, 199, 2, 1024), (5, 3, 2, 0, 3),
            (7, 2 ** 32 - 1, 1, 0, 9), (7, 2 ** 32, 1, 0, 9), (7, 2 ** 56 - 1, 1, 0, 8), (7, 2 ** 56 - 1, 2 ** 32 - 1, 2, 7),
            (11, 5, 2 ** 32 - 1, 0, 1024), (0, 0, 0, 0, 1), (0, 1, 0, 0, 2), (0, 2 ** 32, 3, 0, 7), (M64, 0, 0, 0, 8),
            (M64, 2 ** 56 - 1, 2 ** 32 - 1, 0, 9), (M64, 2 ** 32 - 1, 5, 0, 1), (M64, 9, 9, 2, 2), (0, 2 ** 56 - 1, 0, 0, 1024)]


def uniform_cases():
    """(seed, chain, draw, slot)"""
    M64 = 2 ** 64 - 1
    return [(1, 0, 0, 0), (7, 123456, 42, 3), (2 ** 63 + 1, 2 ** 35, 2 ** 31, 9), (0, 0, 0, 0), (M64, 0, 0, 0), (0, 2 ** 32 - 1, 0, 0),
            (0, 2 ** 32, 0, 0), (M64, 2 ** 56 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (7, 2 ** 56 - 1, 1, 0), (7, 1, 2 ** 32 - 1, 0), (7, 1, 1, 2 ** 32 - 1)]


# ------------------------------------------------------------------ the MFMA tile: D = A (16 x 4) B (4 x 16) + C (16 x 16)
def fma_ieee(a, b, c):
    """fma(a, b, c) of IEEE 754 binary64 in round-to-nearest-even: one rounding of the exact a b + c"""
    if a != a or b != b or c != c:
        return NAN
    if math.isinf(a) or math.isinf(b):
        if a == 0.0 or b == 0.0:
            return NAN                                              # inf * 0
        p = math.copysign(INF, math.copysign(1.0, a) * math.copysign(1.0, b))
        return NAN if math.isinf(c) and c != p else p               # inf - inf
    if math.isinf(c):
        return c                                                    # the exact product is finite, however large
    psign = math.copysign(1.0, a) * math.copysign(1.0, b)
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        if (a == 0.0 or b == 0.0) and c == 0.0:                     # (+-0) + (+-0): -0 only if both are
            return -0.0 if psign < 0 and math.copysign(1.0, c) < 0 else 0.0
        return 0.0                                                  # exact cancellation of two non-zeros: +0
    try:
        r = float(exact)                                            # correctly rounded, in the subnormal range too
    except OverflowError:
        r = INF
    return math.copysign(r, 1.0 if exact > 0 else -1.0)             # an underflow to zero keeps the sign of the exact value


def mfma_reference(A, B, C):
    """The tile as a sequential fma chain, k ascending, starting from C"""
    D = np.empty((16, 16))
    for i in range(16):
        for j in range(16):
            acc = float(C[i, j])
            for k in range(4):
                acc = fma_ieee(float(A[i, k]), float(B[k, j]), acc)
            D[i, j] = acc
    return D


def _sub(rng, shape, bits=52):
    """random subnormals m 2^-1074, 1 <= m < 2^bits, of either sign"""
    m = rng.integers(1, 2 ** bits, shape).astype(np.float64)
    return np.ldexp(m, -1074) * rng.choice([-1.0, 1.0], shape)


def mfma_tiles():
    """name -> (A, B, C).  Names that start with 'sub_' put subnormal numbers into operands, into C or into results."""
    rng = np.random.default_rng(20240607)
    t = {}
    # operands and C all subnormal: every product is below 2^-2044, so D is C unless C is flushed
    t["sub_all"] = (_sub(rng, (16, 4)), _sub(rng, (4, 16)), _sub(rng, (16, 16)))
    # a subnormal operand against a large normal one: normal products, which a flushed operand would turn into zeros
    t["sub_operand_normal_product"] = (_sub(rng, (16, 4)), np.ldexp(rng.uniform(1, 2, (4, 16)), rng.integers(1000, 1020, (4, 16))) * rng.choice([-1.0, 1.0], (4, 16)),
                                       rng.standard_normal((16, 16)))
    t["sub_operand_b"] = (np.ldexp(rng.uniform(1, 2, (16, 4)), rng.integers(980, 1010, (16, 4))) * rng.choice([-1.0, 1.0], (16, 4)), _sub(rng, (4, 16)),
                          np.zeros((16, 16)))
    # normal operands, products and partial sums subnormal (2^-1074 .. 2^-1023), C zero or subnormal
    A = np.ldexp(rng.uniform(1, 2, (16, 4)), rng.integers(-540, -520, (16, 4))) * rng.choice([-1.0, 1.0], (16, 4))
    B = np.ldexp(rng.uniform(1, 2, (4, 16)), rng.integers(-530, -505, (4, 16))) * rng.choice([-1.0, 1.0], (4, 16))
    C = _sub(rng, (16, 16), 40)
    C[::2] = 0.0
    t["sub_products"] = (A, B, C)
    # subnormal C, the k = 1 product of the opposite sign and nearly its size: the sum cancels into the low subnormal range; the other products are zero
    c = np.ldexp(rng.integers(2 ** 44, 2 ** 45, 16).astype(np.float64), -1074)
    u = rng.uniform(1, 2, 16)
    A = np.zeros((16, 4))
    A[:, 1] = np.ldexp(u, -500)
    B = np.zeros((4, 16))
    B[1] = -np.ldexp(c, 500) * (1.0 + np.ldexp(rng.integers(-8, 9, 16).astype(np.float64), -30))
    t["sub_cancel"] = (A, B, u[:, None] * c[None, :])
    # signed zeros: operands from {-0, +0, -1, +1}, C from {-0, +0}
    z = np.array([-0.0, 0.0, -1.0, 1.0])
    t["zeros"] = (z[rng.integers(0, 4, (16, 4))], z[rng.integers(0, 4, (4, 16))], z[rng.integers(0, 2, (16, 16))])
    A0, B0 = np.zeros((16, 4)), np.zeros((4, 16))
    A0[::2] = -0.0
    B0[:, ::3] = -0.0
    t["zeros_only"] = (A0, B0, np.full((16, 16), -0.0))
    # overflow at k = 1, finite products after it, one of them larger than DBL_MAX with the other sign: an fma chain stays at inf
    A = rng.uniform(1, 2, (16, 4)) * rng.choice([-1.0, 1.0], (16, 4))
    B = rng.uniform(1, 2, (4, 16)) * rng.choice([-1.0, 1.0], (4, 16))
    A[:, 1] *= 1e200
    B[1] *= 1e200
    A[:8, 3] *= -1e200 * np.sign(A[:8, 1]) * np.sign(A[:8, 3])
    B[3] = np.abs(B[3]) * 1e200 * np.sign(B[1])
    t["overflow_mid_chain"] = (A, B, rng.standard_normal((16, 16)))
    # partial sums between 2^1023 and DBL_MAX that come back down: the exact chain never overflows
    A = np.ones((16, 4))
    B = np.ones((4, 16))
    for k in (0, 1, 2):
        A[:, k], B[k] = (-1.0 if k == 2 else 1.0) * 2.0 ** 511, 2.0 ** 512 * rng.uniform(0.5, 0.99, 16)
    t["near_overflow"] = (A, B, rng.standard_normal((16, 16)) * 1e300)
    # inf * 0, inf - inf, and a NaN in A, in B, in C alone
    A = rng.standard_normal((16, 4))
    B = rng.standard_normal((4, 16))
    A[0, 2], B[2, 0] = INF, 0.0                                      # row 0: inf * B[2, j]; column 0: inf * 0 = NaN
    A[1, 0], A[1, 3] = INF, INF                                     # row 1: inf B[0,j] + inf B[3,j]: NaN where the signs differ
    A[2, 1] = -INF
    B[1, 5] = -0.0
    C = rng.standard_normal((16, 16))
    C[2, 7], C[3, 3], C[4, 4] = INF, -INF, INF                      # row 2: -inf B[1,7] against +inf in C
    t["inf_rules"] = (A, B, C)
    A = rng.standard_normal((16, 4))
    A[5, 2] = NAN
    t["nan_in_a"] = (A, rng.standard_normal((4, 16)), rng.standard_normal((16, 16)))
    B = rng.standard_normal((4, 16))
    B[0, 9] = NAN
    t["nan_in_b"] = (rng.standard_normal((16, 4)), B, rng.standard_normal((16, 16)))
    C = rng.standard_normal((16, 16))
    C[15, 15], C[0, 0] = NAN, NAN
    t["nan_in_c"] = (rng.standard_normal((16, 4)), rng.standard_normal((4, 16)), C)
    return t
