"""CPU: the AEES reference (tests/aees_ref.py) on hand-checkable cases, the window order and the lazy merge the kernel runs, the mixture
target, the C++ front end's mcmc::aees, and the refusals of mi_mcmc_aees_run."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import mcmc_amd
import orc
import aees_ref
import de_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f(x):
    return -0.5 * (x[0] * x[0] + x[1] * x[1]) + 0.25 * x[0]


def _mh_by_hand(x, v, seed, chain, n, T):
    """single_step_mh with the identity cov and par_scale 1: X + sqrt(T) z (the fma chain over exact zeros is the product)"""
    z = orc.normal_vec(seed, chain, n, aees_ref.STREAM_AEES_NORMAL, 2)
    w = de_ref.block(seed, chain, n, 0, aees_ref.STREAM_AEES)
    prop = x + math.sqrt(T) * z
    vp = _f(prop)
    comp = min(0.01, (vp - v) / T)
    return (prop, vp, 1) if aees_ref.u01(w[2], w[3]) < aees_ref.exp(comp) else (x, v, 0)


def test_two_levels_by_hand():
    """K = 2, d = 2, S = 0, ee_prob 1, one ring: level 1 becomes active at draw 1 and takes an equi-energy step over level 0's window
    [0, 1].  That window is row 0 of kernel_vals -- never written, all zeros (quirk 1) -- so its stable order is the identity and
    the rank-r pick is position r.  The seed is chosen so that r = 1 = n: the entry of draw 1 is not stored yet and the proposal is the
    zero vector (quirk 3), not level 0's state.  ee_prob 1 makes z_eps <= ee_prob always: no MH step on level 1."""
    seed = next(s for s in range(100) if math.floor(aees_ref.u01(*de_ref.block(s, 1, 1, 1, aees_ref.STREAM_AEES)[:2]) * 2) == 1)
    x0 = np.array([0.3, -0.7])
    tr = []
    draws, X, n_acc, n_ee = aees_ref.aees_ref(_f, x0, 0, 2, seed=seed, n_initial=0, n_rings=1, ee_prob=1.0, temper_vec=[4.0], trace=tr)
    x, v = x0.copy(), _f(x0)
    acc0 = 0
    for n in range(2):                                     # level 0 at T = 4, chain id run K + 0
        x, v, a = _mh_by_hand(x, v, seed, 0, n, 4.0)
        acc0 += a
    assert np.array_equal(X[0], x) and n_acc[0] == acc0
    assert tr == [dict(n=1, k=1, s=2, bounds=[], which=0, r=1, ind_mix=1, accept=True)]
    # the zero proposal: f(0) = 0, new = (0 / 4, 0 / 1) against the level's kernel_vals_prev (0, 0): comp = 0, z > exp(0) = 1 never
    assert np.array_equal(X[1], np.zeros(2)) and not np.array_equal(x, np.zeros(2))
    assert list(n_ee) == [0, 1] and list(n_acc) == [acc0, 0]
    assert np.array_equal(draws, np.zeros((2, 2)))         # level 1: inactive at draw 0 (zeros), the zero proposal at draw 1


def test_ee_proposal_is_an_absolute_draw_index():
    """quirk 2: on level 2 the pick is a window position used as an absolute draw index of level 1, so with S = 30 it lands on draws
    before level 1 became active (<= S): their stored states are zeros"""
    tr = []
    aees_ref.aees_ref(_f, np.array([1.0, 1.0]), 10, 20, seed=3, n_initial=20, n_rings=3, ee_prob=0.5, temper_vec=[9.0, 3.0], trace=tr)
    lvl2 = [t for t in tr if t["k"] == 2]
    assert lvl2 and all(t["ind_mix"] <= t["n"] - 30 for t in lvl2)
    assert any(t["ind_mix"] <= 30 for t in lvl2)


def _brute_order(w):
    """insertion by the pinned comparison: a before b iff a < b, or a == b (with -0 == +0), or both NaN, and a came first; NaN last"""
    def less(i, j):
        a, b = w[i], w[j]
        if a != a:
            return b != b and i < j
        if b != b:
            return True
        return a < b or (a == b and i < j)
    out = []
    for i in range(len(w)):
        p = len(out)
        while p > 0 and less(i, out[p - 1]):
            p -= 1
        out.insert(p, i)
    return out


def _u64_key(v):
    """the kernel's key (aees.hpp: aees_key): the IEEE bits made monotone, -0 -> +0, NaN -> the largest key"""
    if v != v:
        return (1 << 64) - 1
    b = 0 if v == 0.0 else struct.unpack("<Q", struct.pack("<d", v))[0]
    return ((~b) & ((1 << 64) - 1)) if (b >> 63) else (b | (1 << 63))


def _lazy(w, steps, chunk=256):
    """the kernel's index upkeep (aees.hpp: aees_merge): the window grows to each m in steps; the new values are rank-sorted in chunks,
    old elements go after every new key strictly below, new ones after every old key <= theirs"""
    keys, pos, length = [], [], 0
    for m in steps:
        while length < m:
            a = min(chunk, m - length)
            nk = [(_u64_key(w[length + t]), length + t) for t in range(a)]
            srt = [None] * a
            for t, (kt, pt) in enumerate(nk):
                srt[sum(1 for u, (ku, _) in enumerate(nk) if ku < kt or (ku == kt and u < t))] = (kt, pt)
            out = [None] * (length + a)
            for i in range(length):
                j = sum(1 for kt, _ in srt if kt < keys[i])
                out[i + j] = (keys[i], pos[i])
            for t, (kt, pt) in enumerate(srt):
                j = sum(1 for k in keys if k <= kt)
                out[t + j] = (kt, pt)
            keys, pos = [k for k, _ in out], [p for _, p in out]
            length += a
        yield list(pos)


def test_window_order_against_brute_force():
    rng = np.random.default_rng(1)
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -1.5, 2.0]
    w = [special[i] if i < len(special) else float(rng.choice(special + [float(rng.integers(-3, 3))])) for i in range(600)]
    rng.shuffle(w)
    steps = [5, 6, 40, 41, 300, 301, 302, 600]
    for m, lazy in zip(steps, _lazy(w, steps, chunk=32)):
        brute = _brute_order(w[:m])
        assert aees_ref.stable_argsort(w[:m]) == brute
        assert lazy == brute


def test_mixture_value_against_logsumexp():
    rng = np.random.default_rng(2)
    M, d = 3, 4
    means, s2, wts = rng.normal(size=(M, d)) * 2, rng.uniform(0.1, 2.0, size=M), rng.dirichlet(np.ones(M))
    f = aees_ref.mixture_fn(means, s2, wts)
    for _ in range(200):
        x = rng.normal(size=d) * 3
        a = np.log(wts) - 0.5 * d * np.log(2 * np.pi * s2) - 0.5 * ((x - means) ** 2).sum(axis=1) / s2
        mx = a.max()
        expect = mx + np.log(np.exp(a - mx).sum())
        assert abs(f(x) - expect) <= 1e-14 * max(1.0, abs(expect))
    assert f(np.array([np.nan, 0, 0, 0])) != f(np.array([np.nan, 0, 0, 0]))
    assert f(np.array([np.inf, 0, 0, 0])) == -np.inf
    assert np.array_equal(mcmc_amd.mixture_log_constants(wts, s2, d), np.log(wts) - (d / 2.0) * np.log(2.0 * np.pi * s2))


def test_reference_style_aees_program_compiles(tmp_path):
    src = tmp_path / "aees_prog.cpp"
    src.write_text(r'''
#include "mcmc.hpp"
double lt(const mcmc::ColVec_t& v, void*) { return -0.5 * (v(0) * v(0) + v(1) * v(1)); }
int main()
{
    mcmc::ColVec_t x0(2); x0(0) = -2.0; x0(1) = -2.0;
    mcmc::ColVec_t T(2); T(0) = 60.0; T(1) = 9.0;
    mcmc::algo_settings_t s;
    s.aees_settings.n_initial_draws = 100; s.aees_settings.n_burnin_draws = 100; s.aees_settings.n_keep_draws = 200;
    s.aees_settings.n_rings = 11; s.aees_settings.ee_prob_par = 0.05; s.aees_settings.temper_vec = T;
    s.aees_settings.par_scale = 1.0;
    mcmc::Mat_t cov(2, 2); cov(0, 0) = 0.35; cov(1, 1) = 0.35; s.aees_settings.cov_mat = cov;
    mcmc::Mat_t draws;
    bool a = mcmc::aees(x0, lt, draws, nullptr, s);
    bool b = mcmc::aees(x0, [](const mcmc::ColVec_t& v, void*) { return -v(0) * v(0); }, draws, nullptr);
    const double mu[4] = {-2, -2, 2, 2}, s2[2] = {0.1, 0.1}, w[2] = {0.5, 0.5};
    double lc[2];
    mcmc::mi355x::mixture_log_constants(2, 2, w, s2, lc);
    mcmc::mi355x::target_t t = mcmc::mi355x::gaussian_mixture(2, 2, mu, s2, lc);
    t.n_chains = 8;
    bool c = mcmc::aees(x0, mcmc::mi355x::device_value_kernel, draws, &t, s);
    return (a && b && c) ? 0 : 1;
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT}/include", "-c", str(src), "-o", str(tmp_path / "aees_prog.o")])


def _lib_or_skip():
    if not os.path.exists(mcmc_amd.LIB_PATH):
        pytest.skip("libmi_mcmc.so not built")
    return mcmc_amd.lib()


def _call(t, s, a, r):
    return mcmc_amd.lib().mi_mcmc_aees_run(C.byref(t) if t is not None else None, C.byref(s) if s is not None else None,
                                           C.byref(a) if a is not None else None, C.byref(r) if r is not None else None, None)


def test_bad_aees_arguments_are_refused_without_a_gpu():
    _lib_or_skip()
    d, P = 2, 3
    s = mcmc_amd.default_settings(n_burnin_draws=2, n_keep_draws=2)
    a = mcmc_amd.aees_settings(n_initial_draws=2, temper_vec=[3.0])
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_ISO, d)
    init = np.zeros((d, P))
    r = mcmc_amd.mi_aees_runs()
    r.struct_size = C.sizeof(mcmc_amd.mi_aees_runs)
    r.n_runs, r.initial_vals = P, init.ctypes.data
    for args in ((None, s, a, r), (t, None, a, r), (t, s, None, r), (t, s, a, None)):
        assert _call(*args) == mcmc_amd.MI_ERR_BAD_ARG
    for obj in (a, r, s, t):
        good = obj.struct_size
        obj.struct_size = good + 8
        assert _call(t, s, a, r) == mcmc_amd.MI_ERR_BAD_ARG
        obj.struct_size = good
    a.n_rings = 0
    assert _call(t, s, a, r) == mcmc_amd.MI_ERR_BAD_ARG and "n_rings" in mcmc_amd.lib().mi_mcmc_last_error().decode()
    a.n_rings = 5
    for bad in (0.0, -1.0, np.inf, np.nan):
        ab = mcmc_amd.aees_settings(n_initial_draws=2, temper_vec=[3.0, bad])
        assert _call(t, s, ab, r) == mcmc_amd.MI_ERR_BAD_ARG and "temper" in mcmc_amd.lib().mi_mcmc_last_error().decode()
    big = mcmc_amd.aees_settings(n_initial_draws=(1 << 31), temper_vec=[3.0])    # n_total = 2 + 2 (2^31 + 2) >= 2^32
    assert _call(t, s, big, r) == mcmc_amd.MI_ERR_BAD_ARG
    ok = mcmc_amd.aees_settings(n_initial_draws=(1 << 30), temper_vec=[3.0])     # n_total = 2 + 2 (2^30 + 2) < 2^32: accepted so far
    r.initial_vals = None
    assert _call(t, s, ok, r) == mcmc_amd.MI_ERR_BAD_ARG
    r.initial_vals = init.ctypes.data
    r.n_runs = 0
    assert _call(t, s, a, r) == mcmc_amd.MI_ERR_BAD_ARG
    r.n_runs = P
    s.vals_bound = 1                                       # bounds without the tables
    assert _call(t, s, a, r) == mcmc_amd.MI_ERR_BAD_ARG
    s.vals_bound = 0
    cb = mcmc_amd.LOG_KERNEL_CB(lambda v, g, u: 0.0)
    x0 = np.zeros(d)
    z = mcmc_amd.aees_settings(n_rings=0)
    rc = mcmc_amd.lib().mi_mcmc_aees_run_callback(x0.ctypes.data, d, cb, None, C.byref(s),
                                                  C.byref(z), None, None, None, None)
    assert rc == mcmc_amd.MI_ERR_BAD_ARG
    rc = mcmc_amd.lib().mi_mcmc_aees_run_callback(None, d, cb, None, C.byref(s), C.byref(a), None, None, None, None)
    assert rc == mcmc_amd.MI_ERR_BAD_ARG
    if mcmc_amd.lib().mi_mcmc_device_count() == 0:         # valid arguments: no CPU fallback
        assert _call(t, s, a, r) == mcmc_amd.MI_ERR_NO_DEVICE


def test_aees_settings_defaults_follow_the_reference():
    _lib_or_skip()
    a = mcmc_amd.aees_settings()
    assert (a.n_initial_draws, a.par_scale, a.n_rings, a.ee_prob_par, a.temper_len) == (1000, 1.0, 5, 0.10, 0)
    assert a.cov_mat is None and a.temper_vec is None
    assert a.struct_size == C.sizeof(mcmc_amd.mi_aees_settings)
