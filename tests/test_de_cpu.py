"""CPU: the DE reference (tests/de_ref.py) on hand-checkable cases, the C++ front end's mcmc::de, and the refusals of mi_mcmc_de_run."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import mcmc_amd
import orc
import de_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_generation_of_three_members_by_hand():
    """n_pop = 3, d = 1 on -x^2/2: every step of the first generation written out"""
    seed, pop, init, b = 11, 5, 0.3, 1e-4
    draws, X, n_acc = de_ref.de_ref(lambda x: -0.5 * x[0] * x[0], np.array([init]), 3, 0, 1, seed=seed, pop=pop, par_b=b)
    u01 = lambda lo, hi: float(2 * ((int(hi) << 32 | int(lo)) >> 12) + 1) / 2.0 ** 53
    blk = lambda gen, slot, tag: orc.philox([pop, gen, slot, tag], [seed, 0])
    x = [(init - 0.5) + ((init + 0.5) - (init - 0.5)) * u01(*blk(0, 2 * i + 1, 3)[:2]) for i in range(3)]     # B = 2 slots per member
    tv = [-0.5 * v * v for v in x]
    gam = 2.38 / math.sqrt(2.0)
    acc = 0
    for i in range(3):
        w = blk(0, 2 * i, 4)
        c1 = (int(w[0]) * 2) >> 32
        c1 += c1 >= i
        c2 = [m for m in range(3) if m not in (i, c1)][0]       # one member left: (w1 * 1) >> 32 = 0, skipped past i and c1
        prop = (x[i] + (x[c1] - x[c2]) * gam) + (-b + (b + b) * u01(*blk(0, 2 * i + 1, 4)[:2]))
        pv = -0.5 * prop * prop
        if pv - tv[i] > math.log(u01(w[2], w[3])):
            x[i], tv[i] = prop, pv
            acc += 1
    assert np.array_equal(draws[0, :, 0], np.array(x)) and np.array_equal(X[:, 0], np.array(x)) and n_acc == acc


def test_partners_are_uniform_over_the_allowed_pairs():
    """chi^2 over 10^5 Philox blocks: (c1, c2) uniform over the 12 ordered pairs of {0..4} \\ {i}"""
    n_pop, i, n = 5, 2, 100_000
    counts = {}
    for k in range(n):
        w = de_ref.block(3, 0, k // 64, k % 64, de_ref.STREAM_DE)
        c1, c2 = de_ref.partners(w, i, n_pop)
        assert c1 != i and c2 != i and c2 != c1 and 0 <= c1 < n_pop and 0 <= c2 < n_pop
        counts[(c1, c2)] = counts.get((c1, c2), 0) + 1
    assert len(counts) == 12
    e = n / 12
    chi2 = sum((v - e) ** 2 / e for v in counts.values())
    assert chi2 < 31.3       # 11 degrees of freedom, p = 0.001


def test_jump_schedule():
    d = 3
    g = de_ref.gamma(d)
    sched = [de_ref.gamma_at(gen, d, True, 2.0) for gen in range(30)]
    assert sched == [2.0 if (gen + 1) % 10 == 0 else g for gen in range(30)]
    assert all(de_ref.gamma_at(gen, d, False, 2.0) == g for gen in range(30))
    tgt = orc.TargetSpec(orc.TARGET_ISO, d, W=4)
    kw = dict(seed=4, n_pop=6, n_burnin=0, n_keep=12)
    a, _, _ = de_ref.de_ref(tgt, np.zeros(d), **kw)
    b, _, _ = de_ref.de_ref(tgt, np.zeros(d), jumps=True, par_gamma_jump=1.7, **kw)
    c, _, _ = de_ref.de_ref(tgt, np.zeros(d), jumps=True, par_gamma_jump=g, **kw)
    assert np.array_equal(a[:9], b[:9]) and not np.array_equal(a[9], b[9])     # generation 9 is the first jump
    assert np.array_equal(a, c)


def test_initial_box_is_used_untransformed_with_bounds():
    """the drawn rows are sampler-space values as they are (the reference's quirk); the box is clamped to the hard bounds"""
    d, n_pop, seed = 2, 4, 9
    lower, upper = np.array([0.0, -np.inf]), np.array([1.0, 0.25])
    init = np.array([0.9, 0.0])
    _, X, _ = de_ref.de_ref(lambda x: 0.0, init, n_pop, 0, 0, seed=seed, lower=lower, upper=upper)
    lo, hi = np.array([0.4, -0.5]), np.array([1.0, 0.25])           # [0.4, 1.4] -> [0.4, 1]; [-0.5, 0.5] -> [-0.5, 0.25]
    for i in range(n_pop):
        u = de_ref.uniforms(seed, 0, 0, i, d, de_ref.STREAM_DE_INIT)
        assert np.array_equal(X[i], lo + (hi - lo) * u)
    # ... and the target sees inv_transform of them: draws of a run that rejects everything are those rows inverse-transformed
    draws, X2, n_acc = de_ref.de_ref(lambda x: 0.0 if x[0] < 0 else -np.inf, init, n_pop, 0, 1, seed=seed, lower=lower, upper=upper)
    bd = de_ref.Bounds(d, lower, upper)
    assert n_acc == 0 and np.array_equal(X2, X)
    assert np.array_equal(draws[0], np.array([bd.inv(x) for x in X]))


def test_recovers_a_2d_gaussian():
    prec = np.array([[2.0, 0.6], [0.6, 1.0]])
    tgt = orc.TargetSpec(orc.TARGET_DENSE, 2, prec=prec, W=4)
    draws, _, n_acc = de_ref.de_ref(tgt, np.array([1.0, -1.0]), 20, 300, 1500, seed=1)
    x = draws.reshape(-1, 2)
    cov = np.linalg.inv(prec)
    se = np.sqrt(np.diag(cov) / 1500 * 20)          # generous: one effective draw per generation, x20 for the autocorrelation
    assert np.all(np.abs(x.mean(axis=0)) < 4 * se)
    assert np.allclose(np.cov(x.T), cov, rtol=0.15, atol=0.05)
    assert 0.05 < n_acc / (1500 * 20) < 0.9


def test_reference_style_de_program_compiles(tmp_path):
    src = tmp_path / "de_prog.cpp"
    src.write_text(r'''
#include "mcmc.hpp"
double lt(const mcmc::ColVec_t& v, void*) { return -0.5 * v(0) * v(0); }
int main()
{
    mcmc::ColVec_t x0(1); x0(0) = 1.0;
    mcmc::algo_settings_t s;
    s.de_settings.n_pop = 10; s.de_settings.jumps = true;
    mcmc::Cube_t draws;
    bool a = mcmc::de(x0, lt, draws, nullptr, s);
    bool b = mcmc::de(x0, [](const mcmc::ColVec_t& v, void*) { return -v(0) * v(0); }, draws, nullptr);
    mcmc::mi355x::target_t t = mcmc::mi355x::gaussian_iso(1);
    bool c = mcmc::de(x0, mcmc::mi355x::device_value_kernel, draws, &t, s);
    return (a && b && c) ? 0 : 1;
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT}/include", "-c", str(src), "-o", str(tmp_path / "de_prog.o")])


def _lib_or_skip():
    if not os.path.exists(mcmc_amd.LIB_PATH):
        pytest.skip("libmi_mcmc.so not built")
    return mcmc_amd.lib()


def _call(t, s, ds, p):
    return mcmc_amd.lib().mi_mcmc_de_run(C.byref(t) if t is not None else None, C.byref(s) if s is not None else None,
                                         C.byref(ds) if ds is not None else None, C.byref(p) if p is not None else None, None)


def test_bad_de_arguments_are_refused_without_a_gpu():
    _lib_or_skip()
    d, P = 3, 2
    s = mcmc_amd.default_settings(n_burnin_draws=2, n_keep_draws=2)
    ds = mcmc_amd.de_settings(n_pop=5)
    t = mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_ISO, d)
    init = np.zeros((d, P))
    pop = np.zeros((5, d, P))
    p = mcmc_amd.mi_populations()
    p.struct_size = C.sizeof(mcmc_amd.mi_populations)
    p.n_populations, p.initial_vals, p.population = P, init.ctypes.data, pop.ctypes.data
    for args in ((None, s, ds, p), (t, None, ds, p), (t, s, None, p), (t, s, ds, None)):
        assert _call(*args) == mcmc_amd.MI_ERR_BAD_ARG
    for n_pop in (0, 1, 2):
        ds.n_pop = n_pop
        assert _call(t, s, ds, p) == mcmc_amd.MI_ERR_BAD_ARG
        assert "n_pop" in mcmc_amd.lib().mi_mcmc_last_error().decode()
    ds.n_pop = 5
    for obj in (ds, p, s, t):
        good = obj.struct_size
        obj.struct_size = good + 8
        assert _call(t, s, ds, p) == mcmc_amd.MI_ERR_BAD_ARG
        obj.struct_size = good
    p.population = None
    assert _call(t, s, ds, p) == mcmc_amd.MI_ERR_BAD_ARG
    p.population = pop.ctypes.data
    p.initial_vals = None                                  # a fresh run without an initial box needs initial_vals
    assert _call(t, s, ds, p) == mcmc_amd.MI_ERR_BAD_ARG
    p.initial_vals = init.ctypes.data
    ds.n_pop = 1 << 31                                     # n_pop * (1 + ceil(d / 2)) >= 2^32
    assert _call(t, s, ds, p) == mcmc_amd.MI_ERR_UNSUPPORTED
    ds.n_pop = 5
    nm = mcmc_amd.make_target(mcmc_amd.TARGET_NORMAL_MODEL, 2, y=np.zeros(4))
    assert _call(nm, s, ds, p) == mcmc_amd.MI_ERR_UNSUPPORTED
    cb = mcmc_amd.LOG_KERNEL_CB(lambda v, g, u: 0.0)
    x0 = np.zeros(d)
    rc = mcmc_amd.lib().mi_mcmc_de_run_callback(x0.ctypes.data, d, cb, None, C.byref(s),
                                                C.byref(mcmc_amd.de_settings(n_pop=2)), None, None)
    assert rc == mcmc_amd.MI_ERR_BAD_ARG
    rc = mcmc_amd.lib().mi_mcmc_de_run_callback(None, d, cb, None, C.byref(s), C.byref(ds), None, None)
    assert rc == mcmc_amd.MI_ERR_BAD_ARG
    if mcmc_amd.lib().mi_mcmc_device_count() == 0:         # valid arguments: no CPU fallback
        assert _call(t, s, ds, p) == mcmc_amd.MI_ERR_NO_DEVICE


def test_de_settings_defaults_follow_the_reference():
    _lib_or_skip()
    ds = mcmc_amd.de_settings()
    assert (ds.jumps, ds.n_pop, ds.par_b, ds.par_gamma_jump, ds.par_gamma) == (0, 100, 1e-4, 2.0, 1.0)
    assert ds.struct_size == C.sizeof(mcmc_amd.mi_de_settings)
