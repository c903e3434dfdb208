"""GPU: mcmc::aees through the C++ front end (include/mcmc.hpp), the Python wrappers, the example program, and the mixture target's
refusal by every other sampler."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mcmc_amd
import aees_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEANS, VARS, WTS = np.array([[-2.0, -2.0], [2.0, 2.0]]), np.array([0.1, 0.1]), np.array([0.5, 0.5])


def _compile(src, exe):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), f"-L{ROOT}/mcmc_amd", "-lmi_mcmc",
                           f"-Wl,-rpath,{ROOT}/mcmc_amd", "-o", str(exe)])


def test_example_crosses_modes_where_rwmh_does_not(tmp_path):
    """1 024 runs of the example all start in the mode at (-2, -2): AEES's kept draws put half their mass in each mode; the random walk
    with the same proposal, from the same start, stays where it started"""
    exe = tmp_path / "aees_mixture"
    _compile(os.path.join(ROOT, "examples", "aees_mixture.cpp"), exe)
    out = subprocess.run([str(exe), "1024"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    num = r"(-?[\d.]+)"
    pat = lambda head: re.search(head + rf" far={num} mean_far=\({num}, {num}\) mean_near=\({num}, {num}\)", out.stdout)
    dev, cb, rw = pat(r"aees device ok=1 runs=1024 n_keep=20000"), pat(r"aees callback ok=1"), pat(r"rwmh callback ok=1")
    assert dev and cb and rw, out.stdout
    far = float(dev.group(1))
    assert abs(far - 0.5) < 0.1, out.stdout
    assert all(abs(float(dev.group(i)) - 2.0) < 0.1 for i in (2, 3)) and all(abs(float(dev.group(i)) + 2.0) < 0.1 for i in (4, 5)), out.stdout
    assert float(rw.group(1)) < 0.02, out.stdout


_PROG = r'''
#include <cstdio>
#include "mcmc.hpp"
int main(int argc, char** argv)
{
    mcmc::ColVec_t x0(2); x0(0) = 0.4; x0(1) = -1.1;
    mcmc::ColVec_t T(3); T(0) = 3.0; T(1) = 12.0; T(2) = 1.5;
    mcmc::algo_settings_t s;
    s.rng_seed_value = 77;
    s.aees_settings.n_initial_draws = 30; s.aees_settings.n_burnin_draws = 20; s.aees_settings.n_keep_draws = 100;
    s.aees_settings.n_rings = 4; s.aees_settings.ee_prob_par = 0.2; s.aees_settings.temper_vec = T; s.aees_settings.par_scale = 0.8;
    mcmc::mi355x::target_t t = mcmc::mi355x::gaussian_iso(2);
    mcmc::Mat_t a, b;
    const bool oka = mcmc::aees(x0, mcmc::mi355x::device_value_kernel, a, &t, s);
    const bool okb = mcmc::aees(x0, [](const mcmc::ColVec_t& v, void*) { return -0.5 * (v(0) * v(0) + v(1) * v(1)); }, b, nullptr, s);
    std::FILE* f = std::fopen(argv[1], "wb");
    for (const mcmc::Mat_t* m : {&a, &b})
        for (size_t k = 0; k < size_t(m->rows()); ++k)
            for (size_t j = 0; j < 2; ++j) { const double v = (*m)(k, j); std::fwrite(&v, 8, 1, f); }
    std::fclose(f);
    std::printf("ok=%d %d rows=%zu %zu acc=%llu\n", int(oka), int(okb), size_t(a.rows()), size_t(b.rows()),
                (unsigned long long)t.n_accept_draws[0]);
    return (oka && okb) ? 0 : 1;
}
'''


def test_device_tag_and_lambda_routes_agree(tmp_path):
    src, exe, dump = tmp_path / "aees_routes.cpp", tmp_path / "aees_routes", tmp_path / "draws.bin"
    src.write_text(_PROG)
    _compile(src, exe)
    out = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"ok=1 1 rows=100 100 acc=(\d+)", out.stdout)
    assert m, out.stdout
    dd = np.fromfile(dump).reshape(2, 100, 2)
    assert np.array_equal(dd[0], dd[1])                   # the device target and the host lambda: the same bits
    x0 = np.array([0.4, -1.1])
    s = mcmc_amd.default_settings(rng_seed_value=77, n_burnin_draws=20, n_keep_draws=100)
    a = mcmc_amd.aees_settings(n_initial_draws=30, n_rings=4, ee_prob_par=0.2, temper_vec=[3.0, 12.0, 1.5], par_scale=0.8)
    ref, info = mcmc_amd.aees(mcmc_amd.TARGET_GAUSS_ISO, x0[None, :], s, a)
    assert np.array_equal(dd[0], ref[..., 0]) and int(m.group(1)) == int(info["n_accept"][-1, 0])


def test_python_callback_and_device_mixture_agree():
    """mcmc_amd.aees_callback with the mixture stated in Python (aees_ref.mixture: the device's operations) and mcmc_amd.aees on
    TARGET_GAUSS_MIXTURE: the same bits, every output"""
    s = mcmc_amd.default_settings(rng_seed_value=5, n_burnin_draws=10, n_keep_draws=60)
    a = mcmc_amd.aees_settings(n_initial_draws=10, n_rings=11, ee_prob_par=0.05, temper_vec=[60.0, 9.0], cov_mat=0.35 * np.eye(2))
    x0 = MEANS[0].copy()
    cd, ci = mcmc_amd.aees_callback(x0, aees_ref.mixture_fn(MEANS, VARS, WTS), s, a)
    dd, di = mcmc_amd.aees(mcmc_amd.mixture_target(MEANS, VARS, WTS), x0[None, :], s, a)
    assert np.array_equal(cd, dd[..., 0]) and np.array_equal(ci["final_states"], di["final_states"][..., 0])
    assert np.array_equal(ci["n_accept"], di["n_accept"][:, 0]) and np.array_equal(ci["n_ee_accept"], di["n_ee_accept"][:, 0])


def test_mixture_is_refused_by_every_other_sampler():
    d, Cn = 2, 4
    t = mcmc_amd.mixture_target(MEANS, VARS, WTS)
    s = mcmc_amd.default_settings(n_burnin_draws=2, n_keep_draws=2)
    theta = np.zeros((d, Cn))
    for name in ("hmc", "mala", "nuts", "rwmh", "rmhmc"):
        ch = mcmc_amd.make_chains(theta, Cn)
        rc = getattr(mcmc_amd.lib(), f"mi_mcmc_{name}_run")(C.byref(t), C.byref(s), C.byref(ch), None)
        assert rc == mcmc_amd.MI_ERR_UNSUPPORTED, (name, rc, mcmc_amd.lib().mi_mcmc_last_error())
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.de(mcmc_amd.TARGET_GAUSS_MIXTURE, np.zeros((Cn, d)), s, mcmc_amd.de_settings(n_pop=5), X=MEANS, prec=VARS,
                    y=mcmc_amd.mixture_log_constants(WTS, VARS, d))
    assert e.value.code == mcmc_amd.MI_ERR_UNSUPPORTED
