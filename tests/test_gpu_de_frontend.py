"""GPU: mcmc::de through the C++ front end (include/mcmc.hpp) and the example program."""
import os
import re
import subprocess

import numpy as np
import pytest

import mcmc_amd
import de_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(src, exe):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), f"-L{ROOT}/mcmc_amd", "-lmi_mcmc",
                           f"-Wl,-rpath,{ROOT}/mcmc_amd", "-o", str(exe)])


def test_example_posterior_mean(tmp_path):
    exe = tmp_path / "de_normal_mean"
    _compile(os.path.join(ROOT, "examples", "de_normal_mean.cpp"), exe)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"de ok=1 n_pop=100 n_keep=2000 mean=(\S+) se=(\S+) analytic=(\S+) analytic_sd=(\S+) accept=(\S+)", out.stdout)
    assert m, out.stdout
    mean, se, analytic, sd, acc = (float(m.group(i)) for i in range(1, 6))
    assert 0 < se < sd and abs(mean - analytic) < 4 * se, out.stdout
    assert 0.05 < acc < 0.95


_PROG = r'''
#include <cstdio>
#include "mcmc.hpp"
int main(int argc, char** argv)
{
    const size_t d = 3;
    mcmc::ColVec_t x0(d);
    for (size_t i = 0; i < d; ++i) x0(i) = 0.25 * double(i) - 0.1;
    mcmc::algo_settings_t s;
    s.rng_seed_value = 21;
    s.de_settings.n_pop = 7; s.de_settings.n_burnin_draws = 5; s.de_settings.n_keep_draws = 6; s.de_settings.jumps = true;
    mcmc::mi355x::target_t t = mcmc::mi355x::gaussian_iso(d);
    mcmc::Cube_t a, b;
    const bool oka = mcmc::de(x0, mcmc::mi355x::device_value_kernel, a, &t, s);
    const size_t na = s.de_settings.n_accept_draws;
    const bool okb = mcmc::de(x0, [](const mcmc::ColVec_t& v, void*) { return -0.5 * (v(0) * v(0) + v(1) * v(1) + v(2) * v(2)); }, b, nullptr, s);
    const size_t nb = s.de_settings.n_accept_draws;
    std::FILE* f = std::fopen(argv[1], "wb");
    for (const mcmc::Cube_t* c : {&a, &b})
        for (size_t k = 0; k < c->n_mat(); ++k)
            for (size_t i = 0; i < 7; ++i)
                for (size_t j = 0; j < d; ++j) { const double v = c->mat(k)(i, j); std::fwrite(&v, 8, 1, f); }
    std::fclose(f);
    std::printf("ok=%d %d acc=%zu %zu\n", int(oka), int(okb), na, nb);
    return (oka && okb) ? 0 : 1;
}
'''


def test_device_tag_and_lambda_routes(tmp_path):
    src, exe, dump = tmp_path / "de_routes.cpp", tmp_path / "de_routes", tmp_path / "draws.bin"
    src.write_text(_PROG)
    _compile(src, exe)
    out = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"ok=1 1 acc=(\d+) (\d+)", out.stdout)
    assert m, out.stdout
    d, n_pop, nb, nk = 3, 7, 5, 6
    dd = np.fromfile(dump).reshape(2, nk, n_pop, d)
    x0 = 0.25 * np.arange(d) - 0.1
    # the device tag: the same bits as mcmc_amd.de on the built-in target
    s = mcmc_amd.default_settings(rng_seed_value=21, n_burnin_draws=nb, n_keep_draws=nk)
    ref, info = mcmc_amd.de(mcmc_amd.TARGET_GAUSS_ISO, x0[None, :], s, mcmc_amd.de_settings(n_pop=n_pop, jumps=1))
    assert np.array_equal(dd[0], ref[..., 0]) and int(m.group(1)) == int(info["n_accept"][0])
    # the lambda: the CPU reference with the same function
    rd, _, racc = de_ref.de_ref(lambda v: -0.5 * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), x0, n_pop, nb, nk, seed=21, jumps=True)
    assert np.array_equal(dd[1], rd) and int(m.group(2)) == racc


def test_python_callback_route_matches_the_reference():
    d, n_pop = 2, 5
    x0 = np.array([0.5, -0.25])
    lower, upper = np.array([0.0, -1.0]), np.array([np.inf, 1.0])
    s = mcmc_amd.default_settings(rng_seed_value=4, n_burnin_draws=3, n_keep_draws=4, vals_bound=1, lower_bounds=lower, upper_bounds=upper)
    f = lambda v: -0.5 * (v[0] - 1.0) * (v[0] - 1.0) - v[1] * v[1]
    draws, n_acc = mcmc_amd.de_callback(x0, f, s, mcmc_amd.de_settings(n_pop=n_pop))
    assert mcmc_amd.last_kernel() == "de_literal_kernel"
    rd, _, racc = de_ref.de_ref(f, x0, n_pop, 3, 4, seed=4, lower=lower, upper=upper)
    assert np.array_equal(draws, rd) and n_acc == racc
