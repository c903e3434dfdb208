"""C++ drop-in header include/mcmc.hpp: mcmc::hmc / mcmc::rwmh on the device route with vals_bound beyond d = 512 run on the matrix-product samplers
(mcmc_amd/csrc/gemm_samplers.hip); mi_mcmc_last_kernel() says so, and the draws lie inside the bounds.  Builds on the CPU; runs on the GPU."""
import os
import re
import subprocess

import pytest

import mcmc_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <limits>
#include <vector>
#include "mcmc.hpp"
#include "mi_mcmc.h"

static int outside(const mcmc::Mat_t& dr, const mcmc::ColVec_t& lo, const mcmc::ColVec_t& hi, size_t d)
{
    int n = 0;                                             // (cols: d x n_chains, dimension-major)
    const size_t C = size_t(dr.cols()) / d;
    for (size_t r = 0; r < size_t(dr.rows()); ++r)
        for (size_t i = 0; i < d; ++i)
            for (size_t c = 0; c < C; ++c) { const double v = dr(r, i * C + c); if (!(v > lo(i) && v < hi(i))) ++n; }
    return n;
}

int main()
{
    const size_t d = 528, C = 96;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> P(d * d, 0.0);
    for (size_t i = 0; i < d; ++i) { P[i * d + i] = 2.0; if (i + 1 < d) { P[i * d + i + 1] = -0.5; P[(i + 1) * d + i] = -0.5; } }
    mcmc::mi355x::target_t tgt = mcmc::mi355x::gaussian_dense(d, P.data());
    tgt.n_chains = C;
    mcmc::ColVec_t init(d), lo(d), hi(d);
    for (size_t i = 0; i < d; ++i) {
        init(i) = 0.001 * double(i % 17);
        lo(i) = (i % 4 == 1 || i % 4 == 3) ? -1.5 : -inf;          // none, lower, upper, both in turn
        hi(i) = (i % 4 == 2 || i % 4 == 3) ? 2.0 : inf;
    }
    mcmc::algo_settings_t s;
    s.rng_seed_value = 11;
    s.vals_bound = true; s.lower_bounds = lo; s.upper_bounds = hi;
    s.hmc_settings.step_size = 0.01; s.hmc_settings.n_leap_steps = 4;      // (the oracle accepts 12 of chain 0's 20 kept draws at 0.01, none at 0.03)
     s.hmc_settings.n_burnin_draws = 10; s.hmc_settings.n_keep_draws = 20;
    s.rwmh_settings.par_scale = 0.02; s.rwmh_settings.n_burnin_draws = 10; s.rwmh_settings.n_keep_draws = 20;
    mcmc::Mat_t dr;
    bool ok = mcmc::hmc(init, mcmc::mi355x::device_kernel, dr, &tgt, s);
    std::printf("device hmc ok=%d rows=%zu cols=%zu acc0=%.3f outside=%d kernel=[%s] %s\n", int(ok), size_t(dr.rows()), size_t(dr.cols()),
                double(s.hmc_settings.n_accept_draws) / 20.0, ok ? outside(dr, lo, hi, d) : -1, mi_mcmc_last_kernel(), ok ? "" : mcmc::mi355x::last_error().c_str());
    if (!ok) return 1;
    ok = mcmc::rwmh(init, mcmc::mi355x::device_value_kernel, dr, &tgt, s);
    std::printf("device rwmh ok=%d rows=%zu cols=%zu acc0=%.3f outside=%d kernel=[%s] %s\n", int(ok), size_t(dr.rows()), size_t(dr.cols()),
                double(s.rwmh_settings.n_accept_draws) / 20.0, ok ? outside(dr, lo, hi, d) : -1, mi_mcmc_last_kernel(), ok ? "" : mcmc::mi355x::last_error().c_str());
    return ok ? 0 : 1;
}
"""


def _build(tmp_path):
    src = tmp_path / "bounds_frontend.cpp"
    src.write_text(SRC)
    exe = str(tmp_path / "bounds_frontend")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT}/include", str(src),
                           f"-L{ROOT}/mcmc_amd", "-lmi_mcmc", f"-Wl,-rpath,{ROOT}/mcmc_amd", "-o", exe])
    return exe


def test_program_with_bounds_compiles_against_the_header(tmp_path):
    if not os.path.exists(mcmc_amd.LIB_PATH):
        pytest.skip("libmi_mcmc.so not built")
    _build(tmp_path)


@pytest.mark.gpu
def test_cpp_front_end_with_bounds_runs_on_the_matrix_product_route(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    for algo in ("hmc", "rwmh"):      # (cols: d x n_chains = 528 x 96)
        m = re.search(rf"device {algo} ok=1 rows=20 cols=50688 acc0=(\S+) outside=0 kernel=\[(.*?)\]", out.stdout)
        assert m, out.stdout
        assert 0.0 < float(m.group(1)) <= 1.0, out.stdout
        assert m.group(2).startswith("gemm_step_kernel<") and "bounds" in m.group(2), out.stdout
