"""C++ drop-in header include/mcmc.hpp: mcmc::nuts on the device route beyond d = 512 runs on the matrix-product route (mcmc_amd/csrc/gemm_nuts.hpp);
mi_mcmc_last_kernel() says so, and chain 0's draws are the bits of the same call through ctypes.  Builds on the CPU; runs on the GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import mcmc_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, C, KEEP = 520, 8, 4

SRC = r"""
#include <cstdio>
#include <vector>
#include "mcmc.hpp"
#include "mi_mcmc.h"

int main(int argc, char** argv)
{
    const size_t d = 520, C = 8;
    std::vector<double> P(d * d, 0.0);
    for (size_t i = 0; i < d; ++i) { P[i * d + i] = 2.0; if (i + 1 < d) { P[i * d + i + 1] = -0.5; P[(i + 1) * d + i] = -0.5; } }
    mcmc::mi355x::target_t tgt = mcmc::mi355x::gaussian_dense(d, P.data());
    tgt.n_chains = C;
    mcmc::ColVec_t init(d);
    for (size_t i = 0; i < d; ++i) init(i) = 0.01 * double(i % 17) - 0.05;
    mcmc::algo_settings_t s;
    s.rng_seed_value = 11;
    s.nuts_settings.n_burnin_draws = 2; s.nuts_settings.n_keep_draws = 4; s.nuts_settings.n_adapt_draws = 3; s.nuts_settings.max_tree_depth = 4;
    s.nuts_settings.step_size = 0.1;
    mcmc::Mat_t dr;
    const bool ok = mcmc::nuts(init, mcmc::mi355x::device_kernel, dr, &tgt, s);
    std::printf("device nuts ok=%d rows=%zu cols=%zu acc0=%zu kernel=[%s] %s\n", int(ok), size_t(dr.rows()), size_t(dr.cols()), size_t(s.nuts_settings.n_accept_draws),
                mi_mcmc_last_kernel(), ok ? "" : mcmc::mi355x::last_error().c_str());
    if (!ok || argc < 2) return ok ? 0 : 1;
    std::FILE* f = std::fopen(argv[1], "wb");                      // chain 0: columns 0 .. d - 1 of every kept row
    if (!f) return 2;
    for (size_t k = 0; k < size_t(dr.rows()); ++k)
        for (size_t j = 0; j < d; ++j) { const double v = dr(k, j); std::fwrite(&v, sizeof v, 1, f); }
    std::fclose(f);
    return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "nuts_gemm_frontend.cpp"
    src.write_text(SRC)
    exe = str(tmp_path / "nuts_gemm_frontend")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT}/include", str(src),
                           f"-L{ROOT}/mcmc_amd", "-lmi_mcmc", f"-Wl,-rpath,{ROOT}/mcmc_amd", "-o", exe])
    return exe


def test_program_with_nuts_beyond_d512_compiles_against_the_header(tmp_path):
    if not os.path.exists(mcmc_amd.LIB_PATH):
        pytest.skip("libmi_mcmc.so not built")
    _build(tmp_path)


@pytest.mark.gpu
def test_cpp_front_end_nuts_runs_on_the_matrix_product_route(tmp_path):
    exe = _build(tmp_path)
    dump = str(tmp_path / "chain0.bin")
    out = subprocess.run([exe, dump], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(rf"device nuts ok=1 rows={KEEP} cols={D * C} acc0=(\d+) kernel=\[(.*?)\]", out.stdout)
    assert m, out.stdout
    assert m.group(2).startswith("gemm_step_kernel<12, 0>") and "nuts" in m.group(2), out.stdout
    # the same call through ctypes
    P = np.zeros((D, D))
    i = np.arange(D)
    P[i, i] = 2.0
    P[i[:-1], i[:-1] + 1] = -0.5
    P[i[:-1] + 1, i[:-1]] = -0.5
    init = np.tile(0.01 * (i % 17) - 0.05, (C, 1))
    st = mcmc_amd.default_settings(rng_seed_value=11, n_burnin_draws=2, n_keep_draws=KEEP, n_adapt_draws=3, max_tree_depth=4, step_size=0.1)
    draws, info = mcmc_amd.sample("nuts", mcmc_amd.TARGET_GAUSS_DENSE, init, st, prec=P)
    assert mcmc_amd.last_kernel().startswith("gemm_step_kernel<12, 0>")
    assert int(m.group(1)) == int(info["n_accept"][0])
    assert np.array_equal(np.fromfile(dump).reshape(KEEP, D), draws[:, :, 0])
