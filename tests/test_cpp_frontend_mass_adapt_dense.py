"""C++ drop-in header include/mcmc.hpp: mcmc::mi355x::hmc_mass_adapted_dense / mala_mass_adapted_dense (NOT reference modes) compile, and return the
bits of the C ABI they wrap (mi_mcmc_{hmc,mala}_run_mass_adapted_dense).  Builds on the CPU; runs on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "mcmc.hpp"
#include "mi_mcmc.h"

int main()
{
    const size_t d = 12, C = 64, burn = 12, keep = 5;
    std::vector<double> P(d * d, 0.0);
    for (size_t i = 0; i < d; ++i) { P[i * d + i] = 2.0 + double(i); if (i + 1 < d) { P[i * d + i + 1] = -0.5; P[(i + 1) * d + i] = -0.5; } }
    mcmc::mi355x::target_t tgt = mcmc::mi355x::gaussian_dense(d, P.data());
    tgt.n_chains = C;
    mcmc::ColVec_t init(d * C);
    uint64_t lcg = 12345;                                  // spread-out starts: a small generator, uniform on (-1, 1)
    for (size_t e = 0; e < d * C; ++e) {
        lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
        init(e) = double(lcg >> 11) / 4503599627370496.0 - 1.0;
    }
    int bad = 0;
    for (int algo = 0; algo < 2; ++algo) {
        mcmc::algo_settings_t s;
        s.rng_seed_value = 11;
        s.hmc_settings.step_size = 0.25; s.hmc_settings.n_leap_steps = 5; s.hmc_settings.n_burnin_draws = burn; s.hmc_settings.n_keep_draws = keep;
        s.mala_settings.step_size = 0.4; s.mala_settings.n_burnin_draws = burn; s.mala_settings.n_keep_draws = keep;
        mcmc::Mat_t dr;
        std::vector<double> M;
        const bool ok = algo == 0 ? mcmc::mi355x::hmc_mass_adapted_dense(init, tgt, dr, s, 2, &M)
                                  : mcmc::mi355x::mala_mass_adapted_dense(init, tgt, dr, s, 2, &M);
        if (!ok) { std::printf("front end failed: %s\n", tgt.last_error.c_str()); return 1; }
        // the C ABI, directly
        std::vector<double> theta(d * C), draws(keep * d * C), M2(d * d);
        for (size_t c = 0; c < C; ++c)
            for (size_t j = 0; j < d; ++j) theta[j * C + c] = init(c * d + j);
        mi_settings m;
        mi_settings_default(&m);
        m.rng_seed_value = 11; m.n_burnin_draws = burn; m.n_keep_draws = keep;
        m.n_leap_steps = 5; m.step_size = algo == 0 ? 0.25 : 0.4;
        mi_chains ch{};
        ch.struct_size = sizeof ch; ch.mem = MI_MEM_HOST; ch.n_chains = C; ch.theta = theta.data(); ch.draws = draws.data();
        const int rc = algo == 0 ? mi_mcmc_hmc_run_mass_adapted_dense(&tgt.desc, &m, &ch, 2, M2.data(), nullptr)
                                 : mi_mcmc_mala_run_mass_adapted_dense(&tgt.desc, &m, &ch, 2, M2.data(), nullptr);
        if (rc != MI_OK) { std::printf("C ABI failed: %s\n", mi_mcmc_last_error()); return 1; }
        bool same = M.size() == d * d && std::memcmp(M.data(), M2.data(), d * d * 8) == 0 && size_t(dr.rows()) == keep && size_t(dr.cols()) == d * C;
        bool moved = false;
        for (size_t k = 0; same && k < keep; ++k)
            for (size_t j = 0; j < d; ++j)
                for (size_t c = 0; c < C; ++c) {
                    const double a = dr(k, c * d + j), b = draws[(k * d + j) * C + c];
                    if (std::memcmp(&a, &b, 8) != 0) same = false;
                    if (a != init(c * d + j)) moved = true;
                }
        std::printf("%s same=%d moved=%d M00=%.6g\n", algo == 0 ? "hmc" : "mala", int(same), int(moved), M.empty() ? 0.0 : M[0]);
        if (!same || !moved) bad = 1;
    }
    return bad;
}
"""


def _build(tmp_path):
    src = tmp_path / "mass_adapt_dense_frontend.cpp"
    src.write_text(SRC)
    exe = str(tmp_path / "mass_adapt_dense_frontend")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT}/include", str(src),
                           f"-L{ROOT}/mcmc_amd", "-lmi_mcmc", f"-Wl,-rpath,{ROOT}/mcmc_amd", "-o", exe])
    return exe


def test_program_with_the_dense_mass_adaptations_compiles_against_the_header(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_cpp_front_end_returns_the_bits_of_the_c_abi(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hmc same=1 moved=1" in out.stdout and "mala same=1 moved=1" in out.stdout, out.stdout
