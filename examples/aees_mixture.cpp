// aees_mixture.cpp -- a two-component Gaussian mixture in two dimensions, sampled with mcmc::aees (adaptive equi-energy sampling).
//
// The flow of the reference's AEES example: components at (-2, -2) and (2, 2) with variance 0.1 and equal weights, every run started in
// the first one; temperatures (60, 9) above T = 1, 11 energy rings, equi-energy probability 0.05, proposal covariance 0.35 I, 1000
// initial, 1000 burn-in and 20000 kept draws.  Three ways:
//   - the device target (mcmc::mi355x::gaussian_mixture): N independent runs in one launch (N = argv[1], default 1024);
//   - a host callback: one run, the sampler on the GPU, the log density on the host;
//   - mcmc::rwmh with the same callback, start and proposal, for comparison: a plain random walk at T = 1 stays in its mode.
// Each prints the share of kept draws in the far component (x_0 > 0) and the mean of each component.
//
//   g++ -std=c++17 -O2 -Iinclude examples/aees_mixture.cpp -Lmcmc_amd -lmi_mcmc -Wl,-rpath,$PWD/mcmc_amd -o aees_mixture
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mcmc.hpp"

struct mixture_t {
    size_t d, M;
    std::vector<double> means;      // M x d row-major
    std::vector<double> var;        // M
    std::vector<double> weight;     // M
};

// log of sum_i w_i N(x; mu_i, s2_i I)
static double mixture_log_density(const mcmc::ColVec_t& x, void* data)
{
    const mixture_t* m = static_cast<const mixture_t*>(data);
    const double two_pi = 6.283185307179586;
    double dens = 0.0;
    for (size_t i = 0; i < m->M; ++i) {
        double dist = 0.0;
        for (size_t j = 0; j < m->d; ++j) {
            const double df = x(j) - m->means[i * m->d + j];
            dist += df * df;
        }
        dens += m->weight[i] * std::exp(-0.5 * dist / m->var[i]) / std::pow(two_pi * m->var[i], 0.5 * double(m->d));
    }
    return std::log(dens);
}

struct summary_t { double far, mean_far[2], mean_near[2]; };

// draws: n x (2 C), run c in columns 2c, 2c + 1
static summary_t summarise(const mcmc::Mat_t& draws, size_t C)
{
    summary_t s{0.0, {0.0, 0.0}, {0.0, 0.0}};
    size_t n_far = 0, n_near = 0;
    for (size_t r = 0; r < size_t(draws.rows()); ++r)
        for (size_t c = 0; c < C; ++c) {
            const double x0 = draws(r, 2 * c), x1 = draws(r, 2 * c + 1);
            if (x0 > 0) { ++n_far; s.mean_far[0] += x0; s.mean_far[1] += x1; }
            else { ++n_near; s.mean_near[0] += x0; s.mean_near[1] += x1; }
        }
    for (int j = 0; j < 2; ++j) {
        s.mean_far[j] /= n_far ? double(n_far) : 1.0;
        s.mean_near[j] /= n_near ? double(n_near) : 1.0;
    }
    s.far = double(n_far) / double(n_far + n_near);
    return s;
}

static void report(const char* what, const summary_t& s)
{
    std::printf("%s far=%.4f mean_far=(%.4f, %.4f) mean_near=(%.4f, %.4f)\n", what, s.far, s.mean_far[0], s.mean_far[1], s.mean_near[0],
                s.mean_near[1]);
}

int main(int argc, char** argv)
{
    const size_t n_runs = argc > 1 ? size_t(std::strtoul(argv[1], nullptr, 10)) : 1024;
    mixture_t mix{2, 2, {-2.0, -2.0, 2.0, 2.0}, {0.1, 0.1}, {0.5, 0.5}};

    mcmc::ColVec_t start(2);
    start(0) = mix.means[0];
    start(1) = mix.means[1];
    mcmc::ColVec_t temps(2);
    temps(0) = 60.0;
    temps(1) = 9.0;
    mcmc::Mat_t cov(2, 2);
    cov(0, 0) = 0.35;
    cov(1, 1) = 0.35;

    mcmc::algo_settings_t settings;
    settings.rng_seed_value = 2024;
    settings.aees_settings.n_initial_draws = 1000;
    settings.aees_settings.n_burnin_draws = 1000;
    settings.aees_settings.n_keep_draws = 20000;
    settings.aees_settings.n_rings = 11;
    settings.aees_settings.ee_prob_par = 0.05;
    settings.aees_settings.temper_vec = temps;
    settings.aees_settings.par_scale = 1.0;
    settings.aees_settings.cov_mat = cov;

    // many runs on the device target
    std::vector<double> log_c(mix.M);
    mcmc::mi355x::mixture_log_constants(mix.d, mix.M, mix.weight.data(), mix.var.data(), log_c.data());
    mcmc::mi355x::target_t tgt = mcmc::mi355x::gaussian_mixture(mix.d, mix.M, mix.means.data(), mix.var.data(), log_c.data());
    tgt.n_chains = n_runs;
    mcmc::Mat_t draws;
    if (!mcmc::aees(start, mcmc::mi355x::device_value_kernel, draws, &tgt, settings)) {
        std::printf("aees device ok=0 error=%s\n", tgt.last_error.c_str());
        return 1;
    }
    char what[96];
    std::snprintf(what, sizeof what, "aees device ok=1 runs=%zu n_keep=%zu", n_runs, size_t(draws.rows()));
    report(what, summarise(draws, n_runs));

    // one run with the log density on the host
    mcmc::Mat_t cb_draws;
    if (!mcmc::aees(start, mixture_log_density, cb_draws, &mix, settings)) {
        std::printf("aees callback ok=0 error=%s\n", mcmc::mi355x::last_error().c_str());
        return 1;
    }
    report("aees callback ok=1", summarise(cb_draws, 1));

    // the random walk from the same start with the same proposal
    mcmc::algo_settings_t rw;
    rw.rng_seed_value = 2024;
    rw.rwmh_settings.n_burnin_draws = 1000;
    rw.rwmh_settings.n_keep_draws = 20000;
    rw.rwmh_settings.par_scale = 1.0;
    rw.rwmh_settings.cov_mat = cov;
    mcmc::Mat_t rw_draws;
    if (!mcmc::rwmh(start, mixture_log_density, rw_draws, &mix, rw)) {
        std::printf("rwmh callback ok=0 error=%s\n", mcmc::mi355x::last_error().c_str());
        return 1;
    }
    report("rwmh callback ok=1", summarise(rw_draws, 1));
    return 0;
}
