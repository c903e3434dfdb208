// de_normal_mean.cpp -- posterior of a normal mean with a normal prior, sampled with mcmc::de (differential-evolution MCMC).
//
// The flow of the reference's example program for DE: 100 observations of N(2, 1), prior N(1, 2^2) on the mean, a lambda as the
// log target, 2000 burn-in and 2000 kept generations of the default population (100 members).  The sampler runs on the GPU
// (de_literal_kernel); the lambda runs on the host, asked once per proposal.
//
//   g++ -std=c++17 -O2 -Iinclude examples/de_normal_mean.cpp -Lmcmc_amd -lmi_mcmc -Wl,-rpath,$PWD/mcmc_amd -o de_normal_mean
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "mcmc.hpp"

struct norm_data_t {
    double sigma;
    std::vector<double> x;
    double mu_0, sigma_0;
};

int main()
{
    const int n_data = 100;
    const double mu = 2.0, pi = 3.14159265358979;
    norm_data_t dta{1.0, {}, 1.0, 2.0};
    std::mt19937_64 gen(12345);
    std::normal_distribution<double> dist;
    for (int i = 0; i < n_data; ++i) dta.x.push_back(mu + dist(gen));

    // log likelihood + log prior of the mean
    auto log_target_dens = [pi](const mcmc::ColVec_t& vals_inp, void* ll_data) -> double {
        const norm_data_t* d = static_cast<const norm_data_t*>(ll_data);
        const double m = vals_inp(0);
        double ss = 0.0;
        for (double xi : d->x) ss += (xi - m) * (xi - m);
        const double ll = -double(d->x.size()) * (0.5 * std::log(2 * pi) + std::log(d->sigma)) - ss / (2 * d->sigma * d->sigma);
        const double lp = -0.5 * std::log(2 * pi) - std::log(d->sigma_0) - (m - d->mu_0) * (m - d->mu_0) / (2 * d->sigma_0 * d->sigma_0);
        return ll + lp;
    };

    mcmc::ColVec_t initial_val(1);
    initial_val(0) = 1.0;
    mcmc::algo_settings_t settings;
    settings.rng_seed_value = 7;
    settings.de_settings.n_burnin_draws = 2000;
    settings.de_settings.n_keep_draws = 2000;

    mcmc::Cube_t draws_out;
    const bool ok = mcmc::de(initial_val, log_target_dens, draws_out, &dta, settings);
    if (!ok) {
        std::printf("de ok=0 error=%s\n", mcmc::mi355x::last_error().c_str());
        return 1;
    }

    // the posterior mean over every member and kept generation; its standard error from 20 batches of generations
    const size_t n_keep = draws_out.n_mat(), n_pop = draws_out.mat(0).rows(), n_batch = 20;
    std::vector<double> batch(n_batch, 0.0);
    double mean = 0.0;
    for (size_t k = 0; k < n_keep; ++k)
        for (size_t i = 0; i < n_pop; ++i) {
            mean += draws_out.mat(k)(i, 0);
            batch[k * n_batch / n_keep] += draws_out.mat(k)(i, 0);
        }
    mean /= double(n_keep * n_pop);
    double var_b = 0.0;
    for (double& b : batch) { b /= double(n_keep / n_batch * n_pop); var_b += (b - mean) * (b - mean); }
    const double se = std::sqrt(var_b / double(n_batch - 1) / double(n_batch));

    // conjugate posterior: precision n / sigma^2 + 1 / sigma_0^2
    double sx = 0.0;
    for (double xi : dta.x) sx += xi;
    const double prec = n_data / (dta.sigma * dta.sigma) + 1.0 / (dta.sigma_0 * dta.sigma_0);
    const double post_mean = (sx / (dta.sigma * dta.sigma) + dta.mu_0 / (dta.sigma_0 * dta.sigma_0)) / prec;
    std::printf("de ok=1 n_pop=%zu n_keep=%zu mean=%.6f se=%.6f analytic=%.6f analytic_sd=%.6f accept=%.4f\n", n_pop, n_keep, mean, se, post_mean,
                1.0 / std::sqrt(prec), double(settings.de_settings.n_accept_draws) / double(n_keep * n_pop));
    return 0;
}
