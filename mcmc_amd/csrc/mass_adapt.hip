// mass_adapt.hip -- the mass adaptations of the C ABI (include/mi_mcmc.h: mi_mcmc_hmc_run_mass_adapted, _per_chain, mi_mcmc_{hmc,mala}_run_mass_adapted_dense).
// They sit ABOVE the sampler entry points: a schedule of ordinary mi_mcmc_hmc_run / mi_mcmc_mala_run calls chained through draw0, with a mass matrix
// estimated from the chains between them -- the pooled variance and the per-chain variance on the two kernels of this file, the pooled covariance by
// mi_mcmc_draws_covariance, its INV / CHOL_LOWER by host_linalg.hpp (whose memo then answers the part's own factorisation).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "sampler_host.hpp"
#include "det_math.hpp"
#include "host_linalg.hpp"

using namespace mi::host;       // fail, DevBuf (host_common.hpp); check_common, StagedChains, stage_in, stage_out, fill_n_leap (sampler_host.hpp)

extern "C" {

// per-dimension variance of the chains' current states, pooled over the chains: out[d] (host); theta [d][C] in `mem`
namespace {
__global__ __launch_bounds__(256) void pooled_variance_kernel(const double* __restrict__ theta, uint64_t C, double* __restrict__ out)
{
    // one workgroup per dimension: mean, then the centred second moment (two passes, fixed reduction tree)
    __shared__ double red[256];
    const double* row = theta + (size_t)blockIdx.x * C;
    auto block_sum = [&](double v) -> double {
        red[threadIdx.x] = v;
        __syncthreads();
        for (int m = 128; m >= 1; m >>= 1) { if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m]; __syncthreads(); }
        const double r = red[0];
        __syncthreads();
        return r;
    };
    double s = 0.0;
    for (uint64_t c = threadIdx.x; c < C; c += 256) s += row[c];
    const double mean = block_sum(s) / (double)C;
    double q = 0.0;
    for (uint64_t c = threadIdx.x; c < C; c += 256) { const double e = row[c] - mean; q = __builtin_fma(e, e, q); }
    const double var = block_sum(q) / (double)(C > 1 ? C - 1 : 1);
    if (threadIdx.x == 0) out[blockIdx.x] = var;
}
}  // namespace

// The schedule the pooled mass adaptations share (diagonal: mi_mcmc_hmc_run_mass_adapted; dense: mi_mcmc_{hmc,mala}_run_mass_adapted_dense): estimate() fills
// the d x d host matrix M from the chains' current states -- first from initial_vals, then after each of n_windows equal parts of the burn-in --, and every
// part is an ordinary run() with precond_mat = M chained through draw0; the kept draws ride the last part.  leap_total: what n_leapfrogs reports for the run.
namespace {
// the burn-in draws done when the first k of n_parts equal parts are (k = n_parts: all of them)
static uint64_t parts_end(uint64_t n_burnin, uint64_t k, uint64_t n_parts) { return (n_burnin * k) / n_parts; }

int run_mass_adapted_parts(int (*run)(const mi_target*, const mi_settings*, mi_chains*, void*), const mi_target* target, const mi_settings* settings,
                           mi_chains* chains, uint32_t n_windows, const double* M, uint64_t leap_total, void* stream, const std::function<int()>& estimate)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t C = chains->n_chains, n_burnin = settings->n_burnin_draws;
    const uint64_t n_parts = (uint64_t)n_windows + 1;
    uint64_t done = 0;
    int rc = estimate();                                 // from the spread of initial_vals
    if (rc) return rc;
    for (uint64_t part = 0; part < n_parts; ++part) {
        const bool last = part + 1 == n_parts;
        const uint64_t upto = parts_end(n_burnin, part + 1, n_parts);
        mi_settings s_ = *settings;
        s_.precond_mat = M;
        s_.n_burnin_draws = upto - done;
        s_.n_keep_draws = last ? settings->n_keep_draws : 0;
        mi_chains c_ = *chains;
        c_.draw0 = chains->draw0 + done;
        if (!last) { c_.draws = nullptr; c_.n_accept = nullptr; }
        if (s_.n_burnin_draws + s_.n_keep_draws > 0) {
            rc = run(target, &s_, &c_, stream);
            if (rc) return rc;
            HIP_TRY(hipStreamSynchronize(st));           // M (host) is read during the call's staging; the next estimate reads theta
        }
        done = upto;
        if (!last) { rc = estimate(); if (rc) return rc; }
    }
    if (chains->n_leapfrogs) {                           // every part's call reported its own count: the run's total is what the caller gets
        const uint64_t total = leap_total;
        if (chains->mem == MI_MEM_DEVICE) { rc = fill_n_leap(chains->n_leapfrogs, C, total, st); if (rc) return rc; }
        else for (uint64_t c = 0; c < C; ++c) chains->n_leapfrogs[c] = total;
        if (chains->n_leapfrogs_executed) {              // hmc executes what it counts: the same total (the header's "equal to n_leapfrogs")
            if (chains->mem == MI_MEM_DEVICE) { rc = fill_n_leap(chains->n_leapfrogs_executed, C, total, st); if (rc) return rc; }
            else for (uint64_t c = 0; c < C; ++c) chains->n_leapfrogs_executed[c] = total;
        }
    }
    return MI_OK;
}
}  // namespace

int mi_mcmc_hmc_run_mass_adapted(const mi_target* target, const mi_settings* settings, mi_chains* chains, uint32_t n_windows,
                                 double* mass_diag_out, void* stream)
{
    int rc = check_common(target, settings, chains);
    if (rc) return rc;
    if (settings->precond_mat) return fail(MI_ERR_BAD_ARG, "hmc (mass adapted): settings.precond_mat must be NULL, the mass matrix is estimated");
    if (target->kind != MI_TARGET_GAUSS_ISO && target->kind != MI_TARGET_GAUSS_DIAG && target->kind != MI_TARGET_GAUSS_DENSE &&
        target->kind != MI_TARGET_LOGISTIC)
        return fail(MI_ERR_UNSUPPORTED, "hmc (mass adapted): implemented for the Gaussian and the logistic-regression targets (a diagonal precond_mat on the device path)");
    if (chains->n_chains < 2) return fail(MI_ERR_BAD_ARG, "hmc (mass adapted): the mass is pooled over the chains, at least 2 are needed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t d = target->d, C = chains->n_chains;
    std::vector<double> var(d), M(d * d, 0.0), mass(d, 1.0);
    DevBuf var_dev, theta_stage;
    HIP_TRY(var_dev.alloc(d * 8));
    auto estimate = [&]() -> int {                       // mass_i = 1 / pooled variance of dimension i over the chains' current states
        const double* th = chains->theta;
        if (chains->mem == MI_MEM_HOST) {
            if (!theta_stage.p) HIP_TRY(theta_stage.alloc(d * C * 8));
            HIP_TRY(hipMemcpyAsync(theta_stage.p, chains->theta, d * C * 8, hipMemcpyHostToDevice, st));
            th = theta_stage.as<double>();
        }
        hipLaunchKernelGGL(pooled_variance_kernel, dim3((unsigned)d), dim3(256), 0, st, th, C, var_dev.as<double>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(var.data(), var_dev.p, d * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint64_t i = 0; i < d; ++i) {
            const double m = 1.0 / var[i];
            mass[i] = (std::isfinite(m) && m > 0.0) ? m : 1.0;
            M[i * d + i] = mass[i];
        }
        return MI_OK;
    };
    if ((uint64_t)n_windows > settings->n_burnin_draws)
        return fail(MI_ERR_BAD_ARG, "hmc (mass adapted): n_windows = %u exceeds n_burnin_draws = %llu (each re-estimation window needs a draw)", n_windows, (unsigned long long)settings->n_burnin_draws);
    rc = run_mass_adapted_parts(mi_mcmc_hmc_run, target, settings, chains, n_windows, M.data(),
                                (settings->n_burnin_draws + settings->n_keep_draws) * settings->n_leap_steps, stream, estimate);
    if (rc) return rc;
    if (mass_diag_out) std::memcpy(mass_diag_out, mass.data(), d * 8);
    return MI_OK;
}

namespace {
// hmc / mala with a DENSE mass matrix pooled over the chains (include/mi_mcmc.h states the estimate, element by element)
int run_mass_adapted_dense(const char* who, bool hmc, const mi_target* target, const mi_settings* settings, mi_chains* chains, uint32_t n_windows,
                           double* precond_out, void* stream)
{
    if (!target || !settings || !chains) return fail(MI_ERR_BAD_ARG, "null target / settings / chains");
    // the adaptation's own conditions first: they need no device
    if (settings->precond_mat) return fail(MI_ERR_BAD_ARG, "%s (dense mass adapted): settings.precond_mat must be NULL, the mass matrix is estimated", who);
    if (chains->mass_diag) return fail(MI_ERR_BAD_ARG, "%s (dense mass adapted): chains.mass_diag must be NULL, the mass matrix is estimated", who);
    if (chains->n_chains < 2) return fail(MI_ERR_BAD_ARG, "%s (dense mass adapted): the mass is pooled over the chains, at least 2 are needed", who);
    if ((uint64_t)n_windows > settings->n_burnin_draws)
        return fail(MI_ERR_BAD_ARG, "%s (dense mass adapted): n_windows = %u exceeds n_burnin_draws = %llu (each re-estimation window needs a draw)", who, n_windows, (unsigned long long)settings->n_burnin_draws);
    int rc = check_common(target, settings, chains);
    if (rc) return rc;
    if (target->kind != MI_TARGET_GAUSS_ISO && target->kind != MI_TARGET_GAUSS_DIAG && target->kind != MI_TARGET_GAUSS_DENSE &&
        target->kind != MI_TARGET_LOGISTIC)
        return fail(MI_ERR_UNSUPPORTED, "%s (dense mass adapted): implemented for the Gaussian and the logistic-regression targets", who);
    const uint64_t d = target->d, C = chains->n_chains;
    std::vector<double> S(d * d), Sp(d * d), M0, M(d * d), L;
    auto all_finite = [](const std::vector<double>& v) { for (double e : v) if (!std::isfinite(e)) return false; return true; };
    auto estimate = [&]() -> int {
        int rc_ = mi_mcmc_draws_covariance(chains->theta, chains->mem, 1, d, C, nullptr, S.data(), stream);
        if (rc_) return rc_;
        bool ok = all_finite(S);
        for (uint64_t i = 0; ok && i < d; ++i) ok = S[i * d + i] > 0.0;
        if (ok) {
            const double a = (double)C / ((double)C + 5.0), b = 1e-3 * (5.0 / ((double)C + 5.0));      // Stan's shrinkage of a window's covariance
            for (uint64_t e = 0; e < d * d; ++e) Sp[e] = a * S[e];
            for (uint64_t i = 0; i < d; ++i) Sp[i * d + i] = a * S[i * d + i] + b;
            if ((rc_ = host_inverse(Sp.data(), d, M0))) return rc_;
            for (uint64_t i = 0; i < d; ++i)
                for (uint64_t j = 0; j < d; ++j) M[i * d + j] = 0.5 * (M0[i * d + j] + M0[j * d + i]);
            ok = all_finite(M);
            if (ok) {                                    // (memoised for d >= 64: the part's own factorisation is this one)
                if ((rc_ = host_cholesky_lower(M.data(), d, L))) return rc_;
                ok = all_finite(L);
            }
        }
        if (!ok) {                                       // degenerate or non-finite spread: this part runs with M = I
            std::fill(M.begin(), M.end(), 0.0);
            for (uint64_t i = 0; i < d; ++i) M[i * d + i] = 1.0;
        }
        return MI_OK;
    };
    rc = run_mass_adapted_parts(hmc ? mi_mcmc_hmc_run : mi_mcmc_mala_run, target, settings, chains, n_windows, M.data(),
                                hmc ? (settings->n_burnin_draws + settings->n_keep_draws) * settings->n_leap_steps : 0, stream, estimate);
    if (rc) return rc;
    if (precond_out) std::memcpy(precond_out, M.data(), d * d * 8);
    return MI_OK;
}
}  // namespace

int mi_mcmc_hmc_run_mass_adapted_dense(const mi_target* target, const mi_settings* settings, mi_chains* chains, uint32_t n_windows,
                                       double* precond_out, void* stream)
{
    return run_mass_adapted_dense("hmc", true, target, settings, chains, n_windows, precond_out, stream);
}

int mi_mcmc_mala_run_mass_adapted_dense(const mi_target* target, const mi_settings* settings, mi_chains* chains, uint32_t n_windows,
                                        double* precond_out, void* stream)
{
    return run_mass_adapted_dense("mala", false, target, settings, chains, n_windows, precond_out, stream);
}

// per chain and dimension: variance of the chain's own draws of one burn-in part (slab [n][d][C]; two passes, draws ascending),
// regularised as Stan regularises its windows, and inverted: mass [d][C]
namespace {
__global__ __launch_bounds__(256) void chain_mass_estimate_kernel(const double* __restrict__ slab, uint32_t n, uint64_t dC, double* __restrict__ mass)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;      // e = i * C + c: coalesced over the chains
    if (e >= dC) return;
    double s = 0.0;
    for (uint32_t t = 0; t < n; ++t) s = s + slab[(size_t)t * dC + e];
    const double mean = s / (double)n;
    double q = 0.0;
    for (uint32_t t = 0; t < n; ++t) { const double x = slab[(size_t)t * dC + e] - mean; q = __builtin_fma(x, x, q); }
    const double var = q / (double)(n - 1);
    const double reg = ((double)n * var + 5.0e-3) / ((double)n + 5.0);
    const double m = 1.0 / reg;
    mass[e] = (mi::is_finite(m) && m > 0.0) ? m : 1.0;
}
}  // namespace

int mi_mcmc_hmc_run_mass_adapted_per_chain(const mi_target* target, const mi_settings* settings, mi_chains* chains, uint32_t n_windows,
                                           double first_step_size, double* mass_diag_out, void* stream)
{
    int rc = check_common(target, settings, chains);
    if (rc) return rc;
    if (settings->precond_mat) return fail(MI_ERR_BAD_ARG, "hmc (per-chain mass): settings.precond_mat must be NULL, the mass matrices are estimated");
    if (n_windows == 0) return fail(MI_ERR_BAD_ARG, "hmc (per-chain mass): n_windows must be at least 1");
    const uint64_t d = target->d, C = chains->n_chains, n_burnin = settings->n_burnin_draws;
    const uint64_t n_parts = (uint64_t)n_windows + 1;
    if (n_burnin / n_parts < 3)
        return fail(MI_ERR_BAD_ARG, "hmc (per-chain mass): n_burnin_draws = %llu leaves fewer than 3 draws for each of the %llu parts (a chain estimates its variances from the draws of one part)",
                    (unsigned long long)n_burnin, (unsigned long long)n_parts);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // everything runs in device memory; a caller with host buffers gets them staged once, not once per part
    StagedChains sc;
    rc = stage_in(chains, d, settings->n_keep_draws, sc, st);
    if (rc) return rc;
    DevBuf mass, slab;
    HIP_TRY(mass.alloc(d * C * 8));
    uint64_t max_part = 0;
    for (uint64_t part = 0; part + 1 < n_parts; ++part) {
        const uint64_t len = parts_end(n_burnin, part + 1, n_parts) - parts_end(n_burnin, part, n_parts);
        max_part = len > max_part ? len : max_part;
    }
    if (hipMalloc(&slab.p, max_part * d * C * 8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MI_ERR_HIP, "hmc (per-chain mass): no memory for the draws of one burn-in part (%llu x d x C doubles): use more windows",
                    (unsigned long long)max_part);
    }
    uint64_t done = 0;
    for (uint64_t part = 0; part < n_parts; ++part) {
        const bool last = part + 1 == n_parts;
        const uint64_t upto = parts_end(n_burnin, part + 1, n_parts);
        mi_settings s_ = *settings;
        mi_chains c_ = sc.dev;
        c_.draw0 = chains->draw0 + done;
        c_.mass_diag = part == 0 ? nullptr : mass.as<double>();       // part 0: M = I, on the raw target's scale
        if (part == 0 && first_step_size != 0.0) s_.step_size = first_step_size;
        if (last) {
            s_.n_burnin_draws = upto - done; s_.n_keep_draws = settings->n_keep_draws;
        } else {                                                     // the part's draws are what the chain learns from
            s_.n_burnin_draws = 0; s_.n_keep_draws = upto - done;
            c_.draws = slab.as<double>(); c_.n_accept = nullptr;
        }
        if (s_.n_burnin_draws + s_.n_keep_draws > 0) {
            rc = mi_mcmc_hmc_run(target, &s_, &c_, stream);
            if (rc) return rc;
        }
        if (!last) {
            const uint64_t n = upto - done, dC = d * C;
            hipLaunchKernelGGL(chain_mass_estimate_kernel, dim3((unsigned)((dC + 255) / 256)), dim3(256), 0, st, slab.as<double>(), (uint32_t)n, dC, mass.as<double>());
            HIP_TRY(hipGetLastError());
        }
        done = upto;
    }
    rc = fill_n_leap(sc.dev.n_leapfrogs, C, (settings->n_burnin_draws + settings->n_keep_draws) * settings->n_leap_steps, st);
    if (rc) return rc;
    if (mass_diag_out)
        HIP_TRY(hipMemcpyAsync(mass_diag_out, mass.p, d * C * 8, chains->mem == MI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    rc = stage_out(chains, d, settings->n_keep_draws, sc, st);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));                   // mass / slab are ours
    return MI_OK;
}

}  // extern "C"
