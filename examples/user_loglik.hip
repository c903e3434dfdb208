// examples/user_loglik.hip -- WAIC and PSIS-LOO for a model the engine does not know: the caller's own kernel writes the pointwise log-likelihood
// matrix next to the draws, and mi_mcmc_loglik_waic / mi_mcmc_loglik_psis_loo (include/mi_mcmc.h) reduce it where it lies.  This is what a user of a
// user-defined device target (examples/user_target.hip, examples/user_tile_target.hip) does: mi_mcmc_draws_waic and mi_mcmc_draws_psis_loo form the
// matrix from a built-in target only.
//
// The model here is the normal model with unknown mean and standard deviation: a column of the slab [n_keep][2][C] is (mu, sigma), y_r the observations,
//     ll[r][k] = -(0.5 * LOG_2PI + log(sigma)) - (e * e) / (2 * (sigma * sigma)),   e = y_r - mu
// -- on purpose the expression that include/mi_mcmc.h states for MI_TARGET_NORMAL_MODEL, over the engine's deterministic logarithm: this kernel is a second,
// independent producer of the bits of mi_mcmc_draws_waic's loglik_out, which tests/ use.  One thread per column k = t * C + c walks the observations
// and writes ll in MI_LOGLIK_SLAB, [n_keep][n_rows][C]: a draws slab whose "dimensions" are the observations, the lanes contiguous along c.
//
//   hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -Iinclude -shared examples/user_loglik.hip \
//         -Lmcmc_amd -lmi_mcmc -Wl,-rpath,$PWD/mcmc_amd -o libuser_loglik.so
#include <hip/hip_runtime.h>

#include "mi_mcmc.h"
#include "mi_mcmc_engine/det_math.hpp"

namespace {

constexpr double LOG_2PI = 1.83787706640934548356;

__global__ __launch_bounds__(256) void normal_loglik_kernel(const double* __restrict__ draws, const double* __restrict__ y, uint64_t n_keep, uint64_t C, uint64_t n_rows,
                                                            double* __restrict__ ll)
{
    const uint64_t K = n_keep * C;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t t = k / C, c = k % C;
        const double mu = draws[(t * 2 + 0) * C + c], sigma = draws[(t * 2 + 1) * C + c];
        const double base = -(0.5 * LOG_2PI + mi::det_log(sigma)), den = 2.0 * (sigma * sigma);
        for (uint64_t r = 0; r < n_rows; ++r) {
            const double e = y[r] - mu;
            ll[(t * n_rows + r) * C + c] = base - (e * e) / den;
        }
    }
}

}  // namespace

// ll_dev [n_keep][n_rows][C] <- the pointwise log-likelihood of the slab draws_dev [n_keep][2][C] at the observations y_dev [n_rows]; everything on the
// device, enqueued on `stream`.  Returns a hipError_t as int (0 = enqueued)
extern "C" int user_loglik_normal(const double* draws_dev, const double* y_dev, uint64_t n_keep, uint64_t n_chains, uint64_t n_rows, double* ll_dev, void* stream)
{
    const uint64_t K = n_keep * n_chains;
    if (K == 0 || n_rows == 0) return 0;
    const uint64_t blocks = (K + 255) / 256;
    hipLaunchKernelGGL(normal_loglik_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, static_cast<hipStream_t>(stream), draws_dev, y_dev, n_keep,
                       n_chains, n_rows, ll_dev);
    return (int)hipGetLastError();
}

// End to end: the matrix of a device slab, then its WAIC and its PSIS-LOO; the matrix never leaves the device.  waic_summary: {elpd_waic, p_waic, lppd,
// se_elpd}, loo_summary: {elpd_loo, p_loo, lppd, se_elpd_loo, n_bad}, on the host; pareto_k_dev [n_rows] on the device, may be NULL.  Returns an mi_status
extern "C" int user_loglik_normal_compare(const double* draws_dev, const double* y_dev, uint64_t n_keep, uint64_t n_chains, uint64_t n_rows, double* waic_summary,
                                          double* loo_summary, double* pareto_k_dev, void* stream)
{
    double* ll = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&ll), n_keep * n_rows * n_chains * sizeof(double)) != hipSuccess) return MI_ERR_OOM;
    int rc = user_loglik_normal(draws_dev, y_dev, n_keep, n_chains, n_rows, ll, stream) ? MI_ERR_HIP : MI_OK;
    if (rc == MI_OK) rc = mi_mcmc_loglik_waic(ll, MI_LOGLIK_SLAB, MI_MEM_DEVICE, n_rows, n_keep, n_chains, nullptr, nullptr, waic_summary, stream);
    if (rc == MI_OK) rc = mi_mcmc_loglik_psis_loo(ll, MI_LOGLIK_SLAB, MI_MEM_DEVICE, n_rows, n_keep, n_chains, nullptr, pareto_k_dev, nullptr, loo_summary, stream);
    (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));
    (void)hipFree(ll);
    return rc;
}
