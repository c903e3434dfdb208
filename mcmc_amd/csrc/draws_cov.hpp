// draws_cov.hpp -- interface of the pooled covariance reducer (draws_cov.hip; the C entry is mi_mcmc_draws_covariance in mi_mcmc.hip, where the
// stream's cached workspace lives): mean [d] and cov [d][d] of the K = n_keep * C columns of a slab [n_keep][d][C], cov = E E^T / (K - 1) as an fp64
// rank-K update on the matrix cores.  The arithmetic and every reduction order are stated in include/mi_mcmc.h; the plan below IS that statement's
// chunking rule, a function of (n_keep, d, C) alone.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mi {
namespace dcov {

constexpr uint64_t COV_MAX_D = 65536;      // 512 x 512 output tiles: the grid index stays far inside 32 bits

struct CovPlan {
    uint64_t K = 0;                        // samples: n_keep * C
    // the mean: G groups of `seg` consecutive samples per dimension
    uint64_t G = 0, seg = 0;
    // the products: T x T output tiles of 128 x 128, the n_pairs with tj <= ti; n_chunks chunks of KC consecutive samples
    uint32_t T = 0, n_pairs = 0;
    uint64_t KC = 0, n_chunks = 0;
    // workspace, in doubles from its start: [G][d] group sums, [d] mean, [n_chunks][n_pairs][128 * 128] chunk partials, [d][d] cov
    size_t o_gsum = 0, o_mean = 0, o_part = 0, o_cov = 0, bytes = 0;
};

CovPlan cov_plan(uint64_t n_keep, uint64_t d, uint64_t C, bool want_cov);
// enqueues the kernels on `st` (x: the slab on the device; ws: plan.bytes of device memory); returns a hipError_t as int (0 = enqueued)
int cov_run(const double* x, uint64_t d, uint64_t C, const CovPlan& plan, void* ws, bool want_cov, hipStream_t st);

}  // namespace dcov
}  // namespace mi
