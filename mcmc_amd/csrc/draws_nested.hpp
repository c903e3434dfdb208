// draws_nested.hpp -- interface of the nested R-hat reducer (draws_nested.hip; the C entries are mi_mcmc_draw_stats_nested and
// mi_mcmc_draw_stats_nested_ranked in draws_api.hip, where the stream's cached workspace lives): the C chains of a slab [n_keep][d][C] are K = C / M
// superchains of M consecutive chains; per dimension the variance of the superchain means (between) is compared with the variance inside the
// superchains (within).  The arithmetic and every reduction order are stated in include/mi_mcmc.h; they are functions of (slab, n_keep, d, C, M)
// alone, so the plan below decides memory only.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mi {
namespace dnest {

constexpr uint64_t NESTED_MAX_D = 65536;
constexpr uint32_t NESTED_TILE = 256;      // chains of one chain-moments workgroup: one lane each

struct NestedPlan {
    uint64_t N = 0, d = 0, C = 0, M = 0, K = 0;
    uint64_t n_tiles = 0;                  // ceil(C / NESTED_TILE)
    // workspace, in doubles from its start: the chain means a [d][C] and variances v [d][C], the superchain means A [d][K] and variances w [d][K],
    // mean / between / within [3][d], and (want_super) the superchain means once more as the caller's [K][d]
    size_t o_a = 0, o_v = 0, o_A = 0, o_w = 0, o_out = 0, o_super = 0, bytes = 0;
};

NestedPlan nested_plan(uint64_t n_keep, uint64_t d, uint64_t C, uint64_t M, bool want_super);
// enqueues the three kernels on `st` (x: the slab on the device; ws: plan.bytes of device memory); returns a hipError_t as int (0 = enqueued)
int nested_run(const double* x, const NestedPlan& plan, void* ws, bool want_super, hipStream_t st);

}  // namespace dnest
}  // namespace mi
