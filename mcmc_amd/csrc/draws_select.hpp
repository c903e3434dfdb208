// draws_select.hpp -- interface of the pooled order-statistics reducer (draws_select.hip; the C entries are mi_mcmc_draws_order_stats and
// mi_mcmc_draws_quantiles in mi_mcmc.hip, where the stream's cached workspace lives): for every dimension of a slab [n_keep][d][C] the values whose keys
// are the ranks[a]-th smallest of its K = n_keep * C keys, by a most-significant-digit radix selection (8-bit digits, 8 rounds).  The key and the
// order are stated in include/mi_mcmc.h.  Every count is an integer, so the plan below decides time and memory only, never a bit of the result; it is a
// function of (n_keep, d, C, n_ranks) alone.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mi {
namespace dsel {

constexpr uint64_t SEL_MAX_D = 65536;
constexpr uint32_t SEL_MAX_RANKS = 32;                 // MI_ORDER_STATS_MAX_RANKS
constexpr uint64_t SEL_TARGET = 16384;                 // elements a histogram workgroup aims at
constexpr uint64_t SEL_SMALL_C = 512;                  // rows shorter than this are walked flattened, with 8-byte loads
constexpr uint64_t SEL_MAX_BLOCKS = 1ull << 22;        // workgroups of one histogram launch
constexpr size_t SEL_HIST_BOUND = (size_t)256 << 20;   // bytes of global histograms and round-1 partials in the workspace

// THE PLAN.  A histogram workgroup owns
//   C >= target:  one of P = ceil(C / target) pieces of one row [t][i][.], piece = ceil(C / P) elements (the last one shorter);
//   C <  target:  rows_per_wg = target / C (integer division) consecutive rows t of one dimension, whole (P = 1);
// with target = max(SEL_TARGET, ceil(K / 2^20)), so a dimension has wg_per_dim = ceil(n_keep / rows_per_wg) * P <= 2^21 + 1 workgroups and a workgroup
// sees at most `target` elements: fewer than 2^32 (its LDS counts are 32-bit) for every K < 2^52, that is for any slab that fits a memory.
// GROUP RULE.  The dimensions are processed in consecutive groups of
//   dims_per_group = min(d, max(1, min(SEL_HIST_BOUND / (n_ranks * 2048 + wg_per_dim * 1024), SEL_MAX_BLOCKS / wg_per_dim)))
// (integer divisions): a dimension takes n_ranks * 256 64-bit counts of global histograms and wg_per_dim * 256 32-bit counts of round-1 partials.
// A group runs its 17 launches (8 x (histogram, scan), 1 inversion) before the next one starts; n_groups = ceil(d / dims_per_group).
struct SelPlan {
    uint64_t K = 0, target = 0;
    uint64_t P = 0, piece = 0, rows_per_wg = 0, wg_per_dim = 0;
    uint64_t dims_per_group = 0, n_groups = 0;
    // workspace, in bytes from its start: two images of the per-(dimension, rank) state [d][n_ranks] {prefix, remaining rank} (the number of fixed
    // bits, 8 per finished round, is the launch's argument); the result [n_ranks][d]; the round-1 partial histograms
    // [dims_per_group][wg_per_dim][256] u32; the global histograms [dims_per_group][n_ranks][256] u64
    size_t o_state0 = 0, o_state1 = 0, o_out = 0, o_part = 0, o_hist = 0, bytes = 0;
};

// the key of include/mi_mcmc.h's ORDER and its inverse (draws_rank.hip sorts by the same key)
__device__ __forceinline__ uint64_t sel_key(double v)
{
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    if ((u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return ~0ull;       // any NaN
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double sel_unkey(uint64_t k)
{
    const uint64_t u = k == ~0ull ? 0x7FF8000000000000ull : ((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k);
    return __longlong_as_double((long long)u);
}

struct SelRanks { uint64_t r[SEL_MAX_RANKS]; };        // travels to the round-1 scan as a kernel argument

SelPlan sel_plan(uint64_t n_keep, uint64_t d, uint64_t C, uint32_t n_ranks);
// enqueues the kernels on `st` (x: the slab on the device; ws: plan.bytes of device memory); returns a hipError_t as int (0 = enqueued)
int sel_run(const double* x, uint64_t n_keep, uint64_t d, uint64_t C, const SelRanks& ranks, uint32_t n_ranks, const SelPlan& plan, void* ws, hipStream_t st);

}  // namespace dsel
}  // namespace mi
