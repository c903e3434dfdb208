// draws_rank.hpp -- interface of the rank transform of a draws slab (draws_rank.hip; the C entries are mi_mcmc_draws_rank_transform and
// mi_mcmc_draw_stats_ranked in mi_mcmc.hip, where the stream's cached workspace lives): for every retained sample of a slab [n_keep][d][C] its exact
// average rank among the S retained samples of its dimension, or the normal score of that rank, by a full sort of the dimension's 64-bit keys
// (least-significant-digit radix sort, 8-bit digits, at most eight stable passes) and a two-level search of every sample in the sorted image.  The
// key, the order, the rank and the score are stated in include/mi_mcmc.h.  Every count is an integer and a sorted image is unique, so the plan below
// decides time and memory only, never a bit of the result; it is a function of (n_keep, C, flags, the budget) alone.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mi {
namespace drank {

constexpr uint64_t RANK_MAX_D = 65536;
constexpr uint32_t RANK_TILE = 16384;                  // keys of one count / scatter workgroup: 4 waves x 64 chunks of 64 keys
constexpr uint32_t RANK_SMALL_C = 512;                 // rows shorter than this are walked flattened, with 8-byte loads (as SEL_SMALL_C)
constexpr uint32_t RANK_STRIDE = 4096;                 // the lookup keeps every RANK_STRIDE-th sorted key of its dimension in LDS ...
constexpr uint32_t RANK_MAX_SAMPLES = 4096;            // ... at most this many (32 KB); beyond S = 2^24 the stride doubles until they fit
constexpr uint32_t RANK_LOOKUP_ELEMS = 16384;          // output elements of one lookup workgroup
constexpr uint64_t RANK_MAX_BLOCKS = 1ull << 22;       // workgroups of one count / scatter launch
constexpr size_t RANK_WS_BUDGET = (size_t)2 << 30;     // bytes of key images, counts and (stats) composed slab of one group of dimensions

constexpr uint32_t RANK_SPLIT = 1u, RANK_FOLD = 2u;    // MI_RANK_SPLIT, MI_RANK_FOLD
constexpr int RANK_AVERAGE = 0, RANK_NORMAL = 1;       // MI_RANK_AVERAGE, MI_RANK_NORMAL

// THE PLAN.  h = floor(n_keep / 2); the retained rows are all n_keep of them, or with RANK_SPLIT the 2 h rows t < h and t >= n_keep - h;
// S = rows * C keys per dimension, key s = r * C + c of retained row r; n_tiles = ceil(S / RANK_TILE).
// GROUP RULE.  A dimension takes
//   dim_bytes = 2 * 8 * S                      two key images
//             + 4 * 256 * n_tiles              the per-tile digit counts of a pass, scanned in place
//             + 4 * 8 * 256                    the digit histograms of all eight passes (which passes can be skipped)
//             + (slab ? 8 * S : 0)             mi_mcmc_draw_stats_ranked only: the composed slab [h][dims][2C] the existing reducer reads
// and the dimensions are processed in consecutive groups of
//   dims_per_group = min(d, max(1, min(budget / dim_bytes, RANK_MAX_BLOCKS / n_tiles)))        (integer divisions)
// with budget = RANK_WS_BUDGET, or what the test hook mi_mcmc_test_set_rank_ws_bytes set.  n_groups = ceil(d / dims_per_group).
struct RankPlan {
    uint64_t n_keep = 0, d = 0, C = 0;
    uint32_t flags = 0;
    uint64_t h = 0, rows = 0, S = 0, n_tiles = 0;
    uint32_t stride = 0, n_samples = 0;                // of the lookup's first level
    uint64_t dim_bytes = 0, dims_per_group = 0, n_groups = 0;
    // workspace, in bytes from its start: the medians [d] and the two tail quantiles [2][d] (doubles, uploaded), the gathered order statistics
    // [8][dims_per_group], the histograms [dims_per_group][8][256] u32, the counts [dims_per_group][256][n_tiles] u32, the two key images
    // [dims_per_group][S] u64, the composed slab [rows / (split ? 2 : 1)][dims_per_group][(split ? 2 : 1) C] doubles
    size_t o_med = 0, o_q = 0, o_os = 0, o_hist = 0, o_cnt = 0, o_img0 = 0, o_img1 = 0, o_slab = 0, bytes = 0;
};

uint64_t rank_dim_bytes(uint64_t n_keep, uint64_t C, uint32_t flags, bool slab);
RankPlan rank_plan(uint64_t n_keep, uint64_t d, uint64_t C, uint32_t flags, bool slab, uint64_t budget /* 0: RANK_WS_BUDGET */);

// Every function enqueues on `st` (and, where it says so, waits for it); returns a hipError_t as int.  x: the slab on the device; ws: plan.bytes.
// Sorts the keys of dimensions [dim0, dim0 + nd): fold = false the keys of x, fold = true those of |x - med_i| (med at ws + o_med, on the device
// already).  Waits ONCE, for the eight digit histograms, and skips the passes whose digit is one value in every dimension of the group.
// *sorted: the image that holds the result, [nd][S].
int rank_sort_group(const double* x, const RankPlan& p, uint64_t dim0, uint64_t nd, bool fold, void* ws, hipStream_t st, const uint64_t** sorted);
// out element of retained sample (r, c) of dimension dim0 + dl: out[(r' * out_d + out_dim0 + dl) * C' + c'], the layout of include/mi_mcmc.h
// with out_d dimensions per row (the whole slab: out_d = d, out_dim0 = dim0; the composed slab of a group: out_d = nd, out_dim0 = 0)
int rank_lookup_group(const double* x, const RankPlan& p, uint64_t dim0, uint64_t nd, bool fold, int what, const uint64_t* sorted, void* ws, double* out,
                      uint64_t out_d, uint64_t out_dim0, hipStream_t st);
// os_host[a * nd + dl] = the value of the ranks[a]-th smallest key of dimension dim0 + dl, a < 8, out of the sorted image; waits for the stream
int rank_order_stats_group(const RankPlan& p, uint64_t nd, const uint64_t* sorted, const uint64_t ranks[8], void* ws, double* os_host, hipStream_t st);
// slab element = x <= q[which][dim] ? 1.0 : 0.0, a NaN x: the canonical quiet NaN; q at ws + o_q, split layout as above
int rank_indicator_group(const double* x, const RankPlan& p, uint64_t dim0, uint64_t nd, int which, void* ws, double* out, hipStream_t st);

// the sorts (one per group of dimensions and kind of key) and the passes they executed so far: process-wide, monotonic; what a test of the skipped
// passes reads
void rank_counts(uint64_t* sorts, uint64_t* passes);

}  // namespace drank
}  // namespace mi
