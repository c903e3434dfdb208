// draws_psis.hpp -- interface of the PSIS-LOO reducer of a draws slab (draws_psis.hip; the C entry is mi_mcmc_draws_psis_loo in draws_api.hip, where the
// stream's cached workspace lives): per data row r the Pareto-smoothed importance-sampling estimate elpd_loo_r and the fitted shape pareto_k_r, from the
// row's K pointwise log-likelihoods ll[r][:] SORTED.  The rows are walked in groups: draws_waic.hip writes a group's block ll [G][K] (and its lppd),
// draws_rank.hip sorts every row of the block -- the block is a slab [1][G][K] --, and the two kernels here read the sorted key image.  The arithmetic
// and its ONE order are stated in include/mi_mcmc.h; the constants below are part of that statement (mcmc_amd/psis.py repeats them).  The plan is a
// function of (kind, d, n_rows, n_keep, C), of where the slab and the target live and of the two budgets, alone; it decides time and memory, never a bit.
#pragma once

#include "draws_rank.hpp"
#include "draws_waic.hpp"

namespace mi {
namespace dpsis {

constexpr uint64_t PSIS_MIN_K = 25;                    // below it the tail has fewer than five values
constexpr uint32_t PSIS_SLOTS = 256;                   // running sums of SUM: the threads of a workgroup
constexpr uint32_t PSIS_BODY_PIECE = 16384;            // values of one piece of the body fold: one workgroup of psis_body_kernel
constexpr uint32_t PSIS_MAX_FIT = 512;                 // m = 30 + floor(sqrt(M)) <= 473 for K < 2^32
constexpr uint32_t PSIS_LDS_TAIL = 8192;               // exceedances a workgroup keeps in LDS (64 KB); a longer tail is re-read from the sorted image
constexpr size_t PSIS_LL_BYTES = (size_t)4 << 30;      // bytes of the block ll [G][K] of one row group
constexpr double PSIS_LOG_MIN_NORMAL = -708.3964185322641;
constexpr double PSIS_W_MIN = 10.0 * 0x1p-52;

enum : int { PSIS_TAIL_LDS = 0, PSIS_TAIL_GLOBAL = 1 };

// M = min(K div 5, m3), m3 the smallest integer whose square is >= 9 K; m = 30 + floor(sqrt(M)): integers only
uint64_t psis_tail_length(uint64_t K);
uint32_t psis_fit_points(uint64_t M);

// THE PLAN.  K = n_keep * C; M, m as above; the tail route is LDS while M <= lds_tail (PSIS_LDS_TAIL, or what the test hook set, never more).
// ROW GROUPS.  G = min(n_rows, 128 * max(1, ll_bytes div (128 * 8 K))) rows (ll_bytes = PSIS_LL_BYTES, or what the test hook set, never more), consecutive;
// n_groups = ceil(n_rows / G).  A group runs waic = waic_plan(kind, d, its rows, n_keep, C, device, device, with ll) on the sub-target (X + r0 d, y + r0),
// then rank = rank_plan(1, G, K, 0, no slab, the rank budget) sorts the block's rows in ITS groups of rank.dims_per_group, and after each of those
//   psis_body_kernel   grid = rows * n_pieces, 256 threads, n_pieces = ceil((K - M) / PSIS_BODY_PIECE): SUM of one piece of one row's body -> part [row][piece]
//   psis_tail_kernel   grid = rows, 256 threads, lds_bytes = 8 min(M, lds_tail) (LDS route) or 0: the fit, the smoothed tail, the folds, the merge
// Workspace, in bytes from its start (every area 256-byte aligned; an area that is not needed has size 0): the results elpd_loo, pareto_k, lppd
// [n_rows] each; the body partials [G][n_pieces]; the staged copies of a host target (X; y) and of a host slab; the workspace of waic (of the largest
// group); the block ll [G][K]; the workspace of rank.
struct PsisPlan {
    int kind = 0, tail_route = 0;
    uint64_t d = 0, n_rows = 0, n_keep = 0, C = 0, K = 0, M = 0;
    uint32_t m = 0, lds_tail = 0;
    uint64_t G = 0, n_groups = 0, n_pieces = 0;
    size_t lds_bytes = 0;
    dwaic::WaicPlan waic;                              // of a full group; the last, shorter group has its own (no larger)
    drank::RankPlan rank;
    size_t o_elpd = 0, o_k = 0, o_lppd = 0, o_part = 0, o_mat = 0, o_y = 0, o_slab = 0, o_waic = 0, o_ll = 0, o_rank = 0, bytes = 0;
    size_t mat_doubles = 0, y_doubles = 0;
};

PsisPlan psis_plan(int kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t C, bool slab_host, bool target_host, uint64_t ll_bytes /* 0: PSIS_LL_BYTES */,
                   uint32_t lds_tail /* 0: PSIS_LDS_TAIL */, uint64_t rank_budget /* 0: RANK_WS_BUDGET */);
// enqueues the two kernels on `st` for rows [0, nd) of a sorted key image [nd][K]: elpd_loo and pareto_k of row j go to elpd[j], pk[j]; part: [nd][n_pieces].
// Returns a hipError_t as int (0 = enqueued)
int psis_run_group(const PsisPlan& plan, const uint64_t* sorted, uint64_t nd, double* part, double* elpd, double* pk, hipStream_t st);

}  // namespace dpsis
}  // namespace mi
