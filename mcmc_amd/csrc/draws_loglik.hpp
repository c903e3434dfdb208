// draws_loglik.hpp -- interface of the two reducers of a CALLER-SUPPLIED pointwise log-likelihood matrix (draws_loglik.hip; the C entries are
// mi_mcmc_loglik_waic and mi_mcmc_loglik_psis_loo in draws_api.hip, where the stream's cached workspace lives): what mi_mcmc_draws_waic and
// mi_mcmc_draws_psis_loo compute of the matrix ll[r][k] they form from a built-in target, of a matrix that a kernel of the caller's own wrote -- the way to a
// WAIC and a LOO for user-defined device targets.  Nothing is defined here: the order of the sums is include/mi_mcmc.h's section THE ORDER of
// mi_mcmc_draws_waic, the PSIS arithmetic its section DEFINITION of mi_mcmc_draws_psis_loo; the constants are draws_waic.hpp's and draws_psis.hpp's.
// The plan is a function of (layout, n_rows, n_keep, C), of where the matrix lives, of which entry asks and of the two budgets, alone; it decides time
// and memory, never a bit.
#pragma once

#include "draws_psis.hpp"

namespace mi {
namespace dloglik {

// MI_LOGLIK_ROWS: [n_rows][n_keep][C];  MI_LOGLIK_SLAB: [n_keep][n_rows][C].  ROWS is the slab [1][n_rows][K]: one addressing serves both
enum : int { LOGLIK_ROWS = 0, LOGLIK_SLAB = 1 };
constexpr uint32_t FOLD_WAVES = 4;                     // waves of a fold workgroup: one (row, chunk) each
constexpr uint64_t LOGLIK_MAX_ELEMS = 1ull << 40;      // 8.8 TB of matrix: beyond any device, and what keeps every byte count inside its type

// THE PLAN.  K = n_keep * C; n_chunks = ceil(K / 2048); ldR = 128 ceil(n_rows / 128) padded rows, the leading dimension of the partials the merge reads.
//   loglik_fold_kernel   one WAVE per (row, chunk), the chunk running fastest; a workgroup of FOLD_WAVES waves: grid = ceil(n_rows * n_chunks / 4), 256 threads.
//   dwaic::waic_merge    grid = ceil(n_rows / 256).
//   PSIS only: the matrix IS the slab the sorter takes -- rank = rank_plan(1, n_rows, K) (ROWS) or rank_plan(n_keep, n_rows, C) (SLAB), under the rank
//     budget --, its rows walked in the rank plan's groups of rank.dims_per_group: rank_sort_group, then psis_run_group with `psis` (K, M, m, the body
//     pieces, the tail route under lds_tail and its LDS bytes; the fields of a PsisPlan that describe a target or row groups stay 0).
// Workspace, in bytes from its start (every area 256-byte aligned; an area that is not needed has size 0): lppd and p_waic [ldR] each; the chunk partials
// [n_chunks][4][ldR]; PSIS: elpd_loo and pareto_k [n_rows] each and the body partials [dims_per_group][n_pieces]; the staged copy of a host matrix;
// PSIS: the workspace of rank.
struct LoglikPlan {
    int layout = 0;
    bool psis_entry = false;
    uint64_t n_rows = 0, n_keep = 0, C = 0, K = 0;
    uint64_t slab_C = 0;                               // the slab's row length: K (ROWS) or C (SLAB)
    uint64_t n_chunks = 0, ldR = 0, fold_grid = 0, merge_grid = 0;
    uint32_t fold_block = 0;
    dpsis::PsisPlan psis;
    size_t o_lppd = 0, o_pw = 0, o_part = 0, o_elpd = 0, o_k = 0, o_body = 0, o_mat = 0, o_rank = 0, bytes = 0;
};

LoglikPlan loglik_plan(int layout, uint64_t n_rows, uint64_t n_keep, uint64_t C, bool mat_host, bool psis_entry, uint32_t lds_tail /* 0: PSIS_LDS_TAIL */,
                       uint64_t rank_budget /* 0: RANK_WS_BUDGET */);
// enqueues the fold and the merge on `st`: mat on the device; lppd and p_waic go to ws + plan.o_lppd / plan.o_pw.  Returns a hipError_t as int (0 = enqueued)
int loglik_fold(const LoglikPlan& plan, const double* mat, void* ws, hipStream_t st);
// every row sorted and PSIS-smoothed, group by group: elpd_loo and pareto_k go to ws + plan.o_elpd / plan.o_k.  Waits once per sort group (the sort's)
int loglik_psis(const LoglikPlan& plan, const double* mat, void* ws, hipStream_t st);

}  // namespace dloglik
}  // namespace mi
