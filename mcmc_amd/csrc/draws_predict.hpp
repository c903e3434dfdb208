// draws_predict.hpp -- interface of the posterior predictive reducer of a draws slab (draws_predict.hip; the C entry is mi_mcmc_draws_predict in
// draws_api.hip, where the stream's cached workspace lives): p[r][k] = sigmoid(eta[r][k]) of every row r of the target's X at every column
// k = t * C + c of a slab [n_keep][d][C], a Bernoulli replicate yrep[r][k] of it from the counter-based generator, and BOTH folds of the two: over the
// columns per row (draws_waic.hip's order) and over the rows per column (draws_logk.hip's).  The arithmetic and its ONE order are stated in
// include/mi_mcmc.h (mcmc_amd/predict.py repeats it).  The plan is a function of the shape, of where the slab and the target live, of what is asked
// for and of the test hook's grid cap, alone.
#pragma once

#include "draws_product.hpp"

namespace mi {
namespace dpred {

using dprod::TM;
using dprod::TN;
using dprod::TK;
constexpr uint64_t PRED_MAX_D = 65536;
constexpr uint32_t PRED_CHUNK = 2048;                  // mi_mcmc_draws_waic's chunk: the unit of the row fold's order
constexpr size_t PRED_ROWS_LDS_BYTES = (size_t)2 * dprod::STAGE * sizeof(double) + (size_t)TM * sizeof(double);      // two stages; the shift of the row tile
constexpr size_t PRED_COLS_LDS_BYTES = (size_t)2 * dprod::STAGE * sizeof(double);
constexpr uint32_t PRED_COUNT_MAX_GRID = 1024;         // workgroups of the counting kernel, at the most: one piece each

// What is asked for: the per-row outputs need the row kernel, the per-column ones the column kernel
struct PredictWants {
    bool row_stats = false, prob = false, yrep = false;           // p_mean / p_var / rep_freq; the matrices
    bool col_stats = false, summary = false;                      // t_rep / ll_rep / ll_obs; the counts
    bool rows() const { return row_stats || prob || yrep; }
    bool cols() const { return col_stats || summary; }
};

// THE PLAN.  n_chunks = ceil(K / 2048), ldR = 128 ceil(n_rows / 128); X packed once as At [Kp][ldR] (draws_product.hpp) for both kernels.
//   rows: predict_shift_kernel, one thread per (chunk, row): grid n_chunks * ceil(n_rows / 256); predict_rows_kernel, EIGHT waves, one 128-row tile and
//     one chunk per workgroup: grid n_chunks * n_row_tiles, 512 threads, PRED_ROWS_LDS_BYTES; predict_merge_kernel, one thread per row.
//   cols: predict_cols_kernel, four waves and 128 columns per workgroup, all row tiles ascending: grid ceil(K / 128), 256 threads, PRED_COLS_LDS_BYTES;
//     with a summary predict_count_kernel, grid-stride over the columns: count_grid = min(ceil(K / 256), 1024, the cap) workgroups, one piece each.
// Workspace, in bytes from its start (every area 256-byte aligned; an area that is not needed has size 0): the packed matrix; the partials
// [n_chunks][4][ldR] (shift, A, S1, S2); the rows' results [3][ldR] (p_mean, p_var, rep_freq); the columns' results [3][K] (t_rep, ll_rep, ll_obs);
// the pieces [count_grid][3] (uint64); the staged copies of a host target (X; y) and of a host slab; the staged matrices prob and yrep of a host call.
struct PredictPlan {
    uint64_t d = 0, n_rows = 0, C = 0, K = 0;
    uint64_t n_chunks = 0, Kp = 0, ldR = 0, n_row_tiles = 0;
    uint64_t rows_grid = 0, cols_grid = 0, pack_grid = 0, merge_grid = 0, count_grid = 0;
    bool rows = false, cols = false, counts = false;
    size_t o_pack = 0, o_part = 0, o_rowout = 0, o_colout = 0, o_pieces = 0, o_mat = 0, o_y = 0, o_slab = 0, o_prob = 0, o_yrep = 0, bytes = 0;
    size_t mat_doubles = 0, y_doubles = 0;             // what the target holds: X (n_rows * d); y (n_rows, 0 without observations)
};

// grid_cap: the test hook's limit on grid-stride grids, 0 = none
PredictPlan predict_plan(uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t C, bool slab_host, bool target_host, bool has_y, const PredictWants& w, uint64_t grid_cap);
// enqueues the kernels on `st`.  x, mat (X), y (NULL: no observations), prob / yrep (NULL: not asked for): device memory; ws: the workspace.  The rows'
// results go to ws + plan.o_rowout, the columns' to ws + plan.o_colout.  Returns a hipError_t as int (0 = enqueued)
int predict_run(const PredictPlan& plan, const double* x, const double* mat, const double* y, uint64_t seed, void* ws, double* prob, double* yrep, hipStream_t st);
// enqueues the counting kernel: piece g of ws + plan.o_pieces = {#{k : t_rep_k >= t_obs}, #{k : ll_rep_k <= ll_obs_k}, sum_k t_rep_k} over its columns
int predict_count(const PredictPlan& plan, double t_obs, void* ws, hipStream_t st);

}  // namespace dpred
}  // namespace mi
