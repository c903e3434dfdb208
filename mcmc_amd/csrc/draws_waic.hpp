// draws_waic.hpp -- interface of the per-observation reducer of a draws slab (draws_waic.hip; the C entry is mi_mcmc_draws_waic in draws_api.hip, where
// the stream's cached workspace lives): the pointwise log-likelihood ll[r][k] of every data row r at every column k = t * C + c of a slab [n_keep][d][C],
// folded over the COLUMNS per row into lppd_r and p_waic_r -- the other fold of the product that draws_logk.hip folds over the rows.  The arithmetic and
// its ONE order are stated in include/mi_mcmc.h; the constants below are part of that statement (mcmc_amd/waic.py repeats them).  The plan is a
// function of (kind, d, n_rows, n_keep, C), of where the slab and the target live and of whether the matrix ll is asked for, alone.
#pragma once

#include "draws_product.hpp"

namespace mi {
namespace dwaic {

using dprod::TM;              // the tiles of the product (draws_product.hpp): a row tile of TM = 128 is two halves of 64, a wave holds 64 rows
using dprod::TN;
using dprod::TK;
constexpr uint64_t WAIC_MAX_D = 65536;
constexpr uint32_t WAIC_CHUNK = 2048;                  // columns of a chunk: the unit of the fold's order, and of a partial
constexpr uint32_t WAIC_SLOTS = 64;                    // running sums per (chunk, row): slot(o) = 16 ((o mod 128) div 32) + o mod 16 of column offset o
constexpr uint32_t WAIC_NORMAL_ROWS = 16;              // rows of a workgroup of the elementwise route
constexpr size_t WAIC_LDS_BYTES = (size_t)2 * dprod::STAGE * sizeof(double) + (size_t)2 * TM * sizeof(double);      // two stages; y and the shift of the row tile

// the kinds are mi_target_kind's values
enum : int { WAIC_LOGISTIC = 4, WAIC_NORMAL_MODEL = 5 };
enum : int { WAIC_ROUTE_ELEMENTWISE = 0, WAIC_ROUTE_PRODUCT = 1 };

// THE PLAN.  n_chunks = ceil(K / 2048) chunks of columns, ldR = 128 ceil(n_rows / 128) padded rows.
//   LOGISTIC (product): X packed as At [Kp][ldR] (draws_product.hpp); a workgroup of EIGHT waves owns one 128-row tile and one chunk and walks the
//     chunk's column tiles of 128 ascending, Kp / 16 staged steps each: grid = n_chunks * n_row_tiles (the row tile runs fastest: neighbours share the
//     chunk's columns), 512 threads, WAIC_LDS_BYTES of LDS.  Before it, one thread per (chunk, row) forms the chunk's shift: grid (ceil(n_rows / 256), n_chunks).
//   NORMAL_MODEL (elementwise): a workgroup of four waves owns 16 rows and one chunk: grid = n_chunks * ceil(n_rows / 16), 256 threads.
//   Both: the partials [n_chunks][4][ldR] (shift, A, S1, S2) and a merge kernel, one thread per row, the chunks ascending: grid = ceil(n_rows / 256).
// Workspace, in bytes from its start (every area 256-byte aligned; an area that is not needed has size 0): the packed matrix; the partials; lppd and
// p_waic [ldR] each; the staged copies of a host target (X; y) and of a host slab; the staged matrix ll of a host call that asks for it.
struct WaicPlan {
    int kind = 0, route = 0;
    uint64_t d = 0, n_rows = 0, C = 0, K = 0;
    uint64_t n_chunks = 0, Kp = 0, ldR = 0, n_row_tiles = 0;
    uint64_t grid = 0, pack_grid = 0, merge_grid = 0;
    uint32_t block = 0;
    size_t lds_bytes = 0;
    size_t o_pack = 0, o_part = 0, o_lppd = 0, o_pw = 0, o_mat = 0, o_y = 0, o_slab = 0, o_ll = 0, bytes = 0;
    size_t mat_doubles = 0, y_doubles = 0;             // what the target holds: X (n_rows * d); y (n_rows)
};

WaicPlan waic_plan(int kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t C, bool slab_host, bool target_host, bool want_loglik);
// enqueues the kernels on `st`.  x, mat (X), y, loglik (NULL: not asked for): device memory; ws: the workspace; lppd and p_waic go to ws + plan.o_lppd /
// plan.o_pw.  Returns a hipError_t as int (0 = enqueued)
int waic_run(const WaicPlan& plan, const double* x, const double* mat, const double* y, void* ws, double* loglik, hipStream_t st);
// enqueues the merge kernel alone, over chunk partials [n_chunks][4][ldR] that somebody else formed in the order above (draws_loglik.hip): lppd, p_waic [n_rows]
int waic_merge(const double* part, uint64_t n_chunks, uint64_t K, uint64_t n_rows, uint64_t ldR, double* lppd, double* p_waic, hipStream_t st);

}  // namespace dwaic
}  // namespace mi
