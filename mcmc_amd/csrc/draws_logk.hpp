// draws_logk.hpp -- interface of the log-kernel reducer of a draws slab (draws_logk.hip; the C entry is mi_mcmc_draws_log_kernel in draws_api.hip, where
// the stream's cached workspace lives): out[t][c] = log K(x[t][:][c]) for every column of a slab [n_keep][d][C].  The arithmetic is stated in
// include/mi_mcmc.h and has ONE order for every shape, so the plan below decides time and memory only, never a bit of the result; it is a function of
// (kind, d, n_rows, n_keep, C) and of where the slab and the target live (what is staged) alone.
#pragma once

#include "draws_product.hpp"

namespace mi {
namespace dlogk {

using dprod::TM;              // the tiles of the product (draws_product.hpp): a workgroup owns TN = 128 columns, 32 per wave, for ALL rows
using dprod::TN;
using dprod::TK;
constexpr uint64_t LOGK_MAX_D = 65536;
constexpr size_t LOGK_LDS_BYTES = (size_t)2 * dprod::STAGE * sizeof(double);      // two stages of 16 matrix rows and 16 column rows

// the kinds are mi_target_kind's values
enum : int { LOGK_ISO = 1, LOGK_DIAG = 2, LOGK_DENSE = 3, LOGK_LOGISTIC = 4, LOGK_NORMAL_MODEL = 5 };
enum : int { LOGK_ROUTE_ELEMENTWISE = 0, LOGK_ROUTE_PRODUCT = 1 };

// THE PLAN.  The samples are the K = n_keep * C columns k = t * C + c.
//   ISO / DIAG / NORMAL_MODEL (elementwise): one lane per column, 256 columns per workgroup: grid = ceil(K / 256).
//   DENSE / LOGISTIC (product): the matrix (P, or X) is packed once per call, TRANSPOSED and zero-padded, as [Kp][ldA] with Kp = 16 ceil(d / 16) the
//     contraction extent and ldA = 128 ceil(rows / 128) the padded output rows (rows = d, or n_rows); a workgroup of four waves owns 128 columns and walks
//     the n_row_tiles = ldA / 128 row tiles ascending, Kp / 16 staged steps each: grid = ceil(K / 128), LOGK_LDS_BYTES of LDS.
// Workspace, in bytes from its start (every area 256-byte aligned; an area that is not needed has size 0): the packed matrix; the staged copies of a
// host target (mat: prec or X; y) and of a host slab; the staged result of a host call.
struct LogkPlan {
    int kind = 0, route = 0;
    uint64_t d = 0, n_rows = 0, C = 0, K = 0;
    uint64_t Kp = 0, ldA = 0, n_row_tiles = 0;
    uint64_t grid = 0, pack_grid = 0;
    uint32_t block = 256;
    size_t lds_bytes = 0;
    size_t o_pack = 0, o_mat = 0, o_y = 0, o_slab = 0, o_out = 0, bytes = 0;
    size_t mat_doubles = 0, y_doubles = 0;             // what the target holds: prec (d, or d * d) or X (n_rows * d); y (n_rows)
};

LogkPlan logk_plan(int kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t C, bool slab_host, bool target_host);
// enqueues the kernels on `st`.  x, mat (prec / X), y, out: device memory; ws: the workspace (the packed matrix goes to ws + plan.o_pack).
// Returns a hipError_t as int (0 = enqueued)
int logk_run(const LogkPlan& plan, const double* x, const double* mat, const double* y, void* ws, double* out, hipStream_t st);
// the two halves of logk_run for a caller that evaluates several slabs under one target (the plans of one (kind, d, n_rows) share Kp, ldA and o_pack):
// the pack of the matrix into ws + plan.o_pack (nothing on the elementwise route), and the evaluation of a slab over a matrix packed before
int logk_pack(const LogkPlan& plan, const double* mat, void* ws, hipStream_t st);
int logk_run_packed(const LogkPlan& plan, const double* x, const double* mat, const double* y, void* ws, double* out, hipStream_t st);

}  // namespace dlogk
}  // namespace mi
