// draws_product.hpp -- the product stage that draws_logk.hip, draws_waic.hip and draws_predict.hip share: X . Theta (or P . Theta) of a matrix and the K = n_keep * C columns of a
// draws slab [n_keep][d][C], which the first folds over the rows and the second over the columns.  The matrix is packed once per call, TRANSPOSED and
// zero-padded, as At [Kp][ld] -- At[j][i] = M[i][j]: a row of At holds, for one contraction index j, the 128 output rows of a tile contiguously.  A staged
// step is 16 contraction entries: rows 0..15 of a stage are At's 16 rows of the tile, by 16-byte direct-to-LDS loads (issue_a below, as gemm_step_kernel
// stages them); rows 16..31 are the same 16 entries of 128 columns of the slab, through registers (8-byte loads: a row of the slab is 16-byte aligned
// only for an even C), one column per thread with its own base and the common stride C.  Element (i, k) of the product is ONE fma chain over j ascending.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "det_math.hpp"

namespace mi {
namespace dprod {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr double LOG_2PI = 1.83787706640934548356;     // MCMC_LOG_2PI (settings_host.hpp)
constexpr uint32_t TM = 128;                           // output rows (dimensions i / data rows r) of a tile of the product
constexpr uint32_t TN = 128;                           // columns of a tile: 32 per wave
constexpr uint32_t TK = 16;                            // contraction entries per staged step
constexpr uint32_t LDS_STRIDE = 144;                   // doubles per staged row (gemm_samplers.hip: the two 16-lane groups of a fragment read on disjoint bank halves)
constexpr int STAGE = 2 * (int)TK * (int)LDS_STRIDE;   // doubles per stage: rows 0..15 of At's tile, rows 16..31 the columns

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// M (rows x cols, row-major, device memory) -> At[j * ld + i] = M[i][j] for j < Kp, i < ld, zeros outside the matrix, enqueued on st with
// grid = min(ceil(Kp * ld / 256), 65536) workgroups (the plans' pack_grid).  Returns a hipError_t as int.  Defined in draws_logk.hip
int pack_transposed(const double* M, uint64_t rows, uint64_t cols, uint64_t Kp, uint64_t ld, uint64_t grid, double* At, hipStream_t st);

// term_r of the logistic definition: y_r eta_r - softplus(eta_r) (softplus: gemm_rowterm_kernel's two branches, det_math.hpp)
__device__ __forceinline__ double logit_term(double yv, double eta)
{
    const double ex = det_exp(eta > 0.0 ? -eta : eta);
    const double l1p = det_log(1.0 + ex);
    const double sp = (eta > 0.0) ? (eta + l1p) : l1p;
    return yv * eta - sp;
}

// Rows row0 .. row0 + 15 of At, columns col0 .. col0 + 127, into rows 0..15 of stage `stage` of the LDS at byte address lds_base: wave w of the WAVES
// that share the step moves rows w, w + WAVES, ..., 1 KiB each (inside At for every staged step and tile of the plan); lane16 = 16 * lane
template <int WAVES>
__device__ __forceinline__ void issue_a(const double* At, uint64_t ld, uint32_t row0, uint64_t col0, uint32_t lds_base, int stage, int wave, uint32_t lane16)
{
#pragma unroll
    for (int i = 0; i < (int)TK / WAVES; ++i) {
        const int r = wave + WAVES * i;
        const double* src = At + ((uint64_t)(row0 + r) * ld + col0);
        const uint32_t dst = lds_base + (uint32_t)((stage * STAGE + r * (int)LDS_STRIDE) * 8);
        uint32_t m0_saved;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                     : "=&s"(m0_saved) : "v"(lane16), "s"(dst), "s"(src) : "memory");
    }
}

// The columns' 16 rows of step kb: the thread stages rows j0 .. j0 + ROWS - 1 (j0 = 16 kb + ROWS * part) of the column whose base is col, in two halves,
// load_b one step ahead and store_b behind the MFMAs.  (d <= 65 536 and C < 2^32: 32-bit factors.)  The loads are unconditional -- no branch per element,
// and the direct-to-LDS loads issued right behind them keep them where they are: a step whose 16 rows all exist (a uniform test) takes them as they are;
// the ragged last step loads row min(j, d - 1) and, on the way to LDS, REPLACES what lies beyond d by a TRUE zero, whatever was loaded (0 * inf in a
// padded slot would poison the column).  A column beyond K is given the slab's first column as its base, a place that exists, instead of a wild one;
// its product is garbage that nothing folds or stores (an MFMA column touches no other column)
template <int ROWS>
__device__ __forceinline__ void load_b(const double* col, uint32_t kb, int part, uint32_t d32, uint64_t C, double (&v)[ROWS])
{
    const uint32_t C32 = (uint32_t)C;
    const uint32_t j0 = kb * TK + (uint32_t)(ROWS * part);
    if (kb * TK + TK <= d32) {
        const double* bp = col + (uint64_t)j0 * (uint64_t)C32;
#pragma unroll
        for (int u = 0; u < ROWS; ++u) v[u] = bp[(uint64_t)u * C];
    } else {
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
            const uint32_t jj = j0 + (uint32_t)u;
            const uint32_t jc = jj < d32 ? jj : d32 - 1u;
            v[u] = col[(uint64_t)jc * (uint64_t)C32];
        }
    }
}
// stage: the stage's first double; c: the column's place in the tile (0..127)
template <int ROWS>
__device__ __forceinline__ void store_b(double* stage, uint32_t kb, int part, int c, uint32_t d32, const double (&v)[ROWS])
{
    double* dst = stage + ((int)TK + ROWS * part) * (int)LDS_STRIDE + c;
    if (kb * TK + TK <= d32) {
#pragma unroll
        for (int u = 0; u < ROWS; ++u) dst[u * (int)LDS_STRIDE] = v[u];
    } else {
        const uint32_t j0 = kb * TK + (uint32_t)(ROWS * part);
#pragma unroll
        for (int u = 0; u < ROWS; ++u) dst[u * (int)LDS_STRIDE] = (j0 + (uint32_t)u < d32) ? v[u] : 0.0;
    }
}

// One staged step on the matrix cores: the four k-steps of v_mfma_f64_16x16x4_f64 into RB row blocks x 2 column tiles.  As / Bs: the lane's first
// element of the stage's matrix rows / column rows (row lane >> 4, place lane & 15 of the wave's first row block / column tile)
template <int RB>
__device__ __forceinline__ void mfma_step(const double* As, const double* Bs, double4_t (&acc)[RB][2])
{
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        double a[RB], b[2];
#pragma unroll
        for (int t = 0; t < RB; ++t) a[t] = As[4 * kk * (int)LDS_STRIDE + 16 * t];
#pragma unroll
        for (int t = 0; t < 2; ++t) b[t] = Bs[4 * kk * (int)LDS_STRIDE + 16 * t];
#pragma unroll
        for (int ti = 0; ti < RB; ++ti)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[ti][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[ni], acc[ti][ni], 0, 0, 0);
    }
}

// v + the values of the lanes c16 ^ 8, ^ 4, ^ 2, ^ 1 in turn: the tree ((0..7) + (8..15)), ... of the 16 column lanes, in every lane
__device__ __forceinline__ double tree16(double v)
{
    v = v + __shfl_xor(v, 8);
    v = v + __shfl_xor(v, 4);
    v = v + __shfl_xor(v, 2);
    v = v + __shfl_xor(v, 1);
    return v;
}

// (q0 + q2) + (q1 + q3) of the four lane groups' values of column lane & 15, in every lane
__device__ __forceinline__ double combine4(double q, int c16)
{
    const double q0 = __shfl(q, c16), q1 = __shfl(q, c16 + 16), q2 = __shfl(q, c16 + 32), q3 = __shfl(q, c16 + 48);
    return (q0 + q2) + (q1 + q3);
}

}  // namespace dprod
}  // namespace mi
