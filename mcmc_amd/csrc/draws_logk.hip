// draws_logk.hip -- the log-kernel value of every column of a draws slab (mi_mcmc_draws_log_kernel; include/mi_mcmc.h states the arithmetic,
// draws_logk.hpp the plan).  The samples are the K = n_keep * C columns k = t * C + c of a slab [n_keep][d][C]: column k starts at element
// (k / C) d C + (k % C) and its row stride is C, for every column -- so a tile of columns may span several t.
//
//   logk_elem_kernel<KIND>      ISO / DIAG / NORMAL_MODEL: one lane per column, coalesced along c, any d; the four strided chains of dot4 in four registers.
//   dprod::pack_kernel          DENSE / LOGISTIC, once per call: the matrix (P: d x d, X: n_rows x d, row-major as given) TRANSPOSED and zero-padded into
//                               At [Kp][ldA] (draws_product.hpp; draws_waic.hip packs its X through the same launcher, defined here).
//   logk_product_kernel<TGT>    the fused product and reduction.  A workgroup of four waves owns 128 columns, a wave 32 of them (two 16-column tiles of
//                               v_mfma_f64_16x16x4_f64) for ALL rows: it walks the row tiles of 128 rows ascending, 16 accumulators (8 row blocks x 2 column
//                               tiles) per row tile, the contraction in steps of 16 through a double-buffered LDS stage, staged as draws_product.hpp
//                               states (a wave moves 4 of At's 16 rows, a thread 8 of its column's), one step ahead.  Element (i, k) of the product is ONE
//                               fma chain over j ascending (the k-steps of an MFMA and the loop both ascend): w_i of the definition, or eta_r.  It never
//                               reaches memory: the C/D map of the instruction,
//                               col = lane & 15, row = (lane >> 4) + 4 reg, gives lane group g = lane >> 4 exactly the rows i = g (mod 4) -- chain g of dot4 /
//                               sum4 -- so after a row tile every lane folds its rows, ascending, into one q per column:
//                                   DENSE     q = fma(x_i, w_i, q)                     (x_i re-read from the slab: the workgroup has just streamed it)
//                                   LOGISTIC  q = q + (y_r eta_r - softplus(eta_r))    (dprod::logit_term)
//                               rows beyond d / n_rows are SKIPPED, not added as zeros (a padded logistic row would add -log 2, and fma(0, 0, -0) is +0).
//                               The fold runs as a rolled loop over the 8 row blocks that rotates the accumulators down by one block per turn (register
//                               moves, ~1 % of a row tile's matrix time), so the 64 row terms of a lane share 8 inlined copies of exp / log.  At the end
//                               the four lane groups meet through __shfl as (q0 + q2) + (q1 + q3); the logistic prior's dot4(x, x) comes from a pass of
//                               lane group g over the rows i = g (mod 4) of its columns.  One 8-byte store per column.
// Nothing waits on the device; the grids are functions of the shape (draws_logk.hpp); no atomics: the result depends on no grid, timing or atomic order.

#include "draws_logk.hpp"
#include "det_math.hpp"

#include <algorithm>

namespace mi {
namespace dprod {

namespace {
__global__ __launch_bounds__(256) void pack_kernel(const double* __restrict__ M, uint64_t rows, uint64_t cols, uint64_t Kp, uint64_t ld, double* __restrict__ At)
{
    const uint64_t n = Kp * ld;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256) {
        const uint64_t j = e / ld, i = e % ld;
        At[e] = (i < rows && j < cols) ? M[i * cols + j] : 0.0;
    }
}
}  // namespace

int pack_transposed(const double* M, uint64_t rows, uint64_t cols, uint64_t Kp, uint64_t ld, uint64_t grid, double* At, hipStream_t st)
{
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)grid), dim3(256), 0, st, M, rows, cols, Kp, ld, At);
    return (int)hipGetLastError();
}

}  // namespace dprod

namespace dlogk {

using dprod::LDS_STRIDE;
using dprod::STAGE;
using dprod::align256;
using dprod::double4_t;
enum : int { TGT_DENSE = 0, TGT_LOGISTIC = 1 };

LogkPlan logk_plan(int kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t C, bool slab_host, bool target_host)
{
    LogkPlan p;
    p.kind = kind;
    p.d = d;
    p.n_rows = n_rows;
    p.C = C;
    p.K = n_keep * C;
    p.route = (kind == LOGK_DENSE || kind == LOGK_LOGISTIC) ? LOGK_ROUTE_PRODUCT : LOGK_ROUTE_ELEMENTWISE;
    size_t pack = 0;
    if (p.route == LOGK_ROUTE_PRODUCT) {
        const uint64_t rows = kind == LOGK_DENSE ? d : n_rows;
        p.Kp = TK * ((d + TK - 1) / TK);
        p.ldA = TM * ((rows + TM - 1) / TM);
        p.n_row_tiles = p.ldA / TM;
        p.grid = (p.K + TN - 1) / TN;
        p.pack_grid = std::min<uint64_t>((p.Kp * p.ldA + 255) / 256, 1u << 16);
        p.lds_bytes = LOGK_LDS_BYTES;
        pack = (size_t)(p.Kp * p.ldA) * sizeof(double);
    } else {
        p.grid = (p.K + 255) / 256;
    }
    switch (kind) {
    case LOGK_DIAG: p.mat_doubles = d; break;
    case LOGK_DENSE: p.mat_doubles = (size_t)d * d; break;
    case LOGK_LOGISTIC: p.mat_doubles = (size_t)n_rows * d; p.y_doubles = n_rows; break;
    case LOGK_NORMAL_MODEL: p.y_doubles = n_rows; break;
    default: break;
    }
    p.o_pack = 0;
    p.o_mat = p.o_pack + align256(pack);
    p.o_y = p.o_mat + (target_host ? align256(p.mat_doubles * sizeof(double)) : 0);
    p.o_slab = p.o_y + (target_host ? align256(p.y_doubles * sizeof(double)) : 0);
    p.o_out = p.o_slab + (slab_host ? align256((size_t)p.K * d * sizeof(double)) : 0);
    p.bytes = p.o_out + (slab_host ? align256((size_t)p.K * sizeof(double)) : 0);
    if (p.bytes == 0) p.bytes = 256;
    return p;
}

namespace {

using dprod::combine4;     // (q0 + q2) + (q1 + q3) of the four lane groups (draws_product.hpp)

template <int KIND>
__global__ __launch_bounds__(256) void logk_elem_kernel(const double* __restrict__ x, uint64_t d, uint64_t C, uint64_t K, const double* __restrict__ prec,
                                                        const double* __restrict__ y, uint64_t n_rows, double* __restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const double* col = x + (k / C) * d * C + (k % C);
    if constexpr (KIND == LOGK_NORMAL_MODEL) {
        const double mu = col[0], sigma = col[C];
        const double n = (double)n_rows;
        double m2 = 0.0;
        for (uint64_t r = 0; r < n_rows; ++r) {
            const double e = y[r] - mu;
            m2 = dfma(e, e, m2);
        }
        const double s2 = sigma * sigma;
        out[k] = -(n * (0.5 * dprod::LOG_2PI + det_log(sigma))) - m2 / (2.0 * s2);
    } else {
        auto w_of = [&](uint64_t i, double xv) -> double { return KIND == LOGK_DIAG ? prec[i] * xv : xv; };
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
        uint64_t i = 0;
        for (; i + 4 <= d; i += 4) {
            const double x0 = col[i * C], x1 = col[(i + 1) * C], x2 = col[(i + 2) * C], x3 = col[(i + 3) * C];
            q0 = dfma(x0, w_of(i, x0), q0);
            q1 = dfma(x1, w_of(i + 1, x1), q1);
            q2 = dfma(x2, w_of(i + 2, x2), q2);
            q3 = dfma(x3, w_of(i + 3, x3), q3);
        }
        if (i < d) { const double xv = col[i * C]; q0 = dfma(xv, w_of(i, xv), q0); }
        if (i + 1 < d) { const double xv = col[(i + 1) * C]; q1 = dfma(xv, w_of(i + 1, xv), q1); }
        if (i + 2 < d) { const double xv = col[(i + 2) * C]; q2 = dfma(xv, w_of(i + 2, xv), q2); }
        out[k] = -0.5 * ((q0 + q2) + (q1 + q3));
    }
}

struct ProdParams {
    const double* At;        // [Kp][ldA]
    const double* x;         // the slab
    const double* y;         // LOGISTIC: [n_rows]
    double* out;             // [K]
    uint64_t d, C, K;        // d: the contraction length
    uint64_t rows;           // output rows that exist: d (DENSE), n_rows (LOGISTIC)
    uint64_t ldA;
    uint32_t nkb, n_row_tiles;      // Kp / 16, ldA / 128
};

template <int TGT>
__global__ MI_NO_DS_MERGE __launch_bounds__(256, 2) void logk_product_kernel(const ProdParams prm)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane >> 4, c16 = lane & 15;
    const uint64_t d = prm.d, C = prm.C, K = prm.K;
    const uint64_t n0 = (uint64_t)blockIdx.x * TN;
    // the column this thread stages (rows 8 s_half .. 8 s_half + 7 of every step), and the two columns whose results it holds
    const int s_c = tid & 127, s_half = tid >> 7;
    const uint64_t s_k = n0 + (uint64_t)s_c;
    const bool s_ok = s_k < K;
    const double* s_col = prm.x + (s_ok ? (s_k / C) * d * C + (s_k % C) : 0);
    uint64_t e_k[2];
    bool e_ok[2];
    const double* e_col[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        e_k[ni] = n0 + (uint64_t)(32 * wave + 16 * ni + c16);
        e_ok[ni] = e_k[ni] < K;
        e_col[ni] = prm.x + (e_ok[ni] ? (e_k[ni] / C) * d * C + (e_k[ni] % C) : 0);
    }
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double*)lds;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    const uint32_t d32 = (uint32_t)d;
    // the staging of draws_product.hpp: four waves share At's 16 rows, a thread moves 8 rows of its column
    auto issue_a = [&](uint32_t kb, uint32_t mt, int stage) __attribute__((always_inline)) {
        dprod::issue_a<4>(prm.At, prm.ldA, kb * TK, (uint64_t)mt * TM, lds_base, stage, wave, lane16);
    };
    auto load_b = [&](uint32_t kb, double (&v)[8]) __attribute__((always_inline)) { dprod::load_b<8>(s_col, kb, s_half, d32, C, v); };
    auto store_b = [&](uint32_t kb, int stage, const double (&v)[8]) __attribute__((always_inline)) {
        dprod::store_b<8>(lds + stage * STAGE, kb, s_half, s_c, d32, v);
    };

    double4_t acc[8][2];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
    double q[2] = {0.0, 0.0};
    double bv[8];
    const uint32_t nkb = prm.nkb;
    const uint64_t total = (uint64_t)nkb * prm.n_row_tiles;
    load_b(0, bv);
    issue_a(0, 0, 0);
    store_b(0, 0, bv);
    uint32_t kb = 0, mt = 0;
#pragma unroll 1
    for (uint64_t s = 0; s < total; ++s) {
        const int stage = (int)(s & 1u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's rows of At for step s landed ...
        __syncthreads();                                      // ... everybody's rows and columns, and nobody still reads the other stage
        uint32_t kb1 = kb + 1, mt1 = mt;
        if (kb1 == nkb) { kb1 = 0; mt1 = mt + 1; }
        const bool more = s + 1 < total;
        if (more) { load_b(kb1, bv); issue_a(kb1, mt1, stage ^ 1); }      // the columns first: what the compiler waits for before it reuses bv is already there
        dprod::mfma_step<8>(lds + stage * STAGE + j * (int)LDS_STRIDE + c16, lds + stage * STAGE + ((int)TK + j) * (int)LDS_STRIDE + 32 * wave + c16, acc);
        if (more) store_b(kb1, stage ^ 1, bv);
        if (kb == nkb - 1) {
            // the row tile is complete: acc[ti][ni][r] is element (row 128 mt + 16 ti + 4 r + j, column e_k[ni]).  Fold block 0, rotate, eight times:
            // the rows of a lane ascend (r inside a block, then the blocks), and the accumulators come out as zeros for the next row tile
            const uint64_t m0 = (uint64_t)mt * TM;
#pragma unroll 1
            for (int it = 0; it < 8; ++it) {
                const uint64_t rb = m0 + (uint64_t)(16 * it);
                if (rb < prm.rows) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint64_t row = rb + (uint64_t)(4 * r + j);
                        const bool rok = row < prm.rows;
                        if constexpr (TGT == TGT_DENSE) {
#pragma unroll
                            for (int ni = 0; ni < 2; ++ni) {
                                const double xv = (rok && e_ok[ni]) ? e_col[ni][row * C] : 0.0;
                                const double f = dfma(xv, acc[0][ni][r], q[ni]);
                                q[ni] = rok ? f : q[ni];
                            }
                        } else {
                            const double yv = rok ? prm.y[row] : 0.0;
#pragma unroll
                            for (int ni = 0; ni < 2; ++ni) {
                                const double f = q[ni] + dprod::logit_term(yv, acc[0][ni][r]);
                                q[ni] = rok ? f : q[ni];
                            }
                        }
                    }
                }
#pragma unroll
                for (int a = 0; a < 7; ++a)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) acc[a][ni] = acc[a + 1][ni];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) acc[7][ni] = double4_t{0.0, 0.0, 0.0, 0.0};
            }
        }
        kb = kb1;
        mt = mt1;
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const double dot = combine4(q[ni], c16);
        double res;
        if constexpr (TGT == TGT_DENSE) res = -0.5 * dot;
        else {
            double p = 0.0;                                  // the prior: chain j of dot4(x, x) runs over the rows i = j (mod 4)
            for (uint64_t i = (uint64_t)j; i < d; i += 4) {
                const double xv = e_ok[ni] ? e_col[ni][i * C] : 0.0;
                p = dfma(xv, xv, p);
            }
            const double xx = combine4(p, c16);
            res = dot - 0.5 * xx;
        }
        if (j == 0 && e_ok[ni]) prm.out[e_k[ni]] = res;
    }
}

template <int TGT>
int launch_product(const LogkPlan& p, const ProdParams& prm, hipStream_t st)
{
    auto kern = logk_product_kernel<TGT>;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)p.grid), dim3(p.block), p.lds_bytes, st, prm);
    return (int)hipGetLastError();
}

}  // namespace

int logk_run(const LogkPlan& p, const double* x, const double* mat, const double* y, void* ws, double* out, hipStream_t st)
{
    const dim3 g((unsigned)p.grid), b(p.block);
    if (p.route == LOGK_ROUTE_ELEMENTWISE) {
        if (p.kind == LOGK_ISO) hipLaunchKernelGGL(logk_elem_kernel<LOGK_ISO>, g, b, 0, st, x, p.d, p.C, p.K, mat, y, p.n_rows, out);
        else if (p.kind == LOGK_DIAG) hipLaunchKernelGGL(logk_elem_kernel<LOGK_DIAG>, g, b, 0, st, x, p.d, p.C, p.K, mat, y, p.n_rows, out);
        else hipLaunchKernelGGL(logk_elem_kernel<LOGK_NORMAL_MODEL>, g, b, 0, st, x, p.d, p.C, p.K, mat, y, p.n_rows, out);
        return (int)hipGetLastError();
    }
    const int e = logk_pack(p, mat, ws, st);
    if (e) return e;
    return logk_run_packed(p, x, mat, y, ws, out, st);
}

int logk_pack(const LogkPlan& p, const double* mat, void* ws, hipStream_t st)
{
    if (p.route != LOGK_ROUTE_PRODUCT) return 0;
    double* At = reinterpret_cast<double*>(static_cast<char*>(ws) + p.o_pack);
    return dprod::pack_transposed(mat, p.kind == LOGK_DENSE ? p.d : p.n_rows, p.d, p.Kp, p.ldA, p.pack_grid, At, st);
}

int logk_run_packed(const LogkPlan& p, const double* x, const double* mat, const double* y, void* ws, double* out, hipStream_t st)
{
    if (p.route == LOGK_ROUTE_ELEMENTWISE) return logk_run(p, x, mat, y, ws, out, st);
    double* At = reinterpret_cast<double*>(static_cast<char*>(ws) + p.o_pack);
    const uint64_t rows = p.kind == LOGK_DENSE ? p.d : p.n_rows;
    ProdParams prm;
    prm.At = At;
    prm.x = x;
    prm.y = y;
    prm.out = out;
    prm.d = p.d;
    prm.C = p.C;
    prm.K = p.K;
    prm.rows = rows;
    prm.ldA = p.ldA;
    prm.nkb = (uint32_t)(p.Kp / TK);
    prm.n_row_tiles = (uint32_t)p.n_row_tiles;
    return p.kind == LOGK_DENSE ? launch_product<TGT_DENSE>(p, prm, st) : launch_product<TGT_LOGISTIC>(p, prm, st);
}

}  // namespace dlogk
}  // namespace mi
