// draws_predict.hip -- posterior predictive checks of a draws slab under the logistic target (mi_mcmc_draws_predict; include/mi_mcmc.h states the
// arithmetic and its order, draws_predict.hpp the plan).  The samples are the K = n_keep * C columns k = t * C + c of a slab [n_keep][d][C].  Element
// (r, k) of the product X . Theta is eta, ONE fma chain over j ascending; from it
//     p = sigmoid(eta);   u = u01 of the Philox block of (seed, k, 0, r, STREAM_PREDICT);   yrep = u < p ? 1 : 0
// and the two kernels below fold (p, yrep) the two ways -- each forms the element for itself, from the same (seed, r, k, bits of eta), so they agree.
//
//   dprod::pack_kernel          once per call: X TRANSPOSED and zero-padded into At [Kp][ldR] (draws_product.hpp's launcher), for both kernels.
//   predict_shift_kernel        the shift of every (chunk, row), p[r][first column of the chunk], one thread each, the plain fma chain.
//   predict_rows_kernel         draws_waic.hip's waic_product_kernel -- eight waves, one 128-row tile and one chunk of 2048 columns per workgroup, the
//                               column tiles of 128 ascending, 8 accumulators and 16 rows x (A, S1, S2) running sums per lane -- with the epilogue
//                                   v = p - shift;  S1 += v;  S2 += v * v;  A += yrep
//                               and 8-byte stores of p and yrep where the matrices are asked for.  A, a count, runs as an integer per lane (16 VGPRs
//                               instead of 32: what keeps the kernel free of scratch) and is a double from the tree on.  The 64 slots meet in waic's tree.
//   predict_merge_kernel        one thread per row: the chunk partials -> (n, mean, M2, A), merged ascending by Chan's rule; p_mean, p_var, rep_freq.
//   predict_cols_kernel         draws_logk.hip's logk_product_kernel<TGT_LOGISTIC> -- four waves, 128 columns per workgroup, all row tiles ascending,
//                               16 accumulators rotated down per row block -- with THREE q per column instead of one:
//                                   qt += yrep;   qr += yrep * eta - softplus(eta);   qo += y_r * eta - softplus(eta)
//                               exp(-|eta|) and 1 + exp(-|eta|) are formed once for sigmoid and softplus (they are the same bits in both).  combine4 at the end.
//   predict_count_kernel        the summary's counts, grid-stride over the columns, one piece of three integers per workgroup; the host adds the pieces.
// Nothing waits on the device; no atomics; the grids are functions of the shape (and, for the grid-stride ones, of the test hook's cap, which changes no result).

#include "draws_predict.hpp"
#include "det_math.hpp"

#include <algorithm>

namespace mi {
namespace dpred {

using dprod::LDS_STRIDE;
using dprod::STAGE;
using dprod::align256;
using dprod::double4_t;
constexpr int SHIFT = 2 * STAGE;                                   // the shift [128] of the row tile behind the two stages

PredictPlan predict_plan(uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t C, bool slab_host, bool target_host, bool has_y, const PredictWants& w, uint64_t grid_cap)
{
    PredictPlan p;
    p.d = d;
    p.n_rows = n_rows;
    p.C = C;
    p.K = n_keep * C;
    p.rows = w.rows();
    p.cols = w.cols();
    p.counts = w.summary;
    p.n_chunks = (p.K + PRED_CHUNK - 1) / PRED_CHUNK;
    p.ldR = TM * ((n_rows + TM - 1) / TM);
    p.Kp = TK * ((d + TK - 1) / TK);
    p.n_row_tiles = p.ldR / TM;
    p.merge_grid = (n_rows + 255) / 256;
    p.rows_grid = p.n_chunks * p.n_row_tiles;
    p.cols_grid = (p.K + TN - 1) / TN;
    auto capped = [&](uint64_t g) { return (grid_cap != 0 && grid_cap < g) ? grid_cap : g; };
    p.pack_grid = capped(std::min<uint64_t>((p.Kp * p.ldR + 255) / 256, 1u << 16));
    p.count_grid = capped(std::min<uint64_t>((p.K + 255) / 256, PRED_COUNT_MAX_GRID));
    p.mat_doubles = (size_t)n_rows * d;
    p.y_doubles = has_y ? n_rows : 0;
    p.o_pack = 0;
    p.o_part = p.o_pack + align256((size_t)(p.Kp * p.ldR) * sizeof(double));
    p.o_rowout = p.o_part + (p.rows ? align256((size_t)p.n_chunks * 4 * p.ldR * sizeof(double)) : 0);
    p.o_colout = p.o_rowout + (p.rows ? align256((size_t)3 * p.ldR * sizeof(double)) : 0);
    p.o_pieces = p.o_colout + (p.cols ? align256((size_t)3 * p.K * sizeof(double)) : 0);
    p.o_mat = p.o_pieces + (p.counts ? align256((size_t)3 * p.count_grid * sizeof(uint64_t)) : 0);
    p.o_y = p.o_mat + (target_host ? align256(p.mat_doubles * sizeof(double)) : 0);
    p.o_slab = p.o_y + (target_host ? align256(p.y_doubles * sizeof(double)) : 0);
    p.o_prob = p.o_slab + (slab_host ? align256((size_t)p.K * d * sizeof(double)) : 0);
    p.o_yrep = p.o_prob + ((slab_host && w.prob) ? align256((size_t)p.K * n_rows * sizeof(double)) : 0);
    p.bytes = p.o_yrep + ((slab_host && w.yrep) ? align256((size_t)p.K * n_rows * sizeof(double)) : 0);
    return p;
}

namespace {

// u[r][k] of the definition: the first two words of the block of (seed, chain = k, draw 0, slot = r, STREAM_PREDICT)
__device__ __forceinline__ double uniform_of(uint64_t seed, uint64_t k, uint32_t row)
{
    const u32x4 w = rng_block(seed, k, 0u, row, STREAM_PREDICT);
    return u01(w.x, w.y);
}

// sigmoid(eta) and softplus(eta) of det_math.hpp, the same bits, from ONE exp and ONE 1 + exp: the argument of sigmoid's exp is -eta for eta >= 0 and
// eta below, softplus' is -eta for eta > 0 and eta otherwise -- they differ at eta = +-0 alone, where exp gives exactly 1 for either sign
__device__ __forceinline__ void sigmoid_softplus(double eta, double& p, double& sp)
{
    const double ex = det_exp(eta > 0.0 ? -eta : eta);
    const double den = 1.0 + ex;
    p = (eta >= 0.0 ? 1.0 : ex) / den;
    const double l1p = det_log(den);
    sp = (eta > 0.0) ? (eta + l1p) : l1p;
}

// part[(ch * 4 + 0) * ldR + r] = p[r][2048 ch]: eta is the fma chain over j ascending from +0, the chain an MFMA accumulator runs
__global__ __launch_bounds__(256) void predict_shift_kernel(const double* __restrict__ At, const double* __restrict__ x, uint64_t d, uint64_t C, uint64_t rows, uint64_t ldR,
                                                            uint64_t row_blocks, double* __restrict__ part)
{
    const uint64_t r = (uint64_t)(blockIdx.x % row_blocks) * 256 + threadIdx.x;
    if (r >= rows) return;
    const uint64_t ch = blockIdx.x / row_blocks, k0 = ch * PRED_CHUNK;
    const double* col = x + (k0 / C) * d * C + (k0 % C);
    double eta = 0.0;
    for (uint64_t j = 0; j < d; ++j) eta = dfma(At[j * ldR + r], col[j * C], eta);
    part[(ch * 4) * ldR + r] = sigmoid(eta);
}

struct RowsParams {
    const double* At;        // [Kp][ldR]
    const double* x;         // the slab
    double* part;            // [n_chunks][4][ldR]; stat 0, the shift, is there already
    double* prob;            // [n_rows][K], or NULL
    double* yrep;            // [n_rows][K], or NULL
    uint64_t seed;
    uint64_t d, C, K;
    uint64_t rows, ldR;
    uint32_t nkb, n_row_tiles;      // Kp / 16, ldR / 128
};

__global__ MI_NO_DS_MERGE __launch_bounds__(512) void predict_rows_kernel(const RowsParams prm)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = wave >> 2, wc = wave & 3;
    const int j = lane >> 4, c16 = lane & 15;
    const uint64_t d = prm.d, C = prm.C, K = prm.K;
    const uint32_t mt = blockIdx.x % prm.n_row_tiles;
    const uint64_t ch = blockIdx.x / prm.n_row_tiles;
    const uint64_t c0 = ch * PRED_CHUNK;
    const uint64_t cend = (K - c0 < PRED_CHUNK) ? K : c0 + PRED_CHUNK;
    const uint32_t n_ct = (uint32_t)((cend - c0 + TN - 1) / TN);
    const uint64_t m0 = (uint64_t)mt * TM;
    // the column this thread stages (rows 4 s_q .. 4 s_q + 3 of every step) in column tile ct; a column beyond K: the slab's first column
    const int s_c = tid & 127, s_q = tid >> 7;
    auto col_of = [&](uint32_t ct) -> const double* {
        const uint64_t k = c0 + (uint64_t)ct * TN + (uint64_t)s_c;
        return prm.x + (k < K ? (k / C) * d * C + (k % C) : 0);
    };
    const double* s_col = col_of(0);
    if (tid < (int)TM) {
        const uint64_t row = m0 + (uint64_t)tid;
        lds[SHIFT + tid] = row < prm.rows ? prm.part[(ch * 4) * prm.ldR + row] : 0.0;
    }
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double*)lds;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    const uint32_t d32 = (uint32_t)d;
    // the staging of draws_product.hpp: eight waves share At's 16 rows, a thread moves 4 rows of its column
    auto issue_a = [&](uint32_t kb, int stage) __attribute__((always_inline)) {
        dprod::issue_a<8>(prm.At, prm.ldR, kb * TK, m0, lds_base, stage, wave, lane16);
    };
    auto load_b = [&](uint32_t kb, double (&v)[4]) __attribute__((always_inline)) { dprod::load_b<4>(s_col, kb, s_q, d32, C, v); };
    auto store_b = [&](uint32_t kb, int stage, const double (&v)[4]) __attribute__((always_inline)) {
        dprod::store_b<4>(lds + stage * STAGE, kb, s_q, s_c, d32, v);
    };

    double4_t acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
    // the running sums of this lane's 16 rows, [row block][reg].  A counts replicated successes -- at most 32 per slot and chunk -- so it runs as an
    // integer, half the registers, and becomes a double for the tree: sums of small integers are exact in either type and in any order
    double s1[4][4], s2[4][4];
    uint32_t sA[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) { s1[a][r] = s2[a][r] = 0.0; sA[a][r] = 0u; }
    double bv[4];
    const uint32_t nkb = prm.nkb;
    const uint64_t total = (uint64_t)nkb * n_ct;
    load_b(0, bv);
    issue_a(0, 0);
    store_b(0, 0, bv);
    uint32_t kb = 0, ct = 0;
#pragma unroll 1
    for (uint64_t s = 0; s < total; ++s) {
        const int stage = (int)(s & 1u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's rows of At for step s landed ...
        __syncthreads();                                      // ... everybody's rows and columns, and nobody still reads the other stage
        uint32_t kb1 = kb + 1, ct1 = ct;
        if (kb1 == nkb) { kb1 = 0; ct1 = ct + 1; }
        const bool more = s + 1 < total;
        if (more) {
            if (ct1 != ct) s_col = col_of(ct1);
            load_b(kb1, bv);
            issue_a(kb1, stage ^ 1);
        }
        dprod::mfma_step<4>(lds + stage * STAGE + j * (int)LDS_STRIDE + 64 * h + c16, lds + stage * STAGE + ((int)TK + j) * (int)LDS_STRIDE + 32 * wc + c16, acc);
        if (more) store_b(kb1, stage ^ 1, bv);
        if (kb == nkb - 1) {
            // the column tile is complete: acc[ti][ni][r] is element (row m0 + 64 h + 16 ti + 4 r + j, column e_k[ni]).  Fold block 0, rotate, four times
            // (the lane's place is taken anew behind a barrier the compiler cannot look through: what the fold derives from it is formed here, once per
            // column tile, instead of living in registers across the matrix loop next to the accumulators and the sums)
            int le = lane;
            asm volatile("" : "+v"(le));
            const int je = le >> 4, ce = le & 15;
            uint64_t e_k[2];
            bool e_ok[2];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                e_k[ni] = c0 + (uint64_t)ct * TN + (uint64_t)(32 * wc + 16 * ni + ce);
                e_ok[ni] = e_k[ni] < K;
            }
#pragma unroll 1
            for (int it = 0; it < 4; ++it) {
                const int rl0 = 64 * h + 16 * it;
                if (m0 + (uint64_t)rl0 < prm.rows) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rl = rl0 + 4 * r + je;
                        const uint64_t row = m0 + (uint64_t)rl;
                        const bool rok = row < prm.rows;
                        const double sh = lds[SHIFT + rl];
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) {
                            const double p = sigmoid(acc[0][ni][r]);
                            const double u = uniform_of(prm.seed, e_k[ni], (uint32_t)row);
                            const double yr = (u < p) ? 1.0 : 0.0;
                            const double v = p - sh;
                            const double vv = v * v;
                            const bool ok = rok && e_ok[ni];
                            const double n1 = s1[0][r] + v, n2 = s2[0][r] + vv;
                            const uint32_t nA = sA[0][r] + (u < p ? 1u : 0u);
                            s1[0][r] = ok ? n1 : s1[0][r];
                            s2[0][r] = ok ? n2 : s2[0][r];
                            sA[0][r] = ok ? nA : sA[0][r];
                            if (ok && prm.prob) prm.prob[row * K + e_k[ni]] = p;
                            if (ok && prm.yrep) prm.yrep[row * K + e_k[ni]] = yr;
                        }
                    }
                }
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) acc[a][ni] = acc[a + 1][ni];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) acc[3][ni] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t tA = sA[0][r];
                    const double t1 = s1[0][r], t2 = s2[0][r];
#pragma unroll
                    for (int a = 0; a < 3; ++a) { sA[a][r] = sA[a + 1][r]; s1[a][r] = s1[a + 1][r]; s2[a][r] = s2[a + 1][r]; }
                    sA[3][r] = tA; s1[3][r] = t1; s2[3][r] = t2;
                }
            }
        }
        kb = kb1;
        ct = ct1;
    }
    // the 64 slots of every row meet: the 16 column lanes in a tree, then the four column waves through LDS (the stages are free: nobody reads them again)
    __syncthreads();
    double* red = lds;                                  // [wc][stat][128 rows]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double tA = dprod::tree16((double)sA[a][r]), t1 = dprod::tree16(s1[a][r]), t2 = dprod::tree16(s2[a][r]);
            const int rl = 64 * h + 16 * a + 4 * r + j;
            if (c16 == 0) {
                red[(wc * 3 + 0) * (int)TM + rl] = tA;
                red[(wc * 3 + 1) * (int)TM + rl] = t1;
                red[(wc * 3 + 2) * (int)TM + rl] = t2;
            }
        }
    __syncthreads();
    if (tid < (int)TM) {
        const uint64_t row = m0 + (uint64_t)tid;
        if (row < prm.rows) {
#pragma unroll
            for (int st = 0; st < 3; ++st) {
                const double w0 = red[(0 * 3 + st) * (int)TM + tid], w1 = red[(1 * 3 + st) * (int)TM + tid];
                const double w2 = red[(2 * 3 + st) * (int)TM + tid], w3 = red[(3 * 3 + st) * (int)TM + tid];
                prm.part[(ch * 4 + 1 + (uint64_t)st) * prm.ldR + row] = (w0 + w1) + (w2 + w3);
            }
        }
    }
}

// one thread per row: (shift, A, S1, S2) of every chunk -> (n, mean, M2), the chunks merged ascending; out [3][ldR] = p_mean, p_var = M2 / (K - 1), rep_freq = A / K
__global__ __launch_bounds__(256) void predict_merge_kernel(const double* __restrict__ part, uint64_t n_chunks, uint64_t K, uint64_t rows, uint64_t ldR, double* __restrict__ out)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    double n = 0.0, mean = 0.0, M2 = 0.0, A = 0.0;
    for (uint64_t ch = 0; ch < n_chunks; ++ch) {
        const uint64_t c0 = ch * PRED_CHUNK;
        const double nb = (double)((K - c0 < PRED_CHUNK) ? K - c0 : (uint64_t)PRED_CHUNK);
        const double* P = part + (ch * 4) * ldR + r;
        const double sh = P[0], Ab = P[ldR], S1 = P[2 * ldR], S2 = P[3 * ldR];
        const double mb = sh + S1 / nb;
        const double M2b = S2 - (S1 * S1) / nb;
        if (ch == 0) {
            n = nb; mean = mb; M2 = M2b; A = Ab;
        } else {
            const double delta = mb - mean;
            const double nn = n + nb;
            mean = mean + delta * (nb / nn);
            M2 = (M2 + M2b) + (delta * delta) * ((n * nb) / nn);
            n = nn;
            A = A + Ab;
        }
    }
    out[r] = mean;
    out[ldR + r] = M2 / (double)(K - 1);
    out[2 * ldR + r] = A / (double)K;
}

struct ColsParams {
    const double* At;        // [Kp][ldR]
    const double* x;         // the slab
    const double* y;         // [n_rows], or NULL: no observations, ll_obs is not formed
    double* out;             // [3][K]: t_rep, ll_rep, ll_obs
    uint64_t seed;
    uint64_t d, C, K;
    uint64_t rows, ldR;
    uint32_t nkb, n_row_tiles;      // Kp / 16, ldR / 128
};

__global__ MI_NO_DS_MERGE __launch_bounds__(256, 2) void predict_cols_kernel(const ColsParams prm)
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
    const double* s_col = prm.x + (s_k < K ? (s_k / C) * d * C + (s_k % C) : 0);
    uint64_t e_k[2];
    bool e_ok[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        e_k[ni] = n0 + (uint64_t)(32 * wave + 16 * ni + c16);
        e_ok[ni] = e_k[ni] < K;
    }
    const bool has_y = prm.y != nullptr;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double*)lds;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    const uint32_t d32 = (uint32_t)d;
    // the staging of draws_product.hpp: four waves share At's 16 rows, a thread moves 8 rows of its column
    auto issue_a = [&](uint32_t kb, uint32_t mt, int stage) __attribute__((always_inline)) {
        dprod::issue_a<4>(prm.At, prm.ldR, kb * TK, (uint64_t)mt * TM, lds_base, stage, wave, lane16);
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
    double qt[2] = {0.0, 0.0}, qr[2] = {0.0, 0.0}, qo[2] = {0.0, 0.0};
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
        if (more) { load_b(kb1, bv); issue_a(kb1, mt1, stage ^ 1); }
        dprod::mfma_step<8>(lds + stage * STAGE + j * (int)LDS_STRIDE + c16, lds + stage * STAGE + ((int)TK + j) * (int)LDS_STRIDE + 32 * wave + c16, acc);
        if (more) store_b(kb1, stage ^ 1, bv);
        if (kb == nkb - 1) {
            // the row tile is complete: acc[ti][ni][r] is element (row 128 mt + 16 ti + 4 r + j, column e_k[ni]).  Fold block 0, rotate, eight times:
            // the rows of a lane ascend (r inside a block, then the blocks) -- chain j of sum4 -- and the accumulators come out as zeros
            const uint64_t m0 = (uint64_t)mt * TM;
#pragma unroll 1
            for (int it = 0; it < 8; ++it) {
                const uint64_t rb = m0 + (uint64_t)(16 * it);
                if (rb < prm.rows) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint64_t row = rb + (uint64_t)(4 * r + j);
                        const bool rok = row < prm.rows;
                        const double yv = (rok && has_y) ? prm.y[row] : 0.0;
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) {
                            const double eta = acc[0][ni][r];
                            double p, sp;
                            sigmoid_softplus(eta, p, sp);
                            const double u = uniform_of(prm.seed, e_k[ni], (uint32_t)row);
                            const double yr = (u < p) ? 1.0 : 0.0;
                            const double ft = qt[ni] + yr;
                            const double fr = qr[ni] + (yr * eta - sp);
                            const double fo = qo[ni] + (yv * eta - sp);
                            qt[ni] = rok ? ft : qt[ni];
                            qr[ni] = rok ? fr : qr[ni];
                            qo[ni] = rok ? fo : qo[ni];
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
        const double t = dprod::combine4(qt[ni], c16), lr = dprod::combine4(qr[ni], c16), lo = dprod::combine4(qo[ni], c16);
        if (j == 0 && e_ok[ni]) {
            prm.out[e_k[ni]] = t;
            prm.out[K + e_k[ni]] = lr;
            if (has_y) prm.out[2 * K + e_k[ni]] = lo;
        }
    }
}

// piece g = {#{k : t_rep_k >= t_obs}, #{k : ll_rep_k <= ll_obs_k}, sum_k t_rep_k} over the columns k = 256 g + tid, + 256 gridDim.x, ...: integers, so
// the order of their sums is free (t_rep_k is a count of rows, below 2^32; a comparison with a NaN is false)
__global__ __launch_bounds__(256) void predict_count_kernel(const double* __restrict__ col, uint64_t K, double t_obs, uint64_t* __restrict__ pieces)
{
    __shared__ uint64_t red[3][256];
    uint64_t nt = 0, nd = 0, st = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < K; k += (uint64_t)gridDim.x * 256) {
        const double t = col[k], lr = col[K + k], lo = col[2 * K + k];
        nt += (t >= t_obs) ? 1u : 0u;
        nd += (lr <= lo) ? 1u : 0u;
        st += (uint64_t)t;
    }
    red[0][threadIdx.x] = nt; red[1][threadIdx.x] = nd; red[2][threadIdx.x] = st;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int i = 0; i < 3; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) pieces[(uint64_t)blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

}  // namespace

int predict_run(const PredictPlan& p, const double* x, const double* mat, const double* y, uint64_t seed, void* ws, double* prob, double* yrep, hipStream_t st)
{
    char* W = static_cast<char*>(ws);
    double* At = reinterpret_cast<double*>(W + p.o_pack);
    hipError_t e;
    const int pe = dprod::pack_transposed(mat, p.n_rows, p.d, p.Kp, p.ldR, p.pack_grid, At, st);
    if (pe) return pe;
    if (p.rows) {
        double* part = reinterpret_cast<double*>(W + p.o_part);
        // (n_chunks * ceil(n_rows / 256) <= the row kernel's grid, which the entry point keeps below 2^31)
        hipLaunchKernelGGL(predict_shift_kernel, dim3((unsigned)(p.n_chunks * p.merge_grid)), dim3(256), 0, st, At, x, p.d, p.C, p.n_rows, p.ldR, p.merge_grid, part);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        RowsParams prm;
        prm.At = At;
        prm.x = x;
        prm.part = part;
        prm.prob = prob;
        prm.yrep = yrep;
        prm.seed = seed;
        prm.d = p.d;
        prm.C = p.C;
        prm.K = p.K;
        prm.rows = p.n_rows;
        prm.ldR = p.ldR;
        prm.nkb = (uint32_t)(p.Kp / TK);
        prm.n_row_tiles = (uint32_t)p.n_row_tiles;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(predict_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PRED_ROWS_LDS_BYTES);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(predict_rows_kernel, dim3((unsigned)p.rows_grid), dim3(512), PRED_ROWS_LDS_BYTES, st, prm);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        hipLaunchKernelGGL(predict_merge_kernel, dim3((unsigned)p.merge_grid), dim3(256), 0, st, part, p.n_chunks, p.K, p.n_rows, p.ldR, reinterpret_cast<double*>(W + p.o_rowout));
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    if (p.cols) {
        ColsParams prm;
        prm.At = At;
        prm.x = x;
        prm.y = y;
        prm.out = reinterpret_cast<double*>(W + p.o_colout);
        prm.seed = seed;
        prm.d = p.d;
        prm.C = p.C;
        prm.K = p.K;
        prm.rows = p.n_rows;
        prm.ldR = p.ldR;
        prm.nkb = (uint32_t)(p.Kp / TK);
        prm.n_row_tiles = (uint32_t)p.n_row_tiles;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(predict_cols_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PRED_COLS_LDS_BYTES);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(predict_cols_kernel, dim3((unsigned)p.cols_grid), dim3(256), PRED_COLS_LDS_BYTES, st, prm);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    return 0;
}

int predict_count(const PredictPlan& p, double t_obs, void* ws, hipStream_t st)
{
    char* W = static_cast<char*>(ws);
    hipLaunchKernelGGL(predict_count_kernel, dim3((unsigned)p.count_grid), dim3(256), 0, st, reinterpret_cast<const double*>(W + p.o_colout), p.K, t_obs,
                       reinterpret_cast<uint64_t*>(W + p.o_pieces));
    return (int)hipGetLastError();
}

}  // namespace dpred
}  // namespace mi
