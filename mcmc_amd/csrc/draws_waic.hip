// draws_waic.hip -- the pointwise log-likelihood of every data row at every column of a draws slab, folded over the columns per row
// (mi_mcmc_draws_waic; include/mi_mcmc.h states the arithmetic and its order, draws_waic.hpp the plan).  The samples are the K = n_keep * C columns
// k = t * C + c of a slab [n_keep][d][C], as in draws_logk.hip; they are cut into chunks of 2048.
//
//   dprod::pack_kernel          LOGISTIC, once per call: X TRANSPOSED and zero-padded into At [Kp][ldR] (draws_product.hpp's launcher, in draws_logk.hip).
//   waic_shift_kernel           LOGISTIC: the shift of every (chunk, row), ll[r][first column of the chunk], one thread each, the plain fma chain.
//   waic_product_kernel         LOGISTIC.  draws_logk.hip's product with the loop nest turned around: a workgroup of EIGHT waves owns one 128-row tile
//                               of X and one chunk of columns, and walks the chunk's column tiles of 128 ascending.  Wave (h, wc) = (wave >> 2, wave & 3)
//                               holds rows 64 h .. 64 h + 63 of the tile and columns 32 wc .. 32 wc + 31 of the column tile: 8 accumulators (4 row blocks
//                               x 2 column tiles of v_mfma_f64_16x16x4_f64), HALF of what a wave of draws_logk.hip holds, so that the running sums of
//                               16 rows x (A, S1, S2) = 96 VGPRs fit next to them at two waves per SIMD.  The staging is draws_product.hpp's (a wave moves
//                               2 of At's 16 rows, a thread 4 of its column's).  After a column tile every lane folds the 16 rows x 2 columns it holds (C/D map:
//                               col = lane & 15, row = (lane >> 4) + 4 reg) into ITS OWN sums of those rows -- nothing crosses lanes inside the loop:
//                                   ll = dprod::logit_term(y_r, eta);  v = ll - shift;  S1 += v;  S2 += v * v;  A += exp(ll)
//                               and stores ll (8 bytes, 16 lanes contiguous along c) where the matrix is asked for.  The fold is a rolled loop over the
//                               4 row blocks that rotates the accumulators down (zeros come in) and the sums around (after 4 turns they are back).
//                               At the end of the chunk the 16 column lanes meet by __shfl_xor 8, 4, 2, 1 and the four column waves through LDS as
//                               (w0 + w1) + (w2 + w3): the fixed tree of the 64 slots.
//   waic_elem_kernel            NORMAL_MODEL: the same slots, sums and tree without a product; a workgroup of four waves owns 16 rows and one chunk.
//   waic_merge_kernel           one thread per row: the chunk partials (shift, A, S1, S2) -> (n, mean, M2), merged ascending by Chan's rule; lppd, p_waic.
// Nothing waits on the device; the grids are functions of the shape; no atomics.

#include "draws_waic.hpp"
#include "det_math.hpp"

#include <algorithm>

namespace mi {
namespace dwaic {

using dprod::LDS_STRIDE;
using dprod::STAGE;
using dprod::align256;
using dprod::double4_t;
using dprod::logit_term;
constexpr int YSH = 2 * STAGE;                                     // y [128], shift [128] behind the two stages

WaicPlan waic_plan(int kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t C, bool slab_host, bool target_host, bool want_loglik)
{
    WaicPlan p;
    p.kind = kind;
    p.d = d;
    p.n_rows = n_rows;
    p.C = C;
    p.K = n_keep * C;
    p.route = kind == WAIC_LOGISTIC ? WAIC_ROUTE_PRODUCT : WAIC_ROUTE_ELEMENTWISE;
    p.n_chunks = (p.K + WAIC_CHUNK - 1) / WAIC_CHUNK;
    p.ldR = TM * ((n_rows + TM - 1) / TM);
    p.merge_grid = (n_rows + 255) / 256;
    size_t pack = 0;
    if (p.route == WAIC_ROUTE_PRODUCT) {
        p.Kp = TK * ((d + TK - 1) / TK);
        p.n_row_tiles = p.ldR / TM;
        p.grid = p.n_chunks * p.n_row_tiles;
        p.block = 512;
        p.pack_grid = std::min<uint64_t>((p.Kp * p.ldR + 255) / 256, 1u << 16);
        p.lds_bytes = WAIC_LDS_BYTES;
        pack = (size_t)(p.Kp * p.ldR) * sizeof(double);
        p.mat_doubles = (size_t)n_rows * d;
    } else {
        p.grid = p.n_chunks * ((n_rows + WAIC_NORMAL_ROWS - 1) / WAIC_NORMAL_ROWS);
        p.block = 256;
    }
    p.y_doubles = n_rows;
    p.o_pack = 0;
    p.o_part = p.o_pack + align256(pack);
    p.o_lppd = p.o_part + align256((size_t)p.n_chunks * 4 * p.ldR * sizeof(double));
    p.o_pw = p.o_lppd + align256((size_t)p.ldR * sizeof(double));
    p.o_mat = p.o_pw + align256((size_t)p.ldR * sizeof(double));
    p.o_y = p.o_mat + (target_host ? align256(p.mat_doubles * sizeof(double)) : 0);
    p.o_slab = p.o_y + (target_host ? align256(p.y_doubles * sizeof(double)) : 0);
    p.o_ll = p.o_slab + (slab_host ? align256((size_t)p.K * d * sizeof(double)) : 0);
    p.bytes = p.o_ll + ((slab_host && want_loglik) ? align256((size_t)p.K * n_rows * sizeof(double)) : 0);
    return p;
}

namespace {

// part[(ch * 4 + 0) * ldR + r] = ll[r][2048 ch]: eta is the fma chain over j ascending from +0, the chain an MFMA accumulator runs
__global__ __launch_bounds__(256) void waic_shift_kernel(const double* __restrict__ At, const double* __restrict__ x, const double* __restrict__ y, uint64_t d, uint64_t C,
                                                         uint64_t rows, uint64_t ldR, uint64_t row_blocks, double* __restrict__ part)
{
    const uint64_t r = (uint64_t)(blockIdx.x % row_blocks) * 256 + threadIdx.x;
    if (r >= rows) return;
    const uint64_t ch = blockIdx.x / row_blocks, k0 = ch * WAIC_CHUNK;
    const double* col = x + (k0 / C) * d * C + (k0 % C);
    double eta = 0.0;
    for (uint64_t j = 0; j < d; ++j) eta = dfma(At[j * ldR + r], col[j * C], eta);
    part[(ch * 4) * ldR + r] = logit_term(y[r], eta);
}

struct ProdParams {
    const double* At;        // [Kp][ldR]
    const double* x;         // the slab
    const double* y;         // [n_rows]
    double* part;            // [n_chunks][4][ldR]; stat 0, the shift, is there already
    double* loglik;          // [n_rows][K], or NULL
    uint64_t d, C, K;
    uint64_t rows, ldR;
    uint32_t nkb, n_row_tiles;      // Kp / 16, ldR / 128
};

using dprod::tree16;       // the tree of the 16 column lanes (draws_product.hpp)

__global__ MI_NO_DS_MERGE __launch_bounds__(512) void waic_product_kernel(const ProdParams prm)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = wave >> 2, wc = wave & 3;
    const int j = lane >> 4, c16 = lane & 15;
    const uint64_t d = prm.d, C = prm.C, K = prm.K;
    const uint32_t mt = blockIdx.x % prm.n_row_tiles;
    const uint64_t ch = blockIdx.x / prm.n_row_tiles;
    const uint64_t c0 = ch * WAIC_CHUNK;
    const uint64_t cend = (K - c0 < WAIC_CHUNK) ? K : c0 + WAIC_CHUNK;
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
        const bool rok = row < prm.rows;
        lds[YSH + tid] = rok ? prm.y[row] : 0.0;
        lds[YSH + (int)TM + tid] = rok ? prm.part[(ch * 4) * prm.ldR + row] : 0.0;
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
    // the running sums of this lane's 16 rows, [row block][reg]
    double sA[4][4], s1[4][4], s2[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) sA[a][r] = s1[a][r] = s2[a][r] = 0.0;
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
            uint64_t e_k[2];
            bool e_ok[2];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                e_k[ni] = c0 + (uint64_t)ct * TN + (uint64_t)(32 * wc + 16 * ni + c16);
                e_ok[ni] = e_k[ni] < K;
            }
#pragma unroll 1
            for (int it = 0; it < 4; ++it) {
                const int rl0 = 64 * h + 16 * it;
                if (m0 + (uint64_t)rl0 < prm.rows) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rl = rl0 + 4 * r + j;
                        const uint64_t row = m0 + (uint64_t)rl;
                        const bool rok = row < prm.rows;
                        const double yv = lds[YSH + rl], sh = lds[YSH + (int)TM + rl];
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) {
                            const double ll = logit_term(yv, acc[0][ni][r]);
                            const double v = ll - sh;
                            const double vv = v * v;
                            const double ex = det_exp(ll);
                            const bool ok = rok && e_ok[ni];
                            const double n1 = s1[0][r] + v, n2 = s2[0][r] + vv, nA = sA[0][r] + ex;
                            s1[0][r] = ok ? n1 : s1[0][r];
                            s2[0][r] = ok ? n2 : s2[0][r];
                            sA[0][r] = ok ? nA : sA[0][r];
                            if (ok && prm.loglik) prm.loglik[row * K + e_k[ni]] = ll;
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
                    const double tA = sA[0][r], t1 = s1[0][r], t2 = s2[0][r];
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
            const double tA = tree16(sA[a][r]), t1 = tree16(s1[a][r]), t2 = tree16(s2[a][r]);
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

// NORMAL_MODEL: thread (wave wc, j = lane >> 4, c16 = lane & 15) holds the rows row0 + j + 4 i, i < 4, and slot 16 wc + c16 of the chunk
__global__ __launch_bounds__(256) void waic_elem_kernel(const double* __restrict__ x, const double* __restrict__ y, uint64_t C, uint64_t K, uint64_t rows, uint64_t ldR,
                                                        uint64_t n_row_groups, double* __restrict__ part, double* __restrict__ loglik)
{
    __shared__ double red[4 * 3 * WAIC_NORMAL_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wc = tid >> 6;
    const int j = lane >> 4, c16 = lane & 15;
    const uint64_t rg = blockIdx.x % n_row_groups, ch = blockIdx.x / n_row_groups;
    const uint64_t row0 = rg * WAIC_NORMAL_ROWS;
    const uint64_t c0 = ch * WAIC_CHUNK;
    const uint64_t cend = (K - c0 < WAIC_CHUNK) ? K : c0 + WAIC_CHUNK;
    auto ll_of = [&](double yv, double mu, double base, double den) -> double {
        const double e = yv - mu;
        return base - (e * e) / den;
    };
    double yv[4], sh[4], sA[4], s1[4], s2[4];
    {
        const double* col = x + (c0 / C) * 2 * C + (c0 % C);
        const double mu = col[0], sigma = col[C];
        const double base = -(0.5 * dprod::LOG_2PI + det_log(sigma)), den = 2.0 * (sigma * sigma);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t row = row0 + (uint64_t)(j + 4 * i);
            yv[i] = row < rows ? y[row] : 0.0;
            sh[i] = ll_of(yv[i], mu, base, den);
            sA[i] = s1[i] = s2[i] = 0.0;
        }
    }
    // the slot's columns ascending: offsets 32 wc + c16 and + 16 of every column tile of 128
    const uint32_t n_half = 2 * (uint32_t)((cend - c0 + TN - 1) / TN);
    for (uint32_t q = 0; q < n_half; ++q) {
        const uint64_t k = c0 + (uint64_t)(q >> 1) * TN + (uint64_t)(32 * wc + 16 * (int)(q & 1u) + c16);
        if (k >= cend) continue;
        const double* col = x + (k / C) * 2 * C + (k % C);
        const double mu = col[0], sigma = col[C];
        const double base = -(0.5 * dprod::LOG_2PI + det_log(sigma)), den = 2.0 * (sigma * sigma);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t row = row0 + (uint64_t)(j + 4 * i);
            const double ll = ll_of(yv[i], mu, base, den);
            const double v = ll - sh[i];
            s1[i] = s1[i] + v;
            s2[i] = s2[i] + v * v;
            sA[i] = sA[i] + det_exp(ll);
            if (loglik && row < rows) loglik[row * K + k] = ll;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double tA = tree16(sA[i]), t1 = tree16(s1[i]), t2 = tree16(s2[i]);
        const int rl = j + 4 * i;
        if (c16 == 0) {
            red[(wc * 3 + 0) * (int)WAIC_NORMAL_ROWS + rl] = tA;
            red[(wc * 3 + 1) * (int)WAIC_NORMAL_ROWS + rl] = t1;
            red[(wc * 3 + 2) * (int)WAIC_NORMAL_ROWS + rl] = t2;
        }
    }
    __syncthreads();
    if (tid < (int)WAIC_NORMAL_ROWS) {
        const uint64_t row = row0 + (uint64_t)tid;
        if (row < rows) {
            // the shift of (chunk, row), as every thread of the row formed it above, for the merge
            const double* col = x + (c0 / C) * 2 * C + (c0 % C);
            const double mu = col[0], sigma = col[C];
            const double base = -(0.5 * dprod::LOG_2PI + det_log(sigma)), den = 2.0 * (sigma * sigma);
            part[(ch * 4) * ldR + row] = ll_of(y[row], mu, base, den);
#pragma unroll
            for (int st = 0; st < 3; ++st) {
                const double w0 = red[(0 * 3 + st) * (int)WAIC_NORMAL_ROWS + tid], w1 = red[(1 * 3 + st) * (int)WAIC_NORMAL_ROWS + tid];
                const double w2 = red[(2 * 3 + st) * (int)WAIC_NORMAL_ROWS + tid], w3 = red[(3 * 3 + st) * (int)WAIC_NORMAL_ROWS + tid];
                part[(ch * 4 + 1 + (uint64_t)st) * ldR + row] = (w0 + w1) + (w2 + w3);
            }
        }
    }
}

// one thread per row: (shift, A, S1, S2) of every chunk -> (n, mean, M2), the chunks merged ascending; lppd = log(A / K), p_waic = M2 / (K - 1)
__global__ __launch_bounds__(256) void waic_merge_kernel(const double* __restrict__ part, uint64_t n_chunks, uint64_t K, uint64_t rows, uint64_t ldR,
                                                         double* __restrict__ lppd, double* __restrict__ p_waic)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    double n = 0.0, mean = 0.0, M2 = 0.0, A = 0.0;
    for (uint64_t ch = 0; ch < n_chunks; ++ch) {
        const uint64_t c0 = ch * WAIC_CHUNK;
        const double nb = (double)((K - c0 < WAIC_CHUNK) ? K - c0 : (uint64_t)WAIC_CHUNK);
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
    lppd[r] = det_log(A / (double)K);
    p_waic[r] = M2 / (double)(K - 1);
}

}  // namespace

int waic_run(const WaicPlan& p, const double* x, const double* mat, const double* y, void* ws, double* loglik, hipStream_t st)
{
    char* W = static_cast<char*>(ws);
    double* part = reinterpret_cast<double*>(W + p.o_part);
    double* lppd = reinterpret_cast<double*>(W + p.o_lppd);
    double* pw = reinterpret_cast<double*>(W + p.o_pw);
    hipError_t e;
    if (p.route == WAIC_ROUTE_PRODUCT) {
        double* At = reinterpret_cast<double*>(W + p.o_pack);
        const int pe = dprod::pack_transposed(mat, p.n_rows, p.d, p.Kp, p.ldR, p.pack_grid, At, st);
        if (pe) return pe;
        // (n_chunks * ceil(n_rows / 256) <= the product kernel's grid, which the entry point keeps below 2^31)
        hipLaunchKernelGGL(waic_shift_kernel, dim3((unsigned)(p.n_chunks * p.merge_grid)), dim3(256), 0, st, At, x, y, p.d, p.C, p.n_rows, p.ldR, p.merge_grid, part);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        ProdParams prm;
        prm.At = At;
        prm.x = x;
        prm.y = y;
        prm.part = part;
        prm.loglik = loglik;
        prm.d = p.d;
        prm.C = p.C;
        prm.K = p.K;
        prm.rows = p.n_rows;
        prm.ldR = p.ldR;
        prm.nkb = (uint32_t)(p.Kp / TK);
        prm.n_row_tiles = (uint32_t)p.n_row_tiles;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(waic_product_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(waic_product_kernel, dim3((unsigned)p.grid), dim3(p.block), p.lds_bytes, st, prm);
    } else {
        const uint64_t groups = (p.n_rows + WAIC_NORMAL_ROWS - 1) / WAIC_NORMAL_ROWS;
        hipLaunchKernelGGL(waic_elem_kernel, dim3((unsigned)p.grid), dim3(p.block), 0, st, x, y, p.C, p.K, p.n_rows, p.ldR, groups, part, loglik);
    }
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(waic_merge_kernel, dim3((unsigned)p.merge_grid), dim3(256), 0, st, part, p.n_chunks, p.K, p.n_rows, p.ldR, lppd, pw);
    return (int)hipGetLastError();
}

int waic_merge(const double* part, uint64_t n_chunks, uint64_t K, uint64_t n_rows, uint64_t ldR, double* lppd, double* p_waic, hipStream_t st)
{
    hipLaunchKernelGGL(waic_merge_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, part, n_chunks, K, n_rows, ldR, lppd, p_waic);
    return (int)hipGetLastError();
}

}  // namespace dwaic
}  // namespace mi
