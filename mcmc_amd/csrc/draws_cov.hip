// draws_cov.hip -- the pooled covariance of a draws slab on the matrix cores (mi_mcmc_draws_covariance, include/mi_mcmc.h states the arithmetic).
//
// Sigma = E E^T / (K - 1) with E the d x K matrix of centred samples is a [d x K] [K x d] fp64 product whose two operands are row blocks of the SAME
// slab [n_keep][d][C], and whose contraction index k = t C + c is the CONTIGUOUS one.  Three kernels, every order a function of (n_keep, d, C) alone:
//
//   cov_mean_kernel    one workgroup per (dimension, sample group): 256 strided plain sums, k ascending, and pooled_variance_kernel's halving tree;
//   cov_mean_finish    the group sums of a dimension added in ascending group order, divided by K;
//   cov_syrk_kernel    one workgroup per (output tile with tj <= ti, K chunk): gemm_step_kernel's shape -- 128 x 128 per workgroup, 64 x 64 per wave, 16
//                      accumulators of v_mfma_f64_16x16x4_f64, K in steps of 16 through a double-buffered LDS stage -- but the stage TRANSPOSES: sixteen
//                      lanes read one 128-byte row segment (samples k .. k + 15 of a dimension), the centring e = x - mu is applied on the way, and the
//                      segment is laid out k-major, element (k, row) at k * 144 + (row ^ k).  The XOR spreads the sixteen k of a ds_write_b64 lane
//                      group over the sixteen 8-byte bank pairs (same row, stride 144 alone would put all of them on one), and keeps the fragment
//                      reads conflict-free: a 32-lane half of a ds_read_b64 holds k-rows 4 kk + {0, 1} (or {2, 3}), which sit 16 doubles apart modulo
//                      32 (144 = 4 * 32 + 16) and each cover a permutation of 16 consecutive doubles.  The next step's segments travel in registers
//                      while the matrix pipe works on this one.  An element of a chunk partial is ONE fma chain over the chunk's samples ascending (the
//                      k-steps of an MFMA and the K loop both ascend), from +0.  Padding -- samples past the chunk or past K, rows past d -- enters
//                      as exact +0 in BOTH operands (never 0 - mu).  A diagonal tile (its own instantiation and launch) stages its rows once, both operands
//                      read the same image, and only its 36 lower 16 x 16 blocks are computed: wave w takes row blocks w and 7 - w, 9 blocks each;
//   cov_finish_kernel  the chunk partials of an element added in ascending chunk order from +0, divided by K - 1, written to (i, j) and (j, i): one
//                      value, so the matrix is symmetric bit for bit (inside a diagonal tile the elements with j <= i are the ones kept).

#include "draws_cov.hpp"
#include "det_math.hpp"          // MI_NO_DS_MERGE

#include <algorithm>

namespace mi {
namespace dcov {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int CT = 128, CK = 16;
constexpr int CS = 144;                              // doubles per staged k-row: 128 + 16
constexpr int CSTAGE = 2 * CK * CS;                  // doubles per stage: 16 k-rows of the A rows, 16 of the B rows
constexpr size_t COV_LDS_BYTES = (size_t)(2 * CSTAGE + 2 * CT) * sizeof(double);      // two stages, then the means of the A rows and of the B rows
constexpr int TILE_ELEMS = CT * CT;

CovPlan cov_plan(uint64_t n_keep, uint64_t d, uint64_t C, bool want_cov)
{
    CovPlan p;
    p.K = n_keep * C;
    p.G = std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(1, 4096 / d), (p.K + 4095) / 4096));
    p.seg = 256 * (((p.K + p.G - 1) / p.G + 255) / 256);
    p.G = (p.K + p.seg - 1) / p.seg;
    p.T = (uint32_t)((d + CT - 1) / CT);
    p.n_pairs = p.T * (p.T + 1) / 2;
    const uint64_t n_target = std::max<uint64_t>(1, 1024 / p.n_pairs);
    p.KC = std::max<uint64_t>(512, 16 * (((p.K + n_target - 1) / n_target + 15) / 16));
    p.n_chunks = (p.K + p.KC - 1) / p.KC;
    p.o_gsum = 0;
    p.o_mean = p.o_gsum + (size_t)p.G * d;
    p.o_part = p.o_mean + (size_t)d;
    p.o_cov = p.o_part + (want_cov ? (size_t)p.n_chunks * p.n_pairs * TILE_ELEMS : 0);
    p.bytes = (p.o_cov + (want_cov ? (size_t)d * d : 0)) * sizeof(double);
    return p;
}

namespace {

// (t, c) of a sample index that moved forward by `step` inside the slab [t][.][c]
__device__ __forceinline__ void advance(uint64_t& t, uint64_t& c, uint64_t step, uint64_t C)
{
    c += step;
    if (c >= C) { const uint64_t q = c / C; t += q; c -= q * C; }
}

__global__ __launch_bounds__(256) void cov_mean_kernel(const double* __restrict__ x, uint64_t d, uint64_t C, uint64_t K, uint64_t seg, double* __restrict__ gsum)
{
    __shared__ double red[256];
    const uint64_t i = blockIdx.x, g = blockIdx.y;
    const uint64_t k_hi = (g + 1) * seg < K ? (g + 1) * seg : K;
    const uint64_t dC = d * C;
    const double* row = x + i * C;
    uint64_t k = g * seg + threadIdx.x;
    uint64_t t = k / C, c = k - t * C;
    double s = 0.0;
    while (k < k_hi) {
        if (k + 7 * 256 < k_hi && c + 7 * 256 < C) {              // eight samples of one slab row: the loads in flight together, the additions in order
            const double* p = row + t * dC + c;
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[u * 256];
#pragma unroll
            for (int u = 0; u < 8; ++u) s = s + v[u];
            k += 8 * 256; advance(t, c, 8 * 256, C);
        } else {
            s = s + row[t * dC + c];
            k += 256; advance(t, c, 256, C);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) { if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m]; __syncthreads(); }
    if (threadIdx.x == 0) gsum[g * d + i] = red[0];
}

__global__ __launch_bounds__(256) void cov_mean_finish_kernel(const double* __restrict__ gsum, uint64_t d, uint64_t G, uint64_t K, double* __restrict__ mean)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d) return;
    double s = 0.0;
    for (uint64_t g = 0; g < G; ++g) s = s + gsum[g * d + i];
    mean[i] = s / (double)K;
}

// pair index -> (ti, tj), tj <= ti, row by row of the lower triangle
__device__ __forceinline__ void pair_tiles(uint32_t p, uint32_t& ti, uint32_t& tj)
{
    uint32_t a = 0;
    while ((a + 1) * (a + 2) / 2 <= p) ++a;
    ti = a; tj = p - a * (a + 1) / 2;
}

// DIAG: the T diagonal tiles (one staged image serves both operands; wave w owns the 16-row blocks w and 7 - w with their column blocks up to the
// diagonal one: 9 of the tile's 36 lower blocks each, so the four SIMDs carry equal shares).  !DIAG: the T (T - 1) / 2 tiles below the diagonal.
template <bool DIAG>
__global__ MI_NO_DS_MERGE __launch_bounds__(256, 2) void cov_syrk_kernel(const double* __restrict__ x, const double* __restrict__ mean, uint64_t d, uint64_t C,
                                                                         uint64_t K, uint64_t KC, uint32_t T, double* __restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane >> 4, c16 = lane & 15;
    const uint32_t n_pairs = T * (T + 1) / 2;
    const uint32_t n_mine = DIAG ? T : n_pairs - T;      // tiles of this launch
    const uint32_t mine = blockIdx.x % n_mine;
    const uint64_t chunk = blockIdx.x / n_mine;
    uint32_t ti, tj;
    if (DIAG) { ti = tj = mine; }
    else { pair_tiles(mine, ti, tj); ++ti; }              // row by row of the STRICTLY lower triangle
    const uint32_t pair = ti * (ti + 1) / 2 + tj;
    const uint64_t m0 = (uint64_t)ti * CT, n0 = (uint64_t)tj * CT;
    const uint64_t k0 = chunk * KC;
    const uint64_t k_end = k0 + KC < K ? k0 + KC : K;
    const uint32_t nkb = (uint32_t)((k_end - k0 + CK - 1) / CK);
    const uint64_t dC = d * C;

    // staging: thread -> sample kk of the step, rows rs + 16 i of the A block and (!DIAG) of the B block
    const int kk = tid & 15, rs = tid >> 4;
    double* const mu = lds + 2 * CSTAGE;                 // [0, 128): the A rows, [128, 256): the B rows (registers are the accumulators')
    {
        const uint64_t r = tid < CT ? m0 + (uint64_t)tid : n0 + (uint64_t)(tid - CT);
        mu[tid] = r < d ? mean[r] : 0.0;
    }
    bool vA[8], vB[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { vA[i] = m0 + (uint64_t)(rs + 16 * i) < d; vB[i] = n0 + (uint64_t)(rs + 16 * i) < d; }
    const double* rowA = x + (m0 + (uint64_t)rs) * C;
    const double* rowB = x + (n0 + (uint64_t)rs) * C;
    const uint64_t rstep = 16 * C;
    uint64_t k = k0 + (uint64_t)kk;
    uint64_t t = k / C, c = k - t * C;
    double fa[8];
    [[maybe_unused]] double fb[8];
    bool fv = false;
    auto fetch = [&]() __attribute__((always_inline)) {
        fv = k < k_end;
        const uint64_t off = t * dC + c;
#pragma unroll
        for (int i = 0; i < 8; ++i) fa[i] = (fv && vA[i]) ? rowA[off + (uint64_t)i * rstep] : 0.0;
        if constexpr (!DIAG) {
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[i] = (fv && vB[i]) ? rowB[off + (uint64_t)i * rstep] : 0.0;
        }
        k += CK; advance(t, c, CK, C);
    };
    auto store = [&](int stage) __attribute__((always_inline)) {
        double* As = lds + stage * CSTAGE + kk * CS;
#pragma unroll
        for (int i = 0; i < 8; ++i) As[(rs + 16 * i) ^ kk] = (fv && vA[i]) ? fa[i] - mu[rs + 16 * i] : 0.0;
        if constexpr (!DIAG) {
            double* Bs = As + CK * CS;
#pragma unroll
            for (int i = 0; i < 8; ++i) Bs[(rs + 16 * i) ^ kk] = (fv && vB[i]) ? fb[i] - mu[CT + rs + 16 * i] : 0.0;
        }
    };

    constexpr int NA = DIAG ? 12 : 16;                   // DIAG: acc[0..3] row block w (columns 0..w), acc[4..11] row block 7 - w (columns 0..7 - w)
    double4_t acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = double4_t{0.0, 0.0, 0.0, 0.0};
    const int wm = wave >> 1, wn = wave & 1;             // !DIAG: the wave's 64 x 64 quarter of the tile
    const int r_lo = wave, r_hi = 7 - wave;              // DIAG: the wave's two 16-row blocks

    fetch();
    __syncthreads();                                     // the means are in LDS
    store(0);
    __syncthreads();
#pragma unroll 1
    for (uint32_t kb = 0; kb < nkb; ++kb) {
        const int stage = (int)(kb & 1u);
        const bool more = kb + 1 < nkb;
        if (more) fetch();
        if constexpr (DIAG) {
            const double* As = lds + stage * CSTAGE;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const int kr = 4 * k4 + j;
                const int o = kr * CS + (c16 ^ kr);
                const double a_lo = As[o + 16 * r_lo], a_hi = As[o + 16 * r_hi];
                double b[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) b[u] = As[o + 16 * u];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (u <= r_hi) acc[4 + u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_hi, b[u], acc[4 + u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u <= r_lo) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_lo, b[u], acc[u], 0, 0, 0);
            }
        } else {
            const double* As = lds + stage * CSTAGE + wm * 64;
            const double* Bs = lds + stage * CSTAGE + CK * CS + wn * 64;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const int kr = 4 * k4 + j;
                const int o = kr * CS + (c16 ^ kr);
                double a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { a[u] = As[o + 16 * u]; b[u] = Bs[o + 16 * u]; }
#pragma unroll
                for (int ai = 0; ai < 4; ++ai)
#pragma unroll
                    for (int bi = 0; bi < 4; ++bi) acc[4 * ai + bi] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ai], b[bi], acc[4 * ai + bi], 0, 0, 0);
            }
        }
        if (more) store(stage ^ 1);
        __syncthreads();                                  // step kb + 1 is staged, and nobody still reads the stage that step kb + 2 overwrites
    }
    // an accumulator's element r is the partial at row 4 r + j, column c16 of its 16 x 16 block
    double* out = part + ((size_t)chunk * n_pairs + pair) * TILE_ELEMS;
    if constexpr (DIAG) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (u <= r_hi) {
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(size_t)(16 * r_hi + 4 * r + j) * CT + (16 * u + c16)] = acc[4 + u][r];
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u <= r_lo) {
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(size_t)(16 * r_lo + 4 * r + j) * CT + (16 * u + c16)] = acc[u][r];
            }
    } else {
#pragma unroll
        for (int ai = 0; ai < 4; ++ai)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int bi = 0; bi < 4; ++bi) out[(size_t)(64 * wm + 16 * ai + 4 * r + j) * CT + (64 * wn + 16 * bi + c16)] = acc[4 * ai + bi][r];
    }
}

__global__ __launch_bounds__(256) void cov_finish_kernel(const double* __restrict__ part, uint64_t d, uint64_t K, uint32_t n_pairs, uint64_t n_chunks,
                                                         double* __restrict__ cov)
{
    const uint32_t pair = blockIdx.x / (TILE_ELEMS / 256);
    const uint32_t e = (blockIdx.x % (TILE_ELEMS / 256)) * 256 + threadIdx.x;
    const uint32_t li = e / CT, lj = e % CT;
    uint32_t ti, tj;
    pair_tiles(pair, ti, tj);
    const uint64_t i = (uint64_t)ti * CT + li, jj = (uint64_t)tj * CT + lj;
    if (i >= d || jj >= d || (ti == tj && lj > li)) return;
    double s = 0.0;
    for (uint64_t q = 0; q < n_chunks; ++q) s = s + part[((size_t)q * n_pairs + pair) * TILE_ELEMS + e];
    const double v = s / (double)(K - 1);
    cov[i * d + jj] = v;
    cov[jj * d + i] = v;
}

}  // namespace

int cov_run(const double* x, uint64_t d, uint64_t C, const CovPlan& p, void* ws, bool want_cov, hipStream_t st)
{
    double* W = static_cast<double*>(ws);
    hipLaunchKernelGGL(cov_mean_kernel, dim3((unsigned)d, (unsigned)p.G), dim3(256), 0, st, x, d, C, p.K, p.seg, W + p.o_gsum);
    hipLaunchKernelGGL(cov_mean_finish_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, W + p.o_gsum, d, p.G, p.K, W + p.o_mean);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !want_cov) return (int)e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cov_syrk_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COV_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cov_syrk_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COV_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    if (p.n_pairs > p.T)                                  // the tiles below the diagonal first: the long workgroups
        hipLaunchKernelGGL(cov_syrk_kernel<false>, dim3((unsigned)(p.n_chunks * (p.n_pairs - p.T))), dim3(256), COV_LDS_BYTES, st, x, W + p.o_mean, d, C, p.K, p.KC,
                           p.T, W + p.o_part);
    hipLaunchKernelGGL(cov_syrk_kernel<true>, dim3((unsigned)(p.n_chunks * p.T)), dim3(256), COV_LDS_BYTES, st, x, W + p.o_mean, d, C, p.K, p.KC, p.T, W + p.o_part);
    hipLaunchKernelGGL(cov_finish_kernel, dim3((unsigned)(p.n_pairs * (TILE_ELEMS / 256))), dim3(256), 0, st, W + p.o_part, d, p.K, p.n_pairs, p.n_chunks,
                       W + p.o_cov);
    return (int)hipGetLastError();
}

}  // namespace dcov
}  // namespace mi
