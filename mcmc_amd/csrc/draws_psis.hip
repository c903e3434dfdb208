// draws_psis.hip -- PSIS-LOO per data row out of the SORTED key image of the row's K pointwise log-likelihoods (mi_mcmc_draws_psis_loo; include/mi_mcmc.h
// states the arithmetic and its order, draws_psis.hpp the plan).  The image is draws_rank.hip's: row j of a group at sorted + j K, ascending by
// dsel::sel_key, so the LARGEST importance ratios exp(-ll) come first: s_0 .. s_{M-1} are the tail, the other K - M values the body.
//
//   psis_body_kernel   a workgroup owns one piece of PSIS_BODY_PIECE body values of one row and folds exp(s_0 - s_i) over it: thread t takes the values
//                      t, t + 256, ... of the piece ascending from +0 (the 256 slots of SUM), the slots meet in LDS by halving; one partial per
//                      (row, piece), stored.  It streams the image once, 8 bytes per lane, lanes along the row.
//   psis_tail_kernel   a workgroup owns one row.  It forms the M exceedances x_j = exp(s_0 - s_{M-j}) - exp(cut) -- into LDS while M <= the capacity
//                      (TAIL_LDS), otherwise every use recomputes them from the image in device memory (the same expression, so the same bits) --,
//                      runs the Zhang-Stephens fit (m passes of SUM over the M logarithms, thread 0 finishing k_j and L_j; then thread j the plain
//                      sum over l of exp(L_l - L_j); thread 0 the two plain sums over j), the SUM of the fitted profile, the smoothed tail and its
//                      two folds, merges the row's body partials ascending and writes elpd_loo_r and pareto_k_r.
// Every branch on the row's values (not finite; degenerate) is uniform over the workgroup.  No atomics, nothing waits on the device.

#include "draws_psis.hpp"
#include "draws_select.hpp"
#include "det_math.hpp"

#include <algorithm>

namespace mi {
namespace dpsis {

using dprod::align256;
using dsel::sel_unkey;

namespace {
// floor(sqrt(v)), v < 2^62, by bits
uint64_t isqrt64(uint64_t v)
{
    uint64_t r = 0;
    for (int sh = 30; sh >= 0; --sh) {
        const uint64_t c = r | (1ull << sh);
        if (c * c <= v) r = c;
    }
    return r;
}
}  // namespace

uint64_t psis_tail_length(uint64_t K)
{
    if (K == 0) return 0;
    const uint64_t m3 = isqrt64(9 * K - 1) + 1;          // the smallest integer whose square is >= 9 K
    return std::min<uint64_t>(K / 5, m3);
}

uint32_t psis_fit_points(uint64_t M) { return 30u + (uint32_t)isqrt64(M); }

PsisPlan psis_plan(int kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t C, bool slab_host, bool target_host, uint64_t ll_bytes, uint32_t lds_tail,
                   uint64_t rank_budget)
{
    PsisPlan p;
    p.kind = kind;
    p.d = d; p.n_rows = n_rows; p.n_keep = n_keep; p.C = C;
    p.K = n_keep * C;
    p.M = psis_tail_length(p.K);
    p.m = psis_fit_points(p.M);
    p.lds_tail = (lds_tail == 0 || lds_tail > PSIS_LDS_TAIL) ? PSIS_LDS_TAIL : lds_tail;
    p.tail_route = p.M <= p.lds_tail ? PSIS_TAIL_LDS : PSIS_TAIL_GLOBAL;
    p.lds_bytes = p.tail_route == PSIS_TAIL_LDS ? (size_t)p.M * sizeof(double) : 0;
    if (ll_bytes == 0 || ll_bytes > PSIS_LL_BYTES) ll_bytes = PSIS_LL_BYTES;
    const uint64_t tile_bytes = (uint64_t)dwaic::TM * 8 * std::max<uint64_t>(1, p.K);
    p.G = std::min<uint64_t>(std::max<uint64_t>(1, n_rows), (uint64_t)dwaic::TM * std::max<uint64_t>(1, ll_bytes / tile_bytes));
    p.n_groups = (n_rows + p.G - 1) / p.G;
    p.n_pieces = (p.K - p.M + PSIS_BODY_PIECE - 1) / PSIS_BODY_PIECE;
    p.waic = dwaic::waic_plan(kind, d, p.G, n_keep, C, false, false, true);
    p.rank = drank::rank_plan(1, p.G, p.K, 0, false, rank_budget);
    p.mat_doubles = kind == dwaic::WAIC_LOGISTIC ? (size_t)n_rows * d : 0;
    p.y_doubles = n_rows;
    const size_t rows8 = align256((size_t)n_rows * sizeof(double));
    p.o_elpd = 0;
    p.o_k = p.o_elpd + rows8;
    p.o_lppd = p.o_k + rows8;
    p.o_part = p.o_lppd + rows8;
    p.o_mat = p.o_part + align256((size_t)p.G * p.n_pieces * sizeof(double));
    p.o_y = p.o_mat + (target_host ? align256(p.mat_doubles * sizeof(double)) : 0);
    p.o_slab = p.o_y + (target_host ? align256(p.y_doubles * sizeof(double)) : 0);
    p.o_waic = p.o_slab + (slab_host ? align256((size_t)p.K * d * sizeof(double)) : 0);
    p.o_ll = p.o_waic + align256(p.waic.bytes);
    p.o_rank = p.o_ll + align256((size_t)p.G * p.K * sizeof(double));
    p.bytes = p.o_rank + align256(p.rank.bytes);
    return p;
}

namespace {

// SUM's tree: the 256 slots halved seven times; every thread gets the result.  red is free again on return
__device__ __forceinline__ double block_sum(double* red, uint32_t tid, double acc)
{
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (uint32_t h = PSIS_SLOTS / 2; h >= 1; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void psis_body_kernel(const uint64_t* __restrict__ sorted, uint64_t K, uint64_t M, uint32_t n_pieces, double* __restrict__ part)
{
    __shared__ double red[PSIS_SLOTS];
    const uint32_t tid = threadIdx.x;
    const uint64_t row = blockIdx.x / n_pieces, piece = blockIdx.x % n_pieces;
    const uint64_t* __restrict__ s = sorted + row * K;
    const double s0 = sel_unkey(s[0]);
    const uint64_t n_body = K - M;
    const uint64_t e0 = piece * PSIS_BODY_PIECE;
    const uint64_t e1 = (n_body - e0 < PSIS_BODY_PIECE) ? n_body : e0 + PSIS_BODY_PIECE;
    double acc = 0.0;
    for (uint64_t e = e0 + tid; e < e1; e += PSIS_SLOTS) acc = acc + det_exp(s0 - sel_unkey(s[M + e]));
    const double r = block_sum(red, tid, acc);
    if (tid == 0) part[row * n_pieces + piece] = r;
}

template <bool TAIL_LDS>
__global__ __launch_bounds__(256) void psis_tail_kernel(const uint64_t* __restrict__ sorted, uint64_t K, uint32_t M, uint32_t m, uint32_t n_pieces,
                                                        const double* __restrict__ part, double* __restrict__ elpd, double* __restrict__ pk)
{
    extern __shared__ __attribute__((aligned(16))) double xs[];         // TAIL_LDS: the exceedances x_1 .. x_M
    __shared__ double red[PSIS_SLOTS];
    __shared__ double bj[PSIS_MAX_FIT], Lj[PSIS_MAX_FIT], wj[PSIS_MAX_FIT];
    __shared__ double bh_s;
    const uint32_t tid = threadIdx.x;
    const uint64_t row = blockIdx.x;
    const uint64_t* __restrict__ s = sorted + row * K;
    const double s0 = sel_unkey(s[0]), s_last = sel_unkey(s[K - 1]);
    if (!is_finite(s0) || !is_finite(s_last)) {          // -inf sorts first, +inf and NaN last
        if (tid == 0) { elpd[row] = __builtin_nan(""); pk[row] = __builtin_nan(""); }
        return;
    }
    const double dcut = s0 - sel_unkey(s[M]);
    const double cut = dcut > PSIS_LOG_MIN_NORMAL ? dcut : PSIS_LOG_MIN_NORMAL;
    const double ec = det_exp(cut);
    // x_j, j = j0 + 1: of sorted element M - j
    auto x_global = [&](uint32_t j0) -> double { return det_exp(s0 - sel_unkey(s[M - 1 - j0])) - ec; };
    if (TAIL_LDS) {
        for (uint32_t j0 = tid; j0 < M; j0 += PSIS_SLOTS) xs[j0] = x_global(j0);
        __syncthreads();
    }
    auto x_at = [&](uint32_t j0) -> double { return TAIL_LDS ? xs[j0] : x_global(j0); };
    const double n = (double)M;
    const double q = x_at((M + 2) / 4 - 1), xM = x_at(M - 1);
    bool deg = !(q > 0.0);
    double kh = 0.0, sigma = 0.0;
    if (!deg) {
        const double q3 = 3.0 * q, ixM = 1.0 / xM;
        for (uint32_t j = 1; j <= m; ++j) {
            const double b = (1.0 - __builtin_sqrt((double)m / ((double)j - 0.5))) / q3 + ixM;
            double acc = 0.0;
            for (uint32_t i0 = tid; i0 < M; i0 += PSIS_SLOTS) acc = acc + det_log(1.0 - b * x_at(i0));
            const double sum = block_sum(red, tid, acc);
            if (tid == 0) {
                const double kj = sum / n;
                const double t = b / kj;
                bj[j - 1] = b;
                Lj[j - 1] = n * ((det_log(-t) - kj) - 1.0);
            }
        }
        __syncthreads();
        for (uint32_t j0 = tid; j0 < m; j0 += PSIS_SLOTS) {
            const double Lme = Lj[j0];
            double acc = 0.0;
            for (uint32_t l = 0; l < m; ++l) acc = acc + det_exp(Lj[l] - Lme);
            const double w = 1.0 / acc;
            wj[j0] = w >= PSIS_W_MIN ? w : 0.0;
        }
        __syncthreads();
        if (tid == 0) {
            double sw = 0.0, bh = 0.0;
            for (uint32_t j0 = 0; j0 < m; ++j0) sw = sw + wj[j0];
            for (uint32_t j0 = 0; j0 < m; ++j0) {
                const double wn = wj[j0] / sw;
                bh = bh + bj[j0] * wn;
            }
            bh_s = bh;
        }
        __syncthreads();
        const double bh = bh_s;
        double acc = 0.0;
        for (uint32_t i0 = tid; i0 < M; i0 += PSIS_SLOTS) acc = acc + det_log(1.0 - bh * x_at(i0));
        const double k0 = block_sum(red, tid, acc) / n;
        sigma = -(k0 / bh);
        kh = (n * k0 + 5.0) / (n + 10.0);
        deg = !is_finite(kh) || !(sigma > 0.0);
    }
    // the tail's log-weights -- smoothed, or raw where the tail is degenerate -- and the two folds
    const double nkh = -kh;
    double aW = 0.0, aN = 0.0;
    for (uint32_t j0 = tid; j0 < M; j0 += PSIS_SLOTS) {
        const double sj = sel_unkey(s[M - 1 - j0]);
        double t;
        if (deg) {
            t = s0 - sj;
        } else {
            const double p = ((double)(j0 + 1) - 0.5) / n;
            const double lg = det_log(1.0 - p);
            double g;
            if (kh == 0.0) g = -(sigma * lg);
            else g = (sigma * (det_exp(nkh * lg) - 1.0)) / kh;
            const double lt = det_log(g + ec);
            t = lt < 0.0 ? lt : 0.0;
        }
        aW = aW + det_exp(t);
        aN = aN + det_exp(t + (sj - s0));
    }
    const double Wt = block_sum(red, tid, aW);
    const double Nt = block_sum(red, tid, aN);
    if (tid == 0) {
        double B = 0.0;
        for (uint32_t p = 0; p < n_pieces; ++p) B = B + part[row * n_pieces + p];
        const double W = B + Wt;
        const double N = (double)(K - M) + Nt;
        elpd[row] = (s0 + det_log(N)) - det_log(W);
        pk[row] = deg ? INF : kh;
    }
}

}  // namespace

int psis_run_group(const PsisPlan& p, const uint64_t* sorted, uint64_t nd, double* part, double* elpd, double* pk, hipStream_t st)
{
    hipError_t e;
    hipLaunchKernelGGL(psis_body_kernel, dim3((unsigned)(nd * p.n_pieces)), dim3(PSIS_SLOTS), 0, st, sorted, p.K, p.M, (uint32_t)p.n_pieces, part);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if (p.tail_route == PSIS_TAIL_LDS) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(psis_tail_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(psis_tail_kernel<true>, dim3((unsigned)nd), dim3(PSIS_SLOTS), p.lds_bytes, st, sorted, p.K, (uint32_t)p.M, p.m, (uint32_t)p.n_pieces, part, elpd, pk);
    } else {
        hipLaunchKernelGGL(psis_tail_kernel<false>, dim3((unsigned)nd), dim3(PSIS_SLOTS), 0, st, sorted, p.K, (uint32_t)p.M, p.m, (uint32_t)p.n_pieces, part, elpd, pk);
    }
    return (int)hipGetLastError();
}

}  // namespace dpsis
}  // namespace mi
