// draws_loglik.hip -- WAIC and PSIS-LOO of a pointwise log-likelihood matrix that the CALLER wrote (mi_mcmc_loglik_waic, mi_mcmc_loglik_psis_loo;
// draws_loglik.hpp states the plan).  The arithmetic is not restated: the sums run in include/mi_mcmc.h's section THE ORDER of mi_mcmc_draws_waic, and
// what follows the sort is draws_psis.hip's.  The matrix is a slab [n_keep][n_rows][C] (MI_LOGLIK_SLAB) or [n_rows][K] = [1][n_rows][K] (MI_LOGLIK_ROWS):
// element (r, k) sits at ((k div C) n_rows + r) C + k mod C of a slab with row length C.
//
//   loglik_fold_kernel   one WAVE owns one (row, chunk); LANE s IS SLOT s of the chunk's 64.  Of every column tile of 128 the lane takes the offsets
//                        o = 32 (s div 16) + s mod 16 and o + 16, ascending -- the slot's columns in the header's order --:
//                            v = ll - shift;  S1 += v;  S2 += v * v;  A += exp(ll)
//                        32 dependent steps per lane for a full chunk.  The wave's two loads of a tile cover its 1 KB (four runs of 128 bytes each);
//                        8-byte loads, so a row that starts 8-byte aligned only (C odd) is nothing special.  The (t, c) of a lane's column is carried
//                        along, not divided out per element: a chunk that straddles t in the SLAB layout wraps c and steps t.  The 16 lanes of a
//                        group meet by __shfl_xor 8, 4, 2, 1 (draws_waic.hip's tree16), the four groups as (w0 + w1) + (w2 + w3) by __shfl_xor 16, 32;
//                        lane 0 stores (shift, A, S1, S2) into the partials [n_chunks][4][ldR] that dwaic::waic_merge reads.
//   PSIS                 the matrix is the slab draws_rank.hip sorts, in place: no block is copied.  Per sort group rank_sort_group, then
//                        dpsis::psis_run_group on the sorted image.
// No atomics, no LDS, nothing waits on the device; the grids are functions of the shape.

#include "draws_loglik.hpp"
#include "det_math.hpp"

#include <algorithm>

namespace mi {
namespace dloglik {

using dprod::align256;
using dwaic::WAIC_CHUNK;

LoglikPlan loglik_plan(int layout, uint64_t n_rows, uint64_t n_keep, uint64_t C, bool mat_host, bool psis_entry, uint32_t lds_tail, uint64_t rank_budget)
{
    LoglikPlan p;
    p.layout = layout;
    p.psis_entry = psis_entry;
    p.n_rows = n_rows; p.n_keep = n_keep; p.C = C;
    p.K = n_keep * C;
    p.slab_C = layout == LOGLIK_SLAB ? C : p.K;
    p.n_chunks = (p.K + WAIC_CHUNK - 1) / WAIC_CHUNK;
    p.ldR = dwaic::TM * ((n_rows + dwaic::TM - 1) / dwaic::TM);
    p.fold_grid = (n_rows * p.n_chunks + FOLD_WAVES - 1) / FOLD_WAVES;
    p.fold_block = 64 * FOLD_WAVES;
    p.merge_grid = (n_rows + 255) / 256;
    size_t rows8 = 0, body = 0, rank = 0;
    if (psis_entry) {
        // the part of a PsisPlan that psis_run_group reads; there is no target and there are no row groups beside the sorter's own
        dpsis::PsisPlan& q = p.psis;
        q.n_rows = n_rows; q.n_keep = n_keep; q.C = C;
        q.K = p.K;
        q.M = dpsis::psis_tail_length(q.K);
        q.m = dpsis::psis_fit_points(q.M);
        q.lds_tail = (lds_tail == 0 || lds_tail > dpsis::PSIS_LDS_TAIL) ? dpsis::PSIS_LDS_TAIL : lds_tail;
        q.tail_route = q.M <= q.lds_tail ? dpsis::PSIS_TAIL_LDS : dpsis::PSIS_TAIL_GLOBAL;
        q.lds_bytes = q.tail_route == dpsis::PSIS_TAIL_LDS ? (size_t)q.M * sizeof(double) : 0;
        q.n_pieces = (q.K - q.M + dpsis::PSIS_BODY_PIECE - 1) / dpsis::PSIS_BODY_PIECE;
        q.rank = layout == LOGLIK_SLAB ? drank::rank_plan(n_keep, n_rows, C, 0, false, rank_budget) : drank::rank_plan(1, n_rows, p.K, 0, false, rank_budget);
        q.G = q.rank.dims_per_group;
        q.n_groups = q.rank.n_groups;
        rows8 = align256((size_t)n_rows * sizeof(double));
        body = align256((size_t)q.rank.dims_per_group * q.n_pieces * sizeof(double));
        rank = align256(q.rank.bytes);
    }
    const size_t ld8 = align256((size_t)p.ldR * sizeof(double));
    p.o_lppd = 0;
    p.o_pw = p.o_lppd + ld8;
    p.o_part = p.o_pw + ld8;
    p.o_elpd = p.o_part + align256((size_t)p.n_chunks * 4 * p.ldR * sizeof(double));
    p.o_k = p.o_elpd + rows8;
    p.o_body = p.o_k + rows8;
    p.o_mat = p.o_body + body;
    p.o_rank = p.o_mat + (mat_host ? align256((size_t)n_rows * p.K * sizeof(double)) : 0);
    p.bytes = p.o_rank + rank;
    return p;
}

namespace {

__global__ __launch_bounds__(256) void loglik_fold_kernel(const double* __restrict__ mat, uint64_t n_rows, uint64_t C, uint64_t K, uint64_t n_chunks, uint64_t ldR,
                                                          double* __restrict__ part)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t pair = (uint64_t)blockIdx.x * FOLD_WAVES + wave;
    if (pair >= n_rows * n_chunks) return;               // the whole wave: nothing below meets another wave
    const uint64_t row = pair / n_chunks, ch = pair % n_chunks;
    const uint64_t c0 = ch * WAIC_CHUNK;
    const uint32_t nb = (K - c0 < WAIC_CHUNK) ? (uint32_t)(K - c0) : WAIC_CHUNK;
    // (t, c) of column k moved on by step < 128 columns: one wrap where a slab row holds at least 128, a division where it is shorter
    auto advance = [&](uint64_t& t, uint64_t& c, uint32_t step) __attribute__((always_inline)) {
        c += step;
        if (c >= C) {
            if (C >= 128) { c -= C; ++t; }
            else { t += c / C; c = c % C; }
        }
    };
    auto at = [&](uint64_t t, uint64_t c) -> double { return mat[(t * n_rows + row) * C + c]; };
    uint64_t t = c0 / C, c = c0 % C;
    const double sh = at(t, c);                          // the chunk's first column
    const uint32_t o0 = 32u * (lane >> 4) + (lane & 15u);
    advance(t, c, o0);
    double A = 0.0, S1 = 0.0, S2 = 0.0;
    for (uint32_t ob = 0; ob < nb; ob += dwaic::TN) {
        const uint32_t oa = ob + o0;
        uint64_t t2 = t, c2 = c;
        advance(t2, c2, 16u);
        const bool ha = oa < nb, hb = oa + 16u < nb;     // k < K: nothing is read beyond the matrix
        const double la = ha ? at(t, c) : 0.0;
        const double lb = hb ? at(t2, c2) : 0.0;
        if (ha) {
            const double v = la - sh;
            S1 = S1 + v;
            S2 = S2 + v * v;
            A = A + det_exp(la);
        }
        if (hb) {
            const double v = lb - sh;
            S1 = S1 + v;
            S2 = S2 + v * v;
            A = A + det_exp(lb);
        }
        t = t2; c = c2;
        advance(t, c, 112u);
    }
    // the header's tree: the 16 slots of a group halved four times, then (w0 + w1) + (w2 + w3); lane 0 holds it
    auto tree64 = [&](double v) __attribute__((always_inline)) -> double {
        v = v + __shfl_xor(v, 8);
        v = v + __shfl_xor(v, 4);
        v = v + __shfl_xor(v, 2);
        v = v + __shfl_xor(v, 1);
        v = v + __shfl_xor(v, 16);
        v = v + __shfl_xor(v, 32);
        return v;
    };
    const double tA = tree64(A), t1 = tree64(S1), t2s = tree64(S2);
    if (lane == 0) {
        double* P = part + (ch * 4) * ldR + row;
        P[0] = sh;
        P[ldR] = tA;
        P[2 * ldR] = t1;
        P[3 * ldR] = t2s;
    }
}

}  // namespace

int loglik_fold(const LoglikPlan& p, const double* mat, void* ws, hipStream_t st)
{
    char* W = static_cast<char*>(ws);
    double* part = reinterpret_cast<double*>(W + p.o_part);
    hipLaunchKernelGGL(loglik_fold_kernel, dim3((unsigned)p.fold_grid), dim3(p.fold_block), 0, st, mat, p.n_rows, p.slab_C, p.K, p.n_chunks, p.ldR, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return dwaic::waic_merge(part, p.n_chunks, p.K, p.n_rows, p.ldR, reinterpret_cast<double*>(W + p.o_lppd), reinterpret_cast<double*>(W + p.o_pw), st);
}

int loglik_psis(const LoglikPlan& p, const double* mat, void* ws, hipStream_t st)
{
    char* W = static_cast<char*>(ws);
    double* elpd = reinterpret_cast<double*>(W + p.o_elpd);
    double* pk = reinterpret_cast<double*>(W + p.o_k);
    double* body = reinterpret_cast<double*>(W + p.o_body);
    const drank::RankPlan& rp = p.psis.rank;
    for (uint64_t dim0 = 0; dim0 < p.n_rows; dim0 += rp.dims_per_group) {
        const uint64_t nd = std::min<uint64_t>(rp.dims_per_group, p.n_rows - dim0);
        const uint64_t* sorted = nullptr;
        int e = drank::rank_sort_group(mat, rp, dim0, nd, false, W + p.o_rank, st, &sorted);
        if (e) return e;
        if ((e = dpsis::psis_run_group(p.psis, sorted, nd, body, elpd + dim0, pk + dim0, st))) return e;
    }
    return 0;
}

}  // namespace dloglik
}  // namespace mi
