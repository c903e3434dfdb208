// draws_nested.hip -- the nested R-hat of a draws slab (mi_mcmc_draw_stats_nested, include/mi_mcmc.h states the arithmetic).
//
// The C chains of a slab [n_keep][d][C] are K = C / M superchains of M consecutive chains.  Three kernels, every order a function of
// (n_keep, d, C, M) alone, no atomics:
//
//   nested_moments_kernel   one lane per chain, one workgroup per (dimension, tile of 256 chains).  The lane walks its column t ascending: a load
//                           of the wave is 512 contiguous bytes, eight rows are in flight ahead of the dependent adds.  The centred pass of the tile
//                           follows its sum pass in the same workgroup, so it re-reads what this workgroup has just pulled through the caches
//                           (n_keep * 2 KB per workgroup); n_keep = 1 has no second pass.  Writes the chain mean a and variance v as [d][C].
//   nested_super_kernel     one wave per (dimension, superchain): the 64 lanes are SUM64's lanes over the M members, which lie contiguous in a and v.
//   nested_dim_kernel       one wave per dimension over the [d][K] tables of the superchain means A and variances w.
//
// SUM64(u_0 .. u_{n-1}): lane s adds u[s + 64 j], j ascending, from +0.0; then r[s] = r[s] + r[s + h] for h = 32, 16, .., 1; the result is r[0].

#include "draws_nested.hpp"

namespace mi {
namespace dnest {

NestedPlan nested_plan(uint64_t n_keep, uint64_t d, uint64_t C, uint64_t M, bool want_super)
{
    NestedPlan p;
    p.N = n_keep; p.d = d; p.C = C; p.M = M; p.K = C / M;
    p.n_tiles = (C + NESTED_TILE - 1) / NESTED_TILE;
    p.o_a = 0;
    p.o_v = p.o_a + (size_t)d * C;
    p.o_A = p.o_v + (size_t)d * C;
    p.o_w = p.o_A + (size_t)d * p.K;
    p.o_out = p.o_w + (size_t)d * p.K;
    p.o_super = p.o_out + (size_t)3 * d;
    p.bytes = (p.o_super + (want_super ? (size_t)d * p.K : 0)) * sizeof(double);
    return p;
}

namespace {

constexpr int UNROLL = 8;

template <bool ONE_DRAW>
__global__ __launch_bounds__(NESTED_TILE) void nested_moments_kernel(const double* __restrict__ x, uint64_t N, uint64_t d, uint64_t C, uint64_t n_tiles,
                                                                      double* __restrict__ a, double* __restrict__ v)
{
    const uint64_t i = blockIdx.x / n_tiles, tile = blockIdx.x - i * n_tiles;
    const uint64_t c = tile * NESTED_TILE + threadIdx.x;
    if (c >= C) return;
    const uint64_t dC = d * C;
    const double* col = x + i * C + c;
    double s = 0.0;
    uint64_t t = 0;
    for (; t + UNROLL <= N; t += UNROLL) {                 // eight rows of the column: the loads in flight together, the additions in order
        const double* p = col + t * dC;
        double u[UNROLL];
#pragma unroll
        for (int r = 0; r < UNROLL; ++r) u[r] = p[(uint64_t)r * dC];
#pragma unroll
        for (int r = 0; r < UNROLL; ++r) s = s + u[r];
    }
    for (; t < N; ++t) s = s + col[t * dC];
    const double m = s / (double)N;
    a[i * C + c] = m;
    if constexpr (ONE_DRAW) {
        v[i * C + c] = 0.0;
    } else {
        double q = 0.0;
        for (t = 0; t + UNROLL <= N; t += UNROLL) {
            const double* p = col + t * dC;
            double u[UNROLL];
#pragma unroll
            for (int r = 0; r < UNROLL; ++r) u[r] = p[(uint64_t)r * dC];
#pragma unroll
            for (int r = 0; r < UNROLL; ++r) {
                const double e = u[r] - m;
                const double pr = e * e;
                q = q + pr;
            }
        }
        for (; t < N; ++t) {
            const double e = col[t * dC] - m;
            const double pr = e * e;
            q = q + pr;
        }
        v[i * C + c] = q / (double)(N - 1);
    }
}

// SUM64 of u(0) .. u(n - 1) by the calling wave; every lane returns r[0]
template <class F>
__device__ __forceinline__ double sum64(uint64_t n, int lane, F u)
{
    double r = 0.0;
    for (uint64_t j = (uint64_t)lane; j < n; j += 64) r = r + u(j);
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) r = r + __shfl_down(r, h, 64);      // lanes s < h hold the tree's r[s]; what the others hold is never read
    return __shfl(r, 0, 64);
}

__global__ __launch_bounds__(256) void nested_super_kernel(const double* __restrict__ a, const double* __restrict__ v, uint64_t d, uint64_t C, uint64_t M,
                                                           uint64_t K, double* __restrict__ A, double* __restrict__ w, double* __restrict__ super_kd)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wv = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // (dimension, superchain), wave-uniform
    if (wv >= d * K) return;
    const uint64_t i = wv / K, k = wv - i * K;
    const double* am = a + i * C + k * M;
    const double* vm = v + i * C + k * M;
    const double Ak = sum64(M, lane, [&](uint64_t m) { return am[m]; }) / (double)M;
    double Bk = 0.0;
    if (M >= 2)
        Bk = sum64(M, lane, [&](uint64_t m) { const double e = am[m] - Ak; return e * e; }) / (double)(M - 1);
    const double Wk = sum64(M, lane, [&](uint64_t m) { return vm[m]; }) / (double)M;
    if (lane == 0) {
        A[i * K + k] = Ak;
        w[i * K + k] = Bk + Wk;
        if (super_kd) super_kd[k * d + i] = Ak;
    }
}

__global__ __launch_bounds__(256) void nested_dim_kernel(const double* __restrict__ A, const double* __restrict__ w, uint64_t d, uint64_t K,
                                                         double* __restrict__ out /* [3][d]: mean, between, within */)
{
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= d) return;
    const double* Ai = A + i * K;
    const double* wi = w + i * K;
    const double mean = sum64(K, lane, [&](uint64_t k) { return Ai[k]; }) / (double)K;
    const double between = sum64(K, lane, [&](uint64_t k) { const double e = Ai[k] - mean; return e * e; }) / (double)(K - 1);
    const double within = sum64(K, lane, [&](uint64_t k) { return wi[k]; }) / (double)K;
    if (lane == 0) {
        out[i] = mean;
        out[d + i] = between;
        out[2 * d + i] = within;
    }
}

}  // namespace

int nested_run(const double* x, const NestedPlan& p, void* ws, bool want_super, hipStream_t st)
{
    double* W = static_cast<double*>(ws);
    const uint64_t g_moments = p.d * p.n_tiles, g_super = (p.d * p.K + 3) / 4, g_dim = (p.d + 3) / 4;
    if (g_moments > 0x7fffffffULL || g_super > 0x7fffffffULL) return (int)hipErrorInvalidValue;      // beyond any slab that fits a device
    if (p.N == 1)
        hipLaunchKernelGGL(nested_moments_kernel<true>, dim3((unsigned)g_moments), dim3(NESTED_TILE), 0, st, x, p.N, p.d, p.C, p.n_tiles, W + p.o_a, W + p.o_v);
    else
        hipLaunchKernelGGL(nested_moments_kernel<false>, dim3((unsigned)g_moments), dim3(NESTED_TILE), 0, st, x, p.N, p.d, p.C, p.n_tiles, W + p.o_a, W + p.o_v);
    hipLaunchKernelGGL(nested_super_kernel, dim3((unsigned)g_super), dim3(256), 0, st, W + p.o_a, W + p.o_v, p.d, p.C, p.M, p.K, W + p.o_A, W + p.o_w,
                       want_super ? W + p.o_super : nullptr);
    hipLaunchKernelGGL(nested_dim_kernel, dim3((unsigned)g_dim), dim3(256), 0, st, W + p.o_A, W + p.o_w, p.d, p.K, W + p.o_out);
    return (int)hipGetLastError();
}

}  // namespace dnest
}  // namespace mi
