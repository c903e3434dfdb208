// draw_stats_lags.hpp -- every autocovariance lag of LONG series of a draws slab [n_keep][d][C], on the fp64 matrix cores (mi_mcmc_draw_stats_lags,
// draw_stats.hip).  stats_gram_kernel (draw_stats.hpp) keeps one accumulator per block (tb, sb) of G = V V', which stops at n = 128: the upper
// triangle is NB (NB + 1) / 2 blocks of 8 registers.  The lags only need the DIAGONAL sums of G, and those need one 16 x 16 accumulator per block
// OFFSET delta = sb - tb:
//     A_delta = sum_tb sum_(chain quads) V_tb V_(tb + delta)',        V_tb = rows [16 tb, 16 tb + 16) of the centred series, 4 chains wide,
// one v_mfma_f64_16x16x4_f64 per (tb, quad, delta): fragment tb of a quad -- lane l holds v[16 tb + (l & 15)][4 cg + (l >> 4)] -- is the A operand of
// its own row block and the B operand of the row blocks tb - delta.  With the f64 C/D map col = l & 15, row = (l >> 4) + 4 r, element (row, col) of
// A_delta belongs to lag 16 delta + col - row: the elements col >= row of A_0 and every element of A_delta, delta >= 1, count each pair (t, t + k) once.
// Lags 0 .. K need the offsets [0, ND), ND = floor((K + 15) / 16) + 1; the host asks for them in BANDS [d_a, d_b) of at most 16 offsets (draw_stats.hip
// states the schedule), one launch per band, and with acov == NULL only for the dimensions whose Geyer sum is still open.
//
// Workgroup = 4 waves, one per SIMD, for (dimension, chain group); it walks its chains in tiles of 16 (wave w owns quad w) and the series in time
// tiles of T = 128 rows: the A rows [t0, t0 + T) and the B rows [t0 + 16 d_a, t0 + T + 16 d_b) sit in LDS as [row][chain] with a row stride of 18
// doubles (lanes l < 32 read the doubles 18 (l & 15) + (l >> 4): 32 different banks of 8 bytes, conflict-free ds_read_b64), 18 KB + 37 KB (NDB = 8) or
// 55 KB (NDB = 16) whatever n_keep is: two workgroups per CU.  Per step tb the wave reads ONE new B fragment into a window of NDB registers whose slot
// indices are compile-time constants (the eight steps of a tile are unrolled), the A fragment, and issues NDB MFMAs: NDB accumulators of 8 registers.
// Rows t >= n and chains past the group's last are zeros in LDS.  Centring is that of the streamed routes of mi_mcmc_draw_stats, v = (x - a_j) - e_j.
// At the end the four waves add their accumulators into LDS one after the other (wave 0, 1, 2, 3) and thread o sums one diagonal of one offset in
// ascending row order: out[g][jj][dl][m], m = col - row + 15.  The host adds the chain groups in ascending order and the two offsets a lag straddles:
// nothing depends on the grid, on timing or on atomics.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi {
namespace dlags {

constexpr int LAGS_T = 128;               // A rows per time tile
constexpr int LAGS_TC = 16;               // chains per tile: one quad per wave
constexpr int LAGS_RS = 18;               // LDS row stride in doubles
constexpr int LAGS_DIAGS = 32;            // out stride per offset: the 31 diagonals m = col - row + 15, one slot of padding
constexpr size_t lags_lds_bytes(int ndb) { return (size_t)(2 * LAGS_T + 16 * ndb) * LAGS_RS * sizeof(double); }

typedef double double4_lags __attribute__((ext_vector_type(4)));

template <int NDB>
__global__ __launch_bounds__(256, 2) void stats_band_kernel(const double* __restrict__ draws, const double* __restrict__ mean, uint32_t n, uint32_t d, uint64_t C,
                                                         uint32_t G, const uint32_t* __restrict__ dims, uint32_t d_a, double* __restrict__ out)
{
    constexpr int T = LAGS_T, TB = T / 16, RS = LAGS_RS, TC = LAGS_TC, BR = T + 16 * NDB;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* const Abuf = lds;                           // [T][RS]
    double* const Bbuf = lds + (size_t)T * RS;          // [BR][RS]
    const uint32_t jj = blockIdx.x, g = blockIdx.y, nd = gridDim.x;
    const uint32_t j = dims ? dims[jj] : jj;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t per = (C + G - 1) / G;
    const uint64_t c_lo = (uint64_t)g * per, c_hi = (c_lo + per < C) ? c_lo + per : C;
    const double mj = mean[j], ej = mean[d + j];        // the centre in two parts: v = (x - mj) - ej
    const size_t row = (size_t)d * C;
    // The barrier of the tile loop orders LDS traffic only (draw_stats.hpp: __syncthreads() is a workgroup-scope fence as well and would drain
    // global loads in flight)
    auto lds_barrier = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    double4_lags acc[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i) acc[i] = double4_lags{0.0, 0.0, 0.0, 0.0};
    const uint32_t b_off = 16u * d_a;                   // first B row of a tile, relative to its first A row
    const uint32_t lr = (uint32_t)tid >> 4, lc = (uint32_t)tid & 15;    // this thread's row (mod 16) and chain of a tile's loads
    for (uint64_t c0 = c_lo; c0 < c_hi; c0 += TC) {
        const uint64_t c = c0 + lc;
        const bool on = c < c_hi;
        const double* p = draws + (size_t)j * C + (on ? c : c_hi - 1);
        for (uint32_t t0 = 0; t0 < n && t0 + b_off < n; t0 += T) {      // (a tile whose B rows all lie past the series adds nothing)
            // 8 row groups (128 rows) in flight per thread at a time: the A rows, then the B rows in chunks
            auto load = [&](double* buf, uint32_t first, int u0) __attribute__((always_inline)) {
                double xr[TB];
#pragma unroll
                for (int u = 0; u < TB; ++u) { const uint32_t t = first + 16u * (u0 + u) + lr; xr[u] = p[(size_t)(t < n ? t : n - 1) * row]; }
#pragma unroll
                for (int u = 0; u < TB; ++u) {
                    const uint32_t t = first + 16u * (u0 + u) + lr;
                    buf[(16 * (u0 + u) + lr) * RS + lc] = (on && t < n) ? (xr[u] - mj) - ej : 0.0;
                }
            };
            load(Abuf, t0, 0);
#pragma unroll
            for (int ch = 0; ch < BR / T; ++ch) load(Bbuf, t0 + b_off, ch * TB);
            lds_barrier();
            const double* fa = Abuf + (size_t)(lane & 15) * RS + 4 * wave + (lane >> 4);
            const double* fb = Bbuf + (size_t)(lane & 15) * RS + 4 * wave + (lane >> 4);
            double win[NDB];                            // slot s holds B block s (mod NDB) of the blocks [tb, tb + NDB)
#pragma unroll
            for (int s = 0; s < NDB - 1; ++s) win[s] = fb[(size_t)(16 * s) * RS];
#pragma unroll
            for (int tb = 0; tb < TB; ++tb) {
                win[(tb + NDB - 1) % NDB] = fb[(size_t)(16 * (tb + NDB - 1)) * RS];
                const double a = fa[(size_t)(16 * tb) * RS];
#pragma unroll
                for (int dl = 0; dl < NDB; ++dl) acc[dl] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, win[(tb + dl) % NDB], acc[dl], 0, 0, 0);
            }
            lds_barrier();                              // everybody is done with the tile
        }
    }
    // ---- the four waves' accumulators, added in LDS in the order 0, 1, 2, 3; then the diagonals
    double* const M = lds;                              // [NDB][16][16]
    for (int wv = 0; wv < 4; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int dl = 0; dl < NDB; ++dl)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double* m_ = M + (size_t)dl * 256 + (size_t)(4 * r + (lane >> 4)) * 16 + (lane & 15);
                    *m_ = (wv == 0) ? acc[dl][r] : *m_ + acc[dl][r];
                }
        }
        __syncthreads();
    }
    for (int o = tid; o < NDB * LAGS_DIAGS; o += 256) {
        const int dl = o / LAGS_DIAGS, m = o % LAGS_DIAGS, r = m - 15;      // lag 16 (d_a + dl) + r
        double s_ = 0.0;
        if (m < 31 && !(d_a + (uint32_t)dl == 0 && r < 0)) {
            const int r_lo = r < 0 ? -r : 0, r_hi = r < 0 ? 15 : 15 - r;
            for (int rw = r_lo; rw <= r_hi; ++rw) s_ += M[(size_t)dl * 256 + (size_t)rw * 16 + rw + r];
        }
        out[(((size_t)g * nd + jj) * NDB + dl) * LAGS_DIAGS + m] = s_;
    }
}

// The R-hat moments of every dimension: out2[g][j][0..3) = sum over the group's chains of the chain mean m_c of the centred series, of m_c^2 and of the
// chain's unbiased variance (0 when n = 1).  One lane per chain, two passes over its series (the second out of the caches): the squared deviations
// are taken from the chain's own mean (draw_stats.hpp says why a one-pass variance about the pooled centre will not do).
__global__ __launch_bounds__(64) void stats_moments_kernel(const double* __restrict__ draws, const double* __restrict__ mean, uint32_t n, uint32_t d, uint64_t C,
                                                           uint32_t G, double* __restrict__ out2)
{
    const uint32_t j = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
    const uint64_t per = (C + G - 1) / G;
    const uint64_t c_lo = (uint64_t)g * per, c_hi = (c_lo + per < C) ? c_lo + per : C;
    const double mj = mean[j], ej = mean[d + j];
    const size_t row = (size_t)d * C;
    double sm = 0.0, sm2 = 0.0, sv = 0.0;
    for (uint64_t c0 = c_lo; c0 < c_hi; c0 += 64) {
        const uint64_t c = c0 + lane;
        const bool on = c < c_hi;
        const double* p = draws + (size_t)j * C + (on ? c : c_hi - 1);
        double s1 = 0.0;
        for (uint32_t t = 0; t < n; ++t) s1 += (p[(size_t)t * row] - mj) - ej;
        const double mc = s1 / (double)n;
        double ss = 0.0;
        for (uint32_t t = 0; t < n; ++t) { const double e = ((p[(size_t)t * row] - mj) - ej) - mc; ss = __builtin_fma(e, e, ss); }
        if (on) { sm += mc; sm2 = __builtin_fma(mc, mc, sm2); sv += (n > 1) ? ss / (double)(n - 1) : 0.0; }
    }
    for (int m = 32; m >= 1; m >>= 1) { sm += __shfl_xor(sm, m); sm2 += __shfl_xor(sm2, m); sv += __shfl_xor(sv, m); }
    if (lane == 0) { double* o = out2 + ((size_t)g * d + j) * 3; o[0] = sm; o[1] = sm2; o[2] = sv; }
}

}  // namespace dlags
}  // namespace mi
