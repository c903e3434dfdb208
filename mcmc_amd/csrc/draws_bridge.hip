// draws_bridge.hip -- the kernels of bridge sampling (mi_mcmc_bridge_proposal, mi_mcmc_bridge_estimate, mi_mcmc_draws_bridge; include/mi_mcmc.h states the
// arithmetic, draws_bridge.hpp the interface).
//
//   bridge_propose_kernel   y = mu + L z.  The tile of draws_logk.hip's product kernel: a workgroup of four waves owns 128 proposal columns, a wave 32 of
//                           them, and walks the row tiles of 128 rows ascending with the contraction in steps of 16 through a double-buffered LDS stage
//                           (draws_product.hpp).  The matrix rows of a stage are the packed L by direct-to-LDS loads; the column rows are NOT loaded: the
//                           thread that would stage rows 8 h .. 8 h + 7 of step kb of column i computes them -- they are the four Box-Muller pairs of
//                           slots 4 (2 kb + h) .. + 3 of Philox stream STREAM_BRIDGE, "chain" i, draw 0 (element 8 b + 4 h' + j of a vector is component h'
//                           of slot 4 b + j: det_math.hpp) -- one step ahead, in front of the MFMAs.  z is regenerated for every row tile, as far as the tile needs it:
//                           row tile mt runs the steps kb < 8 (mt + 1) only, what lies beyond multiplies the zeros above L's diagonal.
//                           L's upper triangle is zero, so the chain over b = 0 .. d - 1 of the MFMA is the chain over b = 0 .. a of the definition: a
//                           running sum that started from +0 is never -0, and + (+-0) leaves it as it is.  After a row tile every lane adds mu_a and
//                           stores its 64 elements (col = lane & 15, row = (lane >> 4) + 4 reg of the C/D map).
//   bridge_logg_kernel      logg of a slab's columns: draws_logk.hip's DENSE fold, with e = x - mu formed on the way into LDS (one rounded subtraction per
//                           element, the same one again where the fold needs e_i), the packed matrix Pg, and -ldh at the end.
//   the folds               one value per lane (diff, exp_shift), one piece of 16 384 per workgroup of 256 (pieces: PSIS's SUM), one chunk of 2 048 per
//                           workgroup of 64 (moments: the 64 slots, the tree).  The host adds pieces and merges chunks in ascending order.
// Nothing waits on the device; no atomics; the grids are functions of the shape: the result depends on no grid, timing or atomic order.

#include "draws_bridge.hpp"
#include "det_math.hpp"
#include "launch_common.hpp"

#include <algorithm>
#include <cmath>

namespace mi {
namespace dbridge {

using dprod::LDS_STRIDE;
using dprod::STAGE;
using dprod::double4_t;

MatPlan mat_plan(uint64_t d)
{
    MatPlan p;
    p.d = d;
    p.Kp = TK * ((d + TK - 1) / TK);
    p.ldA = TM * ((d + TM - 1) / TM);
    p.n_row_tiles = p.ldA / TM;
    p.pack_grid = cap_grid(std::min<uint64_t>((p.Kp * p.ldA + 255) / 256, 1u << 16));
    p.pack_bytes = dprod::align256((size_t)(p.Kp * p.ldA) * sizeof(double));
    return p;
}

uint64_t group_cols(uint64_t d, uint64_t N2, uint64_t budget)
{
    if (budget == 0 || budget > BRIDGE_PROP_BYTES) budget = BRIDGE_PROP_BYTES;
    uint64_t fit = 16 * std::max<uint64_t>(1, budget / (d * sizeof(double) * 16));
    if (fit >= TN) fit = TN * (fit / TN);
    return std::min(N2, fit);
}

int pack_run(const MatPlan& p, const double* M, double* At, hipStream_t st)
{
    return dprod::pack_transposed(M, p.d, p.d, p.Kp, p.ldA, p.pack_grid, At, st);
}

namespace {

__device__ __forceinline__ double combine4(double q, int c16)
{
    const double q0 = __shfl(q, c16), q1 = __shfl(q, c16 + 16), q2 = __shfl(q, c16 + 32), q3 = __shfl(q, c16 + 48);
    return (q0 + q2) + (q1 + q3);
}

struct ProposeParams {
    const double* At;        // the packed L, [Kp][ldA]
    const double* mu;        // [d]
    double* y;               // [d][ldy]
    uint64_t seed, col0, ncols, ldy, d, ldA;
    uint32_t nkb, n_row_tiles;
};

__global__ MI_NO_DS_MERGE __launch_bounds__(256, 2) void bridge_propose_kernel(const ProposeParams prm)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane >> 4, c16 = lane & 15;
    const uint64_t d = prm.d;
    const uint64_t n0 = (uint64_t)blockIdx.x * TN;
    // the column whose normals this thread generates (rows 8 s_half .. 8 s_half + 7 of every step; a column beyond the group: generated, never stored)
    const int s_c = tid & 127, s_half = tid >> 7;
    const uint64_t s_chain = prm.col0 + n0 + (uint64_t)s_c;
    uint64_t e_k[2];
    bool e_ok[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        e_k[ni] = n0 + (uint64_t)(32 * wave + 16 * ni + c16);
        e_ok[ni] = e_k[ni] < prm.ncols;
    }
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double*)lds;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    const uint32_t d32 = (uint32_t)d;
    auto issue_a = [&](uint32_t kb, uint32_t mt, int stage) __attribute__((always_inline)) {
        dprod::issue_a<4>(prm.At, prm.ldA, kb * TK, (uint64_t)mt * TM, lds_base, stage, wave, lane16);
    };
    // rows 16 kb + 8 s_half + u, u = 0 .. 7: block b = 2 kb + s_half of the vector, slots 4 b + k, component 0 -> u = k, component 1 -> u = k + 4
    auto gen_b = [&](uint32_t kb, double (&v)[8]) __attribute__((always_inline)) {
        const uint32_t slot0 = 4u * (2u * kb + (uint32_t)s_half);
#pragma unroll
        for (int k = 0; k < 4; ++k) rng_normal_pair_core(prm.seed, s_chain, 0u, slot0 + (uint32_t)k, STREAM_BRIDGE, v[k], v[k + 4]);
    };
    auto store_b = [&](uint32_t kb, int stage, const double (&v)[8]) __attribute__((always_inline)) {
        dprod::store_b<8>(lds + stage * STAGE, kb, s_half, s_c, d32, v);
    };

    double4_t acc[8][2];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
    double bv[8];
    // row tile mt holds rows < 128 (mt + 1): L_ab = 0 for b > a, so its steps kb >= 8 (mt + 1) multiply zeros and are skipped -- a sum that started
    // from +0 is left as it is by + (+-0), so no bit depends on it
    const uint32_t nkb_all = prm.nkb;
    auto steps_of = [&](uint32_t t) __attribute__((always_inline)) { const uint32_t n = 8u * (t + 1u); return n < nkb_all ? n : nkb_all; };
    uint64_t total = 0;
    for (uint32_t t = 0; t < prm.n_row_tiles; ++t) total += steps_of(t);
    uint32_t nkb = steps_of(0);
    gen_b(0, bv);
    issue_a(0, 0, 0);
    store_b(0, 0, bv);
    uint32_t kb = 0, mt = 0;
#pragma unroll 1
    for (uint64_t s = 0; s < total; ++s) {
        const int stage = (int)(s & 1u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's rows of L for step s landed ...
        __syncthreads();                                      // ... everybody's rows and columns, and nobody still reads the other stage
        uint32_t kb1 = kb + 1, mt1 = mt;
        if (kb1 == nkb) { kb1 = 0; mt1 = mt + 1; }        // (nkb: the steps of row tile mt)
        const bool more = s + 1 < total;
        if (more) { issue_a(kb1, mt1, stage ^ 1); gen_b(kb1, bv); }
        dprod::mfma_step<8>(lds + stage * STAGE + j * (int)LDS_STRIDE + c16, lds + stage * STAGE + ((int)TK + j) * (int)LDS_STRIDE + 32 * wave + c16, acc);
        if (more) store_b(kb1, stage ^ 1, bv);
        if (kb == nkb - 1) {
            // the row tile is complete: acc[ti][ni][r] is element (row 128 mt + 16 ti + 4 r + j, column e_k[ni])
            const uint64_t m0 = (uint64_t)mt * TM;
#pragma unroll
            for (int ti = 0; ti < 8; ++ti) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint64_t row = m0 + (uint64_t)(16 * ti + 4 * r + j);
                    if (row < d) {
                        const double m = prm.mu[row];
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
                            if (e_ok[ni]) prm.y[row * prm.ldy + e_k[ni]] = m + acc[ti][ni][r];
                    }
                }
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) acc[ti][ni] = double4_t{0.0, 0.0, 0.0, 0.0};
            }
        }
        kb = kb1;
        if (mt1 != mt) nkb = steps_of(mt1);
        mt = mt1;
    }
}

struct LoggParams {
    const double* At;        // the packed Pg, [Kp][ldA]
    const double* mu;        // [d]
    const double* x;         // the slab
    double* out;             // [K]
    double ldh;
    uint64_t d, C, K, ldA;
    uint32_t nkb, n_row_tiles;
};

__global__ MI_NO_DS_MERGE __launch_bounds__(256, 2) void bridge_logg_kernel(const LoggParams prm)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane >> 4, c16 = lane & 15;
    const uint64_t d = prm.d, C = prm.C, K = prm.K;
    const uint64_t n0 = (uint64_t)blockIdx.x * TN;
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
    auto issue_a = [&](uint32_t kb, uint32_t mt, int stage) __attribute__((always_inline)) {
        dprod::issue_a<4>(prm.At, prm.ldA, kb * TK, (uint64_t)mt * TM, lds_base, stage, wave, lane16);
    };
    // the column's 8 rows of step kb and their means (row min(j, d - 1) beyond d: what store_b replaces by a true zero), centred in registers
    auto load_b = [&](uint32_t kb, double (&v)[8], double (&m)[8]) __attribute__((always_inline)) {
        dprod::load_b<8>(s_col, kb, s_half, d32, C, v);
        const uint32_t j0 = kb * TK + (uint32_t)(8 * s_half);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t jj = j0 + (uint32_t)u;
            m[u] = prm.mu[jj < d32 ? jj : d32 - 1u];
        }
    };
    auto store_b = [&](uint32_t kb, int stage, const double (&v)[8], const double (&m)[8]) __attribute__((always_inline)) {
        double e[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) e[u] = v[u] - m[u];
        dprod::store_b<8>(lds + stage * STAGE, kb, s_half, s_c, d32, e);
    };

    double4_t acc[8][2];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
    double q[2] = {0.0, 0.0};
    double bv[8], bm[8];
    const uint32_t nkb = prm.nkb;
    const uint64_t total = (uint64_t)nkb * prm.n_row_tiles;
    load_b(0, bv, bm);
    issue_a(0, 0, 0);
    store_b(0, 0, bv, bm);
    uint32_t kb = 0, mt = 0;
#pragma unroll 1
    for (uint64_t s = 0; s < total; ++s) {
        const int stage = (int)(s & 1u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        uint32_t kb1 = kb + 1, mt1 = mt;
        if (kb1 == nkb) { kb1 = 0; mt1 = mt + 1; }
        const bool more = s + 1 < total;
        if (more) { load_b(kb1, bv, bm); issue_a(kb1, mt1, stage ^ 1); }
        dprod::mfma_step<8>(lds + stage * STAGE + j * (int)LDS_STRIDE + c16, lds + stage * STAGE + ((int)TK + j) * (int)LDS_STRIDE + 32 * wave + c16, acc);
        if (more) store_b(kb1, stage ^ 1, bv, bm);
        if (kb == nkb - 1) {
            // the row tile is complete: fold block 0, rotate, eight times (draws_logk.hip): the rows of a lane ascend, chain j of dot4
            const uint64_t m0 = (uint64_t)mt * TM;
#pragma unroll 1
            for (int it = 0; it < 8; ++it) {
                const uint64_t rb = m0 + (uint64_t)(16 * it);
                if (rb < d) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint64_t row = rb + (uint64_t)(4 * r + j);
                        const bool rok = row < d;
                        const double mr = rok ? prm.mu[row] : 0.0;
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) {
                            const double xv = (rok && e_ok[ni]) ? e_col[ni][row * C] : 0.0;
                            const double ev = xv - mr;
                            const double f = dfma(ev, acc[0][ni][r], q[ni]);
                            q[ni] = rok ? f : q[ni];
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
        const double h = -0.5 * dot;
        if (j == 0 && e_ok[ni]) prm.out[e_k[ni]] = h - prm.ldh;
    }
}

__global__ __launch_bounds__(256) void bridge_diff_kernel(const double* __restrict__ a, const double* __restrict__ b, uint64_t n, double* __restrict__ out)
{
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) out[k] = a[k] - b[k];
}

__global__ __launch_bounds__(256) void bridge_exp_shift_kernel(double* __restrict__ v, uint64_t n, double lstar)
{
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) v[k] = det_exp(v[k] - lstar);
}

__global__ __launch_bounds__(256) void bridge_fill_nan_kernel(double* __restrict__ v, uint64_t n)
{
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) v[k] = __longlong_as_double(0x7FF8000000000000ll);
}

// f1 = a / (s1 a + s2 r) (WHICH = 0), f2 = 1 / (s1 b + s2 r) (WHICH = 1): two products, one sum, one IEEE division
__device__ __forceinline__ double bridge_term(int which, double v, double s1, double s2r)
{
    const double sv = s1 * v;
    const double den = sv + s2r;
    return which == 0 ? v / den : 1.0 / den;
}

// workgroup p: SUM of piece p -- slot t takes v_t, v_{t + 256}, ... ascending from +0; the slots meet as u[i] += u[i + 128], + 64, ..., + 1
__global__ __launch_bounds__(256) void bridge_pieces_kernel(const double* __restrict__ a, uint64_t N2, uint64_t P2, const double* __restrict__ b, uint64_t N1,
                                                            double s1, double s2, double r, double* __restrict__ part)
{
    __shared__ double u[256];
    const uint64_t p = blockIdx.x;
    const int which = p < P2 ? 0 : 1;
    const double* v = which == 0 ? a : b;
    const uint64_t n = which == 0 ? N2 : N1;
    const uint64_t lo = (which == 0 ? p : p - P2) * BRIDGE_PIECE;
    const uint64_t hi = lo + BRIDGE_PIECE < n ? lo + BRIDGE_PIECE : n;
    const double s2r = s2 * r;
    double acc = 0.0;
    for (uint64_t k = lo + threadIdx.x; k < hi; k += 256) acc = acc + bridge_term(which, v[k], s1, s2r);
    u[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) u[threadIdx.x] = u[threadIdx.x] + u[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[p] = u[0];
}

// workgroup c: one chunk of 2 048 values of f1 (c < Q2) or f2 -- the shift is the chunk's first value; slot s = 16 w + l takes the offsets
// o = 128 T + 32 w + 16 h + l ascending (T = 0 .. 15, h = 0, 1); the tree of mi_mcmc_draws_waic
__global__ __launch_bounds__(64) void bridge_moments_kernel(const double* __restrict__ a, uint64_t N2, uint64_t Q2, const double* __restrict__ b, uint64_t N1,
                                                            double s1, double s2, double r, double* __restrict__ stat, double* __restrict__ f2_out)
{
    __shared__ double u1[64], u2[64];
    const uint64_t c = blockIdx.x;
    const int which = c < Q2 ? 0 : 1;
    const double* v = which == 0 ? a : b;
    const uint64_t n = which == 0 ? N2 : N1;
    const uint64_t lo = (which == 0 ? c : c - Q2) * BRIDGE_CHUNK;
    const uint64_t nb = lo + BRIDGE_CHUNK < n ? BRIDGE_CHUNK : n - lo;
    const double s2r = s2 * r;
    const int s = threadIdx.x, w = s >> 4, l = s & 15;
    const double sh = bridge_term(which, v[lo], s1, s2r);
    double S1 = 0.0, S2 = 0.0;
    for (int T = 0; T < 16; ++T)
        for (int h = 0; h < 2; ++h) {
            const uint64_t o = (uint64_t)(128 * T + 32 * w + 16 * h + l);
            if (o < nb) {
                const double f = bridge_term(which, v[lo + o], s1, s2r);
                if (which == 1 && f2_out) f2_out[lo + o] = f;
                const double dv = f - sh;
                const double sq = dv * dv;
                S1 = S1 + dv;
                S2 = S2 + sq;
            }
        }
    u1[s] = S1;
    u2[s] = S2;
    __syncthreads();
    for (int h = 8; h >= 1; h >>= 1) {
        if (l < h) { u1[s] = u1[s] + u1[s + h]; u2[s] = u2[s] + u2[s + h]; }
        __syncthreads();
    }
    if (s == 0) {
        stat[3 * c] = sh;
        stat[3 * c + 1] = (u1[0] + u1[16]) + (u1[32] + u1[48]);
        stat[3 * c + 2] = (u2[0] + u2[16]) + (u2[32] + u2[48]);
    }
}

unsigned stride_grid(uint64_t n) { return (unsigned)cap_grid(std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 1u << 16))); }

}  // namespace

int propose_run(const MatPlan& p, const double* At_L, const double* mu, uint64_t seed, uint64_t col0, uint64_t ncols, uint64_t ldy, double* y, hipStream_t st)
{
    auto kern = bridge_propose_kernel;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BRIDGE_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    ProposeParams prm;
    prm.At = At_L; prm.mu = mu; prm.y = y;
    prm.seed = seed; prm.col0 = col0; prm.ncols = ncols; prm.ldy = ldy; prm.d = p.d; prm.ldA = p.ldA;
    prm.nkb = (uint32_t)(p.Kp / TK);
    prm.n_row_tiles = (uint32_t)p.n_row_tiles;
    hipLaunchKernelGGL(kern, dim3((unsigned)((ncols + TN - 1) / TN)), dim3(256), BRIDGE_LDS_BYTES, st, prm);
    return (int)hipGetLastError();
}

int logg_run(const MatPlan& p, const double* At_P, const double* mu, double ldh, const double* x, uint64_t n_keep, uint64_t C, double* out, hipStream_t st)
{
    auto kern = bridge_logg_kernel;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BRIDGE_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    LoggParams prm;
    prm.At = At_P; prm.mu = mu; prm.x = x; prm.out = out; prm.ldh = ldh;
    prm.d = p.d; prm.C = C; prm.K = n_keep * C; prm.ldA = p.ldA;
    prm.nkb = (uint32_t)(p.Kp / TK);
    prm.n_row_tiles = (uint32_t)p.n_row_tiles;
    hipLaunchKernelGGL(kern, dim3((unsigned)((prm.K + TN - 1) / TN)), dim3(256), BRIDGE_LDS_BYTES, st, prm);
    return (int)hipGetLastError();
}

int diff_run(const double* a, const double* b, uint64_t n, double* out, hipStream_t st)
{
    hipLaunchKernelGGL(bridge_diff_kernel, dim3(stride_grid(n)), dim3(256), 0, st, a, b, n, out);
    return (int)hipGetLastError();
}

int exp_shift_run(double* v, uint64_t n, double lstar, hipStream_t st)
{
    hipLaunchKernelGGL(bridge_exp_shift_kernel, dim3(stride_grid(n)), dim3(256), 0, st, v, n, lstar);
    return (int)hipGetLastError();
}

int fill_nan_run(double* v, uint64_t n, hipStream_t st)
{
    hipLaunchKernelGGL(bridge_fill_nan_kernel, dim3(stride_grid(n)), dim3(256), 0, st, v, n);
    return (int)hipGetLastError();
}

int pieces_run(const double* a, uint64_t N2, const double* b, uint64_t N1, double s1, double s2, double r, double* part, hipStream_t st)
{
    const uint64_t P2 = n_pieces(N2), P1 = n_pieces(N1);
    hipLaunchKernelGGL(bridge_pieces_kernel, dim3((unsigned)(P2 + P1)), dim3(256), 0, st, a, N2, P2, b, N1, s1, s2, r, part);
    return (int)hipGetLastError();
}

int moments_run(const double* a, uint64_t N2, const double* b, uint64_t N1, double s1, double s2, double r, double* stat, double* f2_out, hipStream_t st)
{
    const uint64_t Q2 = n_chunks(N2), Q1 = n_chunks(N1);
    hipLaunchKernelGGL(bridge_moments_kernel, dim3((unsigned)(Q2 + Q1)), dim3(64), 0, st, a, N2, Q2, b, N1, s1, s2, r, stat, f2_out);
    return (int)hipGetLastError();
}

}  // namespace dbridge
}  // namespace mi
