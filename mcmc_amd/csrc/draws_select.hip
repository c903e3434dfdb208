// draws_select.hip -- exact pooled order statistics of a draws slab (mi_mcmc_draws_order_stats / mi_mcmc_draws_quantiles; include/mi_mcmc.h states the
// key, the order and the quantile rule; draws_select.hpp the plan).
//
// Most-significant-digit radix selection on the 64-bit keys: 8-bit digits, 8 rounds.  Every (dimension, rank) pair keeps in device memory its key
// prefix and the remaining rank inside that prefix; after round r the prefix holds 8 r bits.  A round is two launches on the caller's stream, nothing
// waits on the device and the host is not asked between rounds:
//
//   sel_hist_kernel   a workgroup owns a contiguous piece of one row [t][i][.] or several whole rows of one dimension (the plan).  It finds the DISTINCT
//                     prefixes of its dimension's ranks (ranks that share a prefix share a histogram: slot = the first rank with that prefix), keeps
//                     them in LDS, forms the keys of a batch of elements per lane, compares them with the distinct prefixes only (one LDS read of a prefix serves the batch) and counts the next digit of a match
//                     in an LDS histogram [distinct][256] of 32-bit counts.  The counts are pre-aggregated per wave, because the digits are skewed:
//                     round 1's digit is the sign and seven exponent bits (posterior draws fall into two to four bins), and a slab of equal values
//                     has one bin in every round -- 64 lanes incrementing one LDS word would serialise.  Up to four times the wave takes the bin of
//                     its first uncounted lane, ballots the lanes that agree and lets one lane add the popcount (all lanes equal: one add); what is
//                     left after four bins is spread out, and those lanes add 1 each.  Loads: 16 bytes per lane on the aligned body of a row piece,
//                     8 bytes for a peeled head and tail (a row starts at byte 8 C (t d + i): 16-byte aligned only when that is even); rows shorter
//                     than SEL_SMALL_C are walked flattened with 8-byte loads so that every lane has an element.  Round 1 (one empty prefix per
//                     dimension) STORES its 256 counts as the workgroup's partial histogram; later rounds ADD their non-zero counts to the global
//                     64-bit histogram [dimension][slot][256] (K can exceed 2^32);
//   sel_scan_kernel   one workgroup per dimension, one wave per rank in turn: 4 bins per lane, a wave prefix sum, the lane whose bins contain the
//                     remaining rank appends the digit to the prefix and subtracts the counts below it (the new state goes to the OTHER image: the
//                     waves of a dimension read each other's old prefixes).  Round 1 first sums the workgroups' partials.  Then the workgroup CLEARS
//                     the histograms the next round adds to: after round 1 all of the dimension's slots, later the slots this round used -- so a call
//                     never reads a count it did not make, whatever an earlier call left in the cached workspace;
//   sel_final_kernel  after round 8 the prefix is the key: inverted into out[rank][dimension] (a NaN key: the canonical quiet NaN).
//
// Counts are integers: the result depends on no grid, timing or atomic order.

#include "draws_select.hpp"

#include <algorithm>
#include <type_traits>

namespace mi {
namespace dsel {

typedef double double2_t __attribute__((ext_vector_type(2)));

struct SelState { uint64_t prefix, rem; };

SelPlan sel_plan(uint64_t n_keep, uint64_t d, uint64_t C, uint32_t n_ranks)
{
    SelPlan p;
    p.K = n_keep * C;
    p.target = std::max<uint64_t>(SEL_TARGET, (p.K + (1ull << 20) - 1) >> 20);
    if (C >= p.target) { p.P = (C + p.target - 1) / p.target; p.piece = (C + p.P - 1) / p.P; p.rows_per_wg = 1; }
    else { p.P = 1; p.piece = C; p.rows_per_wg = p.target / C; }
    p.wg_per_dim = ((n_keep + p.rows_per_wg - 1) / p.rows_per_wg) * p.P;
    const uint64_t by_bytes = SEL_HIST_BOUND / ((uint64_t)n_ranks * 2048 + p.wg_per_dim * 1024);
    const uint64_t by_blocks = SEL_MAX_BLOCKS / p.wg_per_dim;
    p.dims_per_group = std::min<uint64_t>(d, std::max<uint64_t>(1, std::min(by_bytes, by_blocks)));
    p.n_groups = (d + p.dims_per_group - 1) / p.dims_per_group;
    const size_t state = (size_t)d * n_ranks * sizeof(SelState);
    p.o_state0 = 0;
    p.o_state1 = p.o_state0 + state;
    p.o_out = p.o_state1 + state;
    p.o_part = p.o_out + (size_t)n_ranks * d * sizeof(double);
    p.o_hist = p.o_part + (size_t)p.dims_per_group * p.wg_per_dim * 256 * sizeof(uint32_t);
    p.o_hist = (p.o_hist + 15) & ~(size_t)15;
    p.bytes = p.o_hist + (size_t)p.dims_per_group * n_ranks * 256 * sizeof(uint64_t);
    return p;
}

namespace {

// ROUND: 0-based; the prefix holds 8 * ROUND bits.  ROUND 0 is its own instantiation (no state is read, the counts are stored, not added).
template <bool FIRST>
__global__ __launch_bounds__(256) void sel_hist_kernel(const double* __restrict__ x, uint64_t n_keep, uint64_t d, uint64_t C, uint64_t dim0, uint32_t n_ranks,
                                                       uint32_t round, uint64_t P, uint64_t piece, uint64_t rows_per_wg, uint32_t wg_per_dim,
                                                       const SelState* __restrict__ state, uint32_t* __restrict__ part,
                                                       unsigned long long* __restrict__ hist)
{
    extern __shared__ uint32_t cnt[];                    // [distinct prefixes][256]
    __shared__ uint64_t s_raw[SEL_MAX_RANKS], s_pref[SEL_MAX_RANKS];
    __shared__ uint32_t s_slot[SEL_MAX_RANKS], s_ndist;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t dl = blockIdx.x / wg_per_dim, w = blockIdx.x % wg_per_dim;
    const uint64_t i = dim0 + dl;
    const uint32_t n_slots = FIRST ? 1u : n_ranks;
    for (uint32_t k = tid; k < n_slots * 256; k += 256) cnt[k] = 0;
    if (!FIRST) {
        if (tid < n_ranks) s_raw[tid] = state[i * n_ranks + tid].prefix;
        __syncthreads();
        if (wave == 0) {                                 // n_ranks <= 32: all of them in the first wave
            bool first = tid < n_ranks;
            if (first) {
                const uint64_t mine = s_raw[tid];
                for (uint32_t b = 0; b < tid; ++b) first = first && s_raw[b] != mine;
            }
            const uint64_t m = __ballot(first);
            if (first) {
                const uint32_t j = (uint32_t)__popcll(m & ((1ull << lane) - 1));
                s_pref[j] = s_raw[tid];
                s_slot[j] = tid;
            }
            if (tid == 0) s_ndist = (uint32_t)__popcll(m);
        }
    }
    __syncthreads();
    const uint32_t n_dist = FIRST ? 1u : s_ndist;
    const uint32_t hs = FIRST ? 0u : 64 - 8 * round, ds = 56 - 8 * round;      // FIRST: no prefix to compare, hs is not used

    // the bins of N elements per lane (valid or not): the prefixes are compared batch by batch, one LDS read of a prefix serving N compares
    auto bins = [&](const double* v, const bool* ok, int* bin, auto n_tag) __attribute__((always_inline)) {
        constexpr int N = decltype(n_tag)::value;
        uint64_t hi[N];
        uint32_t dg[N];
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const uint64_t key = sel_key(v[u]);
            dg[u] = (uint32_t)(key >> ds) & 255u;
            hi[u] = ok[u] ? key >> hs : ~0ull;           // a prefix has at most 56 bits: ~0 matches none
            bin[u] = (FIRST && ok[u]) ? (int)dg[u] : -1;
        }
        if (!FIRST)
            for (uint32_t j = 0; j < n_dist; ++j) {
                const uint64_t pj = s_pref[j];
#pragma unroll
                for (int u = 0; u < N; ++u)
                    if (hi[u] == pj) bin[u] = (int)(j * 256 + dg[u]);
            }
    };
    // one bin per lane (-1: none), all lanes of the wave arrive
    auto add = [&](int bin) __attribute__((always_inline)) {
        uint64_t rest = __ballot(bin >= 0);
        for (int it = 0; it < 4 && rest; ++it) {
            const int leader = __ffsll((unsigned long long)rest) - 1;
            const int b = __builtin_amdgcn_readlane(bin, leader);
            const uint64_t m = __ballot(bin == b);
            if ((int)lane == leader) atomicAdd(&cnt[b], (uint32_t)__popcll(m));
            rest &= ~m;
        }
        if ((rest >> lane) & 1) atomicAdd(&cnt[bin], 1u);
    };

    const uint64_t t0 = (uint64_t)(w / P) * rows_per_wg;
    const uint64_t t1 = t0 + rows_per_wg < n_keep ? t0 + rows_per_wg : n_keep;
    uint64_t c0 = (uint64_t)(w % P) * piece;
    const uint64_t c1 = c0 + piece < C ? c0 + piece : C;
    if (c0 > c1) c0 = c1;
    if (C < SEL_SMALL_C) {                               // whole short rows (P = 1), flattened: element e is (row e / C, chain e % C)
        const uint32_t C32 = (uint32_t)C;
        const uint32_t total = (uint32_t)(t1 - t0) * C32;
        for (uint32_t base = 0; base < total; base += 4 * 256) {
            double v[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t e = base + u * 256 + tid;
                ok[u] = e < total;
                const uint32_t r = e / C32, c = e - r * C32;
                v[u] = ok[u] ? x[((t0 + r) * d + i) * C + c] : 0.0;
            }
            int bin[4];
            bins(v, ok, bin, std::integral_constant<int, 4>{});
#pragma unroll
            for (int u = 0; u < 4; ++u) add(bin[u]);
        }
    } else {
        const uint32_t n = (uint32_t)(c1 - c0);
        for (uint64_t t = t0; t < t1; ++t) {
            const double* p = x + (t * d + i) * C + c0;
            const uint32_t head = (n && ((uintptr_t)p & 8)) ? 1u : 0u;
            const uint32_t body = (n - head) / 2, tail = n - head - 2 * body;
            const double2_t* p2 = reinterpret_cast<const double2_t*>(p + head);
            for (uint32_t base = 0; base < body; base += 4 * 256) {
                double v[8];
                bool ok[8];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t e = base + u * 256 + tid;
                    ok[2 * u] = ok[2 * u + 1] = e < body;
                    const double2_t v2 = ok[2 * u] ? p2[e] : double2_t{0.0, 0.0};
                    v[2 * u] = v2.x;
                    v[2 * u + 1] = v2.y;
                }
                int bin[8];
                bins(v, ok, bin, std::integral_constant<int, 8>{});
#pragma unroll
                for (int u = 0; u < 8; ++u) add(bin[u]);
            }
            if (wave == 0 && (head | tail)) {            // lane 0: the head, lane 1: the tail
                const bool ok = (lane == 0 && head) || (lane == 1 && tail);
                const double v = ok ? p[lane == 0 ? 0 : n - 1] : 0.0;
                int bin;
                bins(&v, &ok, &bin, std::integral_constant<int, 1>{});
                add(bin);
            }
        }
    }
    __syncthreads();
    if (FIRST) part[((uint64_t)dl * wg_per_dim + w) * 256 + tid] = cnt[tid];
    else
        for (uint32_t j = 0; j < n_dist; ++j) {
            const uint32_t c = cnt[j * 256 + tid];
            if (c) atomicAdd(&hist[((uint64_t)dl * n_ranks + s_slot[j]) * 256 + tid], (unsigned long long)c);
        }
}

template <bool FIRST>
__global__ __launch_bounds__(256) void sel_scan_kernel(uint64_t dim0, uint32_t n_ranks, SelRanks ranks, uint32_t wg_per_dim, const uint32_t* __restrict__ part,
                                                       unsigned long long* __restrict__ hist, const SelState* __restrict__ in, SelState* __restrict__ out)
{
    __shared__ unsigned long long s_cnt[256];
    __shared__ uint64_t s_pref[SEL_MAX_RANKS];
    __shared__ uint32_t s_slot[SEL_MAX_RANKS];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t dl = blockIdx.x;
    const uint64_t i = dim0 + dl;
    if (FIRST) {
        unsigned long long s = 0;
        const uint32_t* p = part + (uint64_t)dl * wg_per_dim * 256 + tid;
        for (uint32_t w = 0; w < wg_per_dim; ++w) s += p[(uint64_t)w * 256];
        s_cnt[tid] = s;
    } else {
        if (tid < n_ranks) s_pref[tid] = in[i * n_ranks + tid].prefix;
        __syncthreads();
        if (tid < n_ranks) {                             // the histogram of a rank: that of the first rank with its prefix
            const uint64_t mine = s_pref[tid];
            uint32_t slot = tid;
            for (uint32_t b = tid; b-- > 0;) if (s_pref[b] == mine) slot = b;
            s_slot[tid] = slot;
        }
    }
    __syncthreads();
    for (uint32_t a = wave; a < n_ranks; a += 4) {
        uint64_t prefix = 0, rem;
        unsigned long long c[4];
        if (FIRST) {
            rem = ranks.r[a];
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = s_cnt[4 * lane + k];
        } else {
            prefix = s_pref[a];
            rem = in[i * n_ranks + a].rem;
            const unsigned long long* h = hist + ((uint64_t)dl * n_ranks + s_slot[a]) * 256 + 4 * lane;
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = h[k];
        }
        const unsigned long long s4 = c[0] + c[1] + c[2] + c[3];
        unsigned long long incl = s4;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long up = __shfl_up(incl, off);
            if ((int)lane >= off) incl += up;
        }
        const unsigned long long excl = incl - s4;
        if (rem >= excl && rem < incl) {                 // exactly one lane: the counts of a prefix add up to more than its remaining rank
            uint64_t r = rem - excl;
            uint32_t k = 0;
            if (r >= c[0]) { r -= c[0]; k = 1; if (r >= c[1]) { r -= c[1]; k = 2; if (r >= c[2]) { r -= c[2]; k = 3; } } }
            SelState s;
            s.prefix = (prefix << 8) | (uint64_t)(4 * lane + k);
            s.rem = r;
            out[i * n_ranks + a] = s;
        }
    }
    __syncthreads();                                     // every rank has read its histogram: clear what the next round adds to
    for (uint32_t a = 0; a < n_ranks; ++a)
        if (FIRST || s_slot[a] == a) hist[((uint64_t)dl * n_ranks + a) * 256 + tid] = 0;
}

__global__ __launch_bounds__(256) void sel_final_kernel(const SelState* __restrict__ state, uint64_t d, uint64_t dim0, uint64_t n_dims, uint32_t n_ranks,
                                                        double* __restrict__ out)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_dims * n_ranks) return;
    const uint64_t i = dim0 + e / n_ranks;
    const uint32_t a = (uint32_t)(e % n_ranks);
    out[(uint64_t)a * d + i] = sel_unkey(state[i * n_ranks + a].prefix);
}

}  // namespace

int sel_run(const double* x, uint64_t n_keep, uint64_t d, uint64_t C, const SelRanks& ranks, uint32_t n_ranks, const SelPlan& p, void* ws, hipStream_t st)
{
    char* W = static_cast<char*>(ws);
    SelState* state[2] = {reinterpret_cast<SelState*>(W + p.o_state0), reinterpret_cast<SelState*>(W + p.o_state1)};
    double* out = reinterpret_cast<double*>(W + p.o_out);
    uint32_t* part = reinterpret_cast<uint32_t*>(W + p.o_part);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(W + p.o_hist);
    const uint32_t wg = (uint32_t)p.wg_per_dim;
    for (uint64_t dim0 = 0; dim0 < d; dim0 += p.dims_per_group) {
        const uint64_t nd = std::min<uint64_t>(p.dims_per_group, d - dim0);
        const dim3 g_hist((unsigned)(nd * wg)), g_scan((unsigned)nd), b(256);
        for (uint32_t round = 0; round < 8; ++round) {
            const SelState* in = state[round & 1];       // round 0 reads none; round 7 leaves the keys in state[0]
            SelState* nxt = state[(round + 1) & 1];
            if (round == 0) {
                hipLaunchKernelGGL(sel_hist_kernel<true>, g_hist, b, 1024, st, x, n_keep, d, C, dim0, n_ranks, round, p.P, p.piece, p.rows_per_wg, wg, in, part, hist);
                hipLaunchKernelGGL(sel_scan_kernel<true>, g_scan, b, 0, st, dim0, n_ranks, ranks, wg, part, hist, in, nxt);
            } else {
                hipLaunchKernelGGL(sel_hist_kernel<false>, g_hist, b, (size_t)n_ranks * 1024, st, x, n_keep, d, C, dim0, n_ranks, round, p.P, p.piece, p.rows_per_wg, wg,
                                   in, part, hist);
                hipLaunchKernelGGL(sel_scan_kernel<false>, g_scan, b, 0, st, dim0, n_ranks, ranks, wg, part, hist, in, nxt);
            }
        }
        hipLaunchKernelGGL(sel_final_kernel, dim3((unsigned)((nd * n_ranks + 255) / 256)), b, 0, st, state[0], d, dim0, nd, n_ranks, out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return (int)hipSuccess;
}

}  // namespace dsel
}  // namespace mi
