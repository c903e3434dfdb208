// draws_rank.hip -- exact ranks and normal scores of the retained samples of a draws slab (mi_mcmc_draws_rank_transform, and beneath
// mi_mcmc_draw_stats_ranked; include/mi_mcmc.h states the retained rows, the value ranked, the key, the rank and the score; draws_rank.hpp the plan).
//
// Per group of dimensions, all plain launches on the caller's stream; nothing waits on the device:
//
//   rank_keys_kernel     a workgroup owns one tile of RANK_TILE consecutive keys s = r * C + c of one dimension's image [S].  It walks the row pieces
//                        [t(r)][i][c0, c1) the tile covers -- 16-byte loads on the aligned body of a piece, 8-byte loads for a peeled head and tail
//                        (a row starts at byte 8 C (t d + i): 16-byte aligned only when that is even); rows shorter than RANK_SMALL_C flattened with
//                        8-byte loads --, forms key(v) (v = x, or |x - med_i|: one subtraction, the sign cleared), stores it and counts its eight
//                        digits in LDS histograms [8][256], pre-aggregated per wave as in sel_hist_kernel (digits of posterior draws are skewed);
//                        the non-zero counts are added to the dimension's histograms in device memory (integer adds: no order matters);
//   rank_const_kernel    ORs into eight flags whether a digit takes more than one value in any dimension of the group.  The host reads the 32
//                        bytes back -- the one wait of a sort -- and skips the passes of constant digits: they would move no key past another;
//   per executed pass, from the lowest digit up, between the two images:
//   rank_count_kernel    the digit counts of every tile, [dimension][digit][tile], 32 bits, every entry STORED (the cached workspace may hold
//                        an earlier call's counts: nothing is added to them);
//   rank_scan_kernel     one workgroup per dimension: the exclusive prefix sum over digit-major, tile-minor, in place;
//   rank_scatter_kernel  a wave owns a quarter of the tile, in element order, and walks it in chunks of 64 keys.  First the per-wave digit counts
//                        (LDS), prefixed over the four waves in element order on top of the tile's offsets; then per chunk eight ballots over the
//                        digit's bits give every lane its peers (the lanes with the same digit): position = the wave's running offset of the digit
//                        + popcount of the peers below the lane, and the lowest peer advances the offset by the popcount of all of them.  Stable,
//                        so the result is the unique sorted image whatever the timing;
//   rank_lookup_kernel   one thread per output element recomputes key(v) and finds lo (keys below) and hi (keys not above) in its dimension's
//                        sorted image: lo in two levels -- every RANK_STRIDE-th sorted key in LDS, then at most 13 probes inside one 32 KB window --, hi by
//                        galloping up from lo (two probes where the key is unique).
//                        Workgroups are numbered dimension-major, so a dimension's image, row stream and output pass the cache together.
//   rank_os_kernel       (fold, stats) order statistics straight out of the sorted image of the un-folded keys;
//   rank_indicator_kernel (stats) 1{x <= q_i} in the split layout.

#include "draws_rank.hpp"
#include "draws_select.hpp"
#include "det_math.hpp"

#include <algorithm>
#include <atomic>

namespace mi {
namespace drank {

namespace { std::atomic<uint64_t> g_sorts{0}, g_passes{0}; }
void rank_counts(uint64_t* sorts, uint64_t* passes)
{
    if (sorts) *sorts = g_sorts.load(std::memory_order_relaxed);
    if (passes) *passes = g_passes.load(std::memory_order_relaxed);
}

using dsel::sel_key;
using dsel::sel_unkey;

typedef double double2_t __attribute__((ext_vector_type(2)));

namespace {
inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
}

uint64_t rank_dim_bytes(uint64_t n_keep, uint64_t C, uint32_t flags, bool slab)
{
    const uint64_t rows = (flags & RANK_SPLIT) ? 2 * (n_keep / 2) : n_keep;
    const uint64_t S = rows * C, n_tiles = (S + RANK_TILE - 1) / RANK_TILE;
    return 16 * S + 1024 * n_tiles + 8192 + (slab ? 8 * S : 0);
}

RankPlan rank_plan(uint64_t n_keep, uint64_t d, uint64_t C, uint32_t flags, bool slab, uint64_t budget)
{
    RankPlan p;
    p.n_keep = n_keep; p.d = d; p.C = C; p.flags = flags;
    p.h = n_keep / 2;
    p.rows = (flags & RANK_SPLIT) ? 2 * p.h : n_keep;
    p.S = p.rows * C;
    p.n_tiles = (p.S + RANK_TILE - 1) / RANK_TILE;
    p.stride = RANK_STRIDE;
    while ((p.S + p.stride - 1) / p.stride > RANK_MAX_SAMPLES) p.stride *= 2;
    p.n_samples = (uint32_t)((p.S + p.stride - 1) / p.stride);
    p.dim_bytes = rank_dim_bytes(n_keep, C, flags, slab);
    if (budget == 0 || budget > RANK_WS_BUDGET) budget = RANK_WS_BUDGET;
    const uint64_t by_bytes = budget / std::max<uint64_t>(1, p.dim_bytes);
    const uint64_t by_blocks = RANK_MAX_BLOCKS / std::max<uint64_t>(1, p.n_tiles);
    p.dims_per_group = std::min<uint64_t>(d, std::max<uint64_t>(1, std::min(by_bytes, by_blocks)));
    p.n_groups = (d + p.dims_per_group - 1) / p.dims_per_group;
    const uint64_t g = p.dims_per_group;
    p.o_med = 0;
    p.o_q = up16(p.o_med + d * 8);
    p.o_os = up16(p.o_q + 2 * d * 8);
    p.o_hist = up16(p.o_os + 8 * g * 8);                                 // 8 flags (u32) first, then the histograms
    p.o_cnt = up16(p.o_hist + 32 + g * 8 * 256 * 4);
    p.o_img0 = up16(p.o_cnt + g * 256 * p.n_tiles * 4);
    p.o_img1 = up16(p.o_img0 + g * p.S * 8);
    p.o_slab = up16(p.o_img1 + g * p.S * 8);
    p.bytes = p.o_slab + (slab ? g * p.S * 8 : 0);
    return p;
}

namespace {

// what the kernels need of the plan: retained row r is row t = r + (r >= h ? shift : 0) of the slab (not split: h = rows, shift = 0)
struct Geom {
    uint64_t d, C;
    uint32_t S, h, shift, n_tiles;
};

Geom geom_of(const RankPlan& p)
{
    Geom g;
    g.d = p.d; g.C = p.C; g.S = (uint32_t)p.S; g.n_tiles = (uint32_t)p.n_tiles;
    if (p.flags & RANK_SPLIT) { g.h = (uint32_t)p.h; g.shift = (uint32_t)(p.n_keep - 2 * p.h); }
    else { g.h = (uint32_t)p.rows; g.shift = 0; }
    return g;
}

__device__ __forceinline__ uint64_t row_of(const Geom& g, uint32_t r) { return (uint64_t)r + (r >= g.h ? g.shift : 0u); }

// one bin per lane (-1: none) into LDS counts, all lanes of the wave arrive: up to four times the wave takes the bin of its first uncounted lane,
// ballots the lanes that agree and lets one lane add the popcount; what is left is spread out, and those lanes add 1 each
__device__ __forceinline__ void wave_add(uint32_t* cnt, int bin, uint32_t lane)
{
    uint64_t rest = __ballot(bin >= 0);
    for (int it = 0; it < 4 && rest; ++it) {
        const int leader = __ffsll((unsigned long long)rest) - 1;
        const int b = __builtin_amdgcn_readlane(bin, leader);
        const uint64_t m = __ballot(bin == b);
        if ((int)lane == leader) atomicAdd(&cnt[b], (uint32_t)__popcll(m));
        rest &= ~m;
    }
    if ((rest >> lane) & 1) atomicAdd(&cnt[bin], 1u);
}

template <bool FOLD>
__global__ __launch_bounds__(256) void rank_keys_kernel(const double* __restrict__ x, Geom g, uint64_t dim0, const double* __restrict__ med,
                                                        uint64_t* __restrict__ img, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t cnt[8 * 256];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t dl = blockIdx.x / g.n_tiles, tile = blockIdx.x % g.n_tiles;
    const uint64_t i = dim0 + dl;
    for (uint32_t k = tid; k < 8 * 256; k += 256) cnt[k] = 0;
    __syncthreads();
    const double m = FOLD ? med[i] : 0.0;
    const uint32_t s0 = tile * RANK_TILE;
    const uint32_t s1 = (g.S - s0 < RANK_TILE) ? g.S : s0 + RANK_TILE;
    uint64_t* __restrict__ dst = img + (uint64_t)dl * g.S;
    // all lanes of the wave arrive
    auto emit = [&](uint32_t s, double xv, bool ok) __attribute__((always_inline)) {
        const double v = FOLD ? __builtin_fabs(xv - m) : xv;
        const uint64_t key = sel_key(v);
        if (ok) dst[s] = key;
#pragma unroll
        for (int p = 0; p < 8; ++p) wave_add(cnt, ok ? (int)(p * 256 + ((uint32_t)(key >> (8 * p)) & 255u)) : -1, lane);
    };
    const uint32_t C32 = (uint32_t)g.C;
    if (C32 < RANK_SMALL_C) {                            // short rows, flattened: key s is (row s / C, chain s % C)
        for (uint32_t base = s0; base < s1; base += 256) {
            const uint32_t s = base + tid;
            const bool ok = s < s1;
            const uint32_t r = ok ? s / C32 : 0u, c = ok ? s - r * C32 : 0u;
            const double xv = ok ? x[(row_of(g, r) * g.d + i) * g.C + c] : 0.0;
            emit(s, xv, ok);
        }
    } else {
        for (uint32_t r = s0 / C32; (uint64_t)r * C32 < s1; ++r) {
            const uint64_t rs = (uint64_t)r * C32;       // the first key of the row
            const uint32_t c0 = rs < s0 ? (uint32_t)(s0 - rs) : 0u;
            const uint32_t c1 = rs + C32 > s1 ? (uint32_t)(s1 - rs) : C32;
            const uint32_t n = c1 - c0, sb = (uint32_t)(rs + c0);
            const double* p = x + (row_of(g, r) * g.d + i) * g.C + c0;
            const uint32_t head = (n && ((uintptr_t)p & 8)) ? 1u : 0u;
            const uint32_t body = (n - head) / 2, tail = n - head - 2 * body;
            const double2_t* p2 = reinterpret_cast<const double2_t*>(p + head);
            for (uint32_t base = 0; base < body; base += 256) {
                const uint32_t e = base + tid;
                const bool ok = e < body;
                const double2_t v2 = ok ? p2[e] : double2_t{0.0, 0.0};
                emit(sb + head + 2 * e, v2.x, ok);
                emit(sb + head + 2 * e + 1, v2.y, ok);
            }
            if (wave == 0 && (head | tail)) {            // lane 0: the head, lane 1: the tail
                const bool ok = (lane == 0 && head) || (lane == 1 && tail);
                const uint32_t off = lane == 0 ? 0u : n - 1;
                emit(sb + off, ok ? p[off] : 0.0, ok);
            }
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < 8 * 256; k += 256) {
        const uint32_t c = cnt[k];
        if (c) atomicAdd(&hist[(uint64_t)dl * 2048 + k], c);
    }
}

// flags[p] |= 1 where digit p takes more than one value among the S keys of a dimension: a bin that is neither empty nor all of them
__global__ __launch_bounds__(256) void rank_const_kernel(const uint32_t* __restrict__ hist, uint32_t S, uint32_t* __restrict__ flags)
{
    const uint32_t* h = hist + (uint64_t)blockIdx.x * 2048;
    for (uint32_t p = 0; p < 8; ++p) {
        const uint32_t c = h[p * 256 + threadIdx.x];
        if (c != 0 && c != S) atomicOr(&flags[p], 1u);
    }
}

__global__ __launch_bounds__(256) void rank_count_kernel(const uint64_t* __restrict__ src, uint32_t S, uint32_t n_tiles, uint32_t sh, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t cnt[256];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t dl = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    cnt[tid] = 0;
    __syncthreads();
    const uint32_t s0 = tile * RANK_TILE;
    const uint32_t s1 = (S - s0 < RANK_TILE) ? S : s0 + RANK_TILE;
    const uint64_t* __restrict__ k = src + (uint64_t)dl * S;
    for (uint32_t base = s0; base < s1; base += 256) {
        const uint32_t s = base + tid;
        const bool ok = s < s1;
        const uint64_t key = ok ? k[s] : 0ull;
        wave_add(cnt, ok ? (int)((uint32_t)(key >> sh) & 255u) : -1, lane);
    }
    __syncthreads();
    counts[((uint64_t)dl * 256 + tid) * n_tiles + tile] = cnt[tid];
}

// exclusive prefix sum of a dimension's N = 256 n_tiles counts (digit-major, tile-minor), in place: thread j owns the entries [j per, (j + 1) per)
__global__ __launch_bounds__(256) void rank_scan_kernel(uint32_t n_tiles, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t part[256];
    const uint32_t tid = threadIdx.x;
    uint32_t* __restrict__ c = counts + (uint64_t)blockIdx.x * 256 * n_tiles;
    const uint32_t N = 256 * n_tiles, per = n_tiles;     // N / 256
    const uint32_t lo = tid * per, hi = lo + per;
    uint32_t s = 0;
    for (uint32_t k = lo; k < hi; ++k) s += c[k];
    part[tid] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {       // inclusive, Hillis-Steele
        const uint32_t v = tid >= off ? part[tid - off] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - s;
    for (uint32_t k = lo; k < hi && k < N; ++k) { const uint32_t v = c[k]; c[k] = run; run += v; }
}

__global__ __launch_bounds__(256) void rank_scatter_kernel(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, uint32_t S, uint32_t n_tiles, uint32_t sh,
                                                           const uint32_t* __restrict__ offs)
{
    __shared__ uint32_t wcnt[4 * 256];                   // [wave][digit]: first the wave's counts, then its running offsets
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t dl = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    for (uint32_t k = tid; k < 4 * 256; k += 256) wcnt[k] = 0;
    __syncthreads();
    const uint32_t s0 = tile * RANK_TILE;
    const uint32_t s1 = (S - s0 < RANK_TILE) ? S : s0 + RANK_TILE;
    const uint32_t w0 = s0 + wave * (RANK_TILE / 4);     // the wave's quarter, in element order
    const uint32_t w1 = (s1 - s0 < (wave + 1) * (RANK_TILE / 4)) ? s1 : w0 + RANK_TILE / 4;
    const uint64_t* __restrict__ k = src + (uint64_t)dl * S;
    uint64_t* __restrict__ o = dst + (uint64_t)dl * S;
    uint32_t* mine = wcnt + wave * 256;
    for (uint32_t base = w0; base < w1; base += 64) {
        const uint32_t s = base + lane;
        const bool ok = s < w1;
        const uint64_t key = ok ? k[s] : 0ull;
        wave_add(mine, ok ? (int)((uint32_t)(key >> sh) & 255u) : -1, lane);
    }
    __syncthreads();
    {
        uint32_t run = offs[((uint64_t)dl * 256 + tid) * n_tiles + tile];
#pragma unroll
        for (int w = 0; w < 4; ++w) { const uint32_t c = wcnt[w * 256 + tid]; wcnt[w * 256 + tid] = run; run += c; }
    }
    __syncthreads();
    volatile uint32_t* run_of = mine;                    // only this wave touches its 256 offsets: LDS serves a wave's accesses in order
    const uint64_t below = (1ull << lane) - 1;
    for (uint32_t base = w0; base < w1; base += 64) {
        const uint32_t s = base + lane;
        const bool ok = s < w1;
        const uint64_t key = ok ? k[s] : 0ull;
        const uint32_t dg = (uint32_t)(key >> sh) & 255u;
        uint64_t peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (dg >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t at = ok ? run_of[dg] : 0u;
        const uint32_t pos = at + (uint32_t)__popcll(peers & below);
        if (ok && pos < S) o[pos] = key;                 // (pos < S holds by construction: the counts are those of these very keys)
        if (ok && (peers & below) == 0) run_of[dg] = at + (uint32_t)__popcll(peers);
    }
}

// lo = the number of sorted keys below `key`, in two levels: the samples in LDS, then one window of the image
__device__ __forceinline__ uint32_t rank_below(const uint64_t* __restrict__ srt, const uint64_t* smp, uint32_t S, uint32_t stride, uint32_t n_samples, uint64_t key)
{
    uint32_t a = 0, b = n_samples;                       // the samples srt[j stride] before a are below key, those from b on are not
    while (a < b) {
        const uint32_t mid = (a + b) >> 1;
        if (smp[mid] < key) a = mid + 1; else b = mid;
    }
    uint32_t lo = a ? (a - 1) * stride + 1 : 0u;         // srt[(a - 1) stride] is below key, srt[a stride] (or the end) is not
    uint32_t hi = a < n_samples ? a * stride : S;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (srt[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// hi = the number of sorted keys not above `key`, galloping up from lo: two probes where the key is unique (draws of a continuous target), and
// 2 log2 of the number of its ties otherwise
__device__ __forceinline__ uint32_t rank_not_above(const uint64_t* __restrict__ srt, uint32_t S, uint32_t lo, uint64_t key)
{
    uint32_t a = lo, b = lo, step = 1;                   // the keys before a are not above key; srt[b] is above it, or b is the end
    while (b < S && srt[b] <= key) {
        a = b + 1;
        b = (S - b > step) ? b + step : S;
        step <<= 1;
    }
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (srt[mid] <= key) a = mid + 1; else b = mid;
    }
    return a;
}

// where retained sample (r, c) of local dimension od goes: split puts the second halves at columns C ...
__device__ __forceinline__ uint64_t out_index(const Geom& g, uint32_t r, uint32_t c, uint64_t out_d, uint64_t od, uint32_t split)
{
    if (!split) return ((uint64_t)r * out_d + od) * g.C + c;
    const bool second = r >= g.h;
    return ((uint64_t)(second ? r - g.h : r) * out_d + od) * (2 * g.C) + (second ? g.C : 0) + c;
}

template <int WHAT, bool FOLD>
__global__ __launch_bounds__(256) void rank_lookup_kernel(const double* __restrict__ x, Geom g, uint64_t dim0, const double* __restrict__ med,
                                                          const uint64_t* __restrict__ sorted, uint32_t stride, uint32_t n_samples, uint32_t split,
                                                          double* __restrict__ out, uint64_t out_d, uint64_t out_dim0)
{
    extern __shared__ uint64_t smp[];                    // every stride-th sorted key of the dimension
    const uint32_t tid = threadIdx.x;
    const uint32_t dl = blockIdx.x / g.n_tiles, chunk = blockIdx.x % g.n_tiles;
    const uint64_t i = dim0 + dl;
    const uint64_t* __restrict__ srt = sorted + (uint64_t)dl * g.S;
    for (uint32_t j = tid; j < n_samples; j += 256) smp[j] = srt[(uint64_t)j * stride];
    __syncthreads();
    const double m = FOLD ? med[i] : 0.0;
    const uint32_t C32 = (uint32_t)g.C;
    const uint32_t s0 = chunk * RANK_LOOKUP_ELEMS;
    const uint32_t s1 = (g.S - s0 < RANK_LOOKUP_ELEMS) ? g.S : s0 + RANK_LOOKUP_ELEMS;
    const double denom = (double)g.S + 0.25;
    for (uint32_t s = s0 + tid; s < s1; s += 256) {
        const uint32_t r = s / C32, c = s - r * C32;
        const double xv = x[(row_of(g, r) * g.d + i) * g.C + c];
        const double v = FOLD ? __builtin_fabs(xv - m) : xv;
        const uint64_t key = sel_key(v);
        const uint32_t lo = rank_below(srt, smp, g.S, stride, n_samples, key);
        const uint32_t hi = rank_not_above(srt, g.S, lo, key);
        const uint64_t R2 = (uint64_t)lo + (uint64_t)hi + 1;
        const double avg = 0.5 * (double)R2;
        double res;
        if (key == ~0ull) res = __longlong_as_double(0x7FF8000000000000ll);
        else if (WHAT == RANK_AVERAGE) res = avg;
        else res = norm_ppf((avg - 0.375) / denom);
        out[out_index(g, r, c, out_d, out_dim0 + dl, split)] = res;
    }
}

struct OsRanks { uint64_t r[8]; };

__global__ __launch_bounds__(256) void rank_os_kernel(const uint64_t* __restrict__ sorted, uint32_t S, uint32_t nd, OsRanks ranks, double* __restrict__ os)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 8 * nd) return;
    const uint32_t a = e / nd, dl = e % nd;
    const uint64_t rk = ranks.r[a] < S ? ranks.r[a] : S - 1;
    os[e] = sel_unkey(sorted[(uint64_t)dl * S + rk]);
}

__global__ __launch_bounds__(256) void rank_indicator_kernel(const double* __restrict__ x, Geom g, uint64_t dim0, const double* __restrict__ q, uint32_t split,
                                                             double* __restrict__ out, uint64_t out_d)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t dl = blockIdx.x / g.n_tiles, chunk = blockIdx.x % g.n_tiles;
    const uint64_t i = dim0 + dl;
    const double qi = q[i];
    const uint32_t C32 = (uint32_t)g.C;
    const uint32_t s0 = chunk * RANK_LOOKUP_ELEMS;
    const uint32_t s1 = (g.S - s0 < RANK_LOOKUP_ELEMS) ? g.S : s0 + RANK_LOOKUP_ELEMS;
    for (uint32_t s = s0 + tid; s < s1; s += 256) {
        const uint32_t r = s / C32, c = s - r * C32;
        const double xv = x[(row_of(g, r) * g.d + i) * g.C + c];
        out[out_index(g, r, c, out_d, dl, split)] = xv != xv ? __longlong_as_double(0x7FF8000000000000ll) : (xv <= qi ? 1.0 : 0.0);
    }
}

}  // namespace

static_assert(RANK_LOOKUP_ELEMS == RANK_TILE, "the lookup and the indicator number their workgroups by n_tiles");

int rank_sort_group(const double* x, const RankPlan& p, uint64_t dim0, uint64_t nd, bool fold, void* ws, hipStream_t st, const uint64_t** sorted)
{
    char* W = static_cast<char*>(ws);
    const Geom g = geom_of(p);
    const double* med = reinterpret_cast<const double*>(W + p.o_med);
    uint32_t* flags = reinterpret_cast<uint32_t*>(W + p.o_hist);
    uint32_t* hist = flags + 8;
    uint32_t* counts = reinterpret_cast<uint32_t*>(W + p.o_cnt);
    uint64_t* img[2] = {reinterpret_cast<uint64_t*>(W + p.o_img0), reinterpret_cast<uint64_t*>(W + p.o_img1)};
    const dim3 grid((unsigned)(nd * p.n_tiles)), b(256);
    hipError_t e = hipMemsetAsync(flags, 0, 32 + (size_t)nd * 2048 * 4, st);
    if (e != hipSuccess) return (int)e;
    if (fold) hipLaunchKernelGGL(rank_keys_kernel<true>, grid, b, 0, st, x, g, dim0, med, img[0], hist);
    else hipLaunchKernelGGL(rank_keys_kernel<false>, grid, b, 0, st, x, g, dim0, med, img[0], hist);
    hipLaunchKernelGGL(rank_const_kernel, dim3((unsigned)nd), b, 0, st, hist, g.S, flags);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    uint32_t varies[8];
    if ((e = hipMemcpyAsync(varies, flags, 32, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e;
    int cur = 0;
    for (uint32_t pass = 0; pass < 8; ++pass) {
        if (!varies[pass]) continue;                     // one digit value in every dimension of the group: the pass would be the identity
        hipLaunchKernelGGL(rank_count_kernel, grid, b, 0, st, img[cur], g.S, g.n_tiles, 8 * pass, counts);
        hipLaunchKernelGGL(rank_scan_kernel, dim3((unsigned)nd), b, 0, st, g.n_tiles, counts);
        hipLaunchKernelGGL(rank_scatter_kernel, grid, b, 0, st, img[cur], img[cur ^ 1], g.S, g.n_tiles, 8 * pass, counts);
        cur ^= 1;
        g_passes.fetch_add(1, std::memory_order_relaxed);
    }
    g_sorts.fetch_add(1, std::memory_order_relaxed);
    *sorted = img[cur];
    return (int)hipGetLastError();
}

int rank_lookup_group(const double* x, const RankPlan& p, uint64_t dim0, uint64_t nd, bool fold, int what, const uint64_t* sorted, void* ws, double* out,
                      uint64_t out_d, uint64_t out_dim0, hipStream_t st)
{
    const Geom g = geom_of(p);
    const double* med = reinterpret_cast<const double*>(static_cast<char*>(ws) + p.o_med);
    const dim3 grid((unsigned)(nd * p.n_tiles)), b(256);
    const size_t lds = (size_t)p.n_samples * 8;
    const uint32_t split = (p.flags & RANK_SPLIT) ? 1u : 0u;
#define MI_RANK_LOOKUP(W_, F_) hipLaunchKernelGGL((rank_lookup_kernel<W_, F_>), grid, b, lds, st, x, g, dim0, med, sorted, p.stride, p.n_samples, split, out, out_d, out_dim0)
    if (what == RANK_AVERAGE) { if (fold) MI_RANK_LOOKUP(RANK_AVERAGE, true); else MI_RANK_LOOKUP(RANK_AVERAGE, false); }
    else { if (fold) MI_RANK_LOOKUP(RANK_NORMAL, true); else MI_RANK_LOOKUP(RANK_NORMAL, false); }
#undef MI_RANK_LOOKUP
    return (int)hipGetLastError();
}

int rank_order_stats_group(const RankPlan& p, uint64_t nd, const uint64_t* sorted, const uint64_t ranks[8], void* ws, double* os_host, hipStream_t st)
{
    double* os = reinterpret_cast<double*>(static_cast<char*>(ws) + p.o_os);
    OsRanks r;
    for (int a = 0; a < 8; ++a) r.r[a] = ranks[a];
    hipLaunchKernelGGL(rank_os_kernel, dim3((unsigned)((8 * nd + 255) / 256)), dim3(256), 0, st, sorted, (uint32_t)p.S, (uint32_t)nd, r, os);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if ((e = hipMemcpyAsync(os_host, os, 8 * nd * 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
    return (int)hipStreamSynchronize(st);
}

int rank_indicator_group(const double* x, const RankPlan& p, uint64_t dim0, uint64_t nd, int which, void* ws, double* out, hipStream_t st)
{
    const Geom g = geom_of(p);
    const double* q = reinterpret_cast<const double*>(static_cast<char*>(ws) + p.o_q) + (size_t)which * p.d;
    const uint32_t split = (p.flags & RANK_SPLIT) ? 1u : 0u;
    hipLaunchKernelGGL(rank_indicator_kernel, dim3((unsigned)(nd * p.n_tiles)), dim3(256), 0, st, x, g, dim0, q, split, out, nd);
    return (int)hipGetLastError();
}

}  // namespace drank
}  // namespace mi
