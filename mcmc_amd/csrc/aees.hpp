// aees.hpp -- mcmc::aees (src/aees.cpp:28-305, include/mcmc/aees.ipp:30-70) for many independent runs at once.
//
// A run is one call of mcmc::aees: K temperature levels swept in order at every draw (the reference with omp_n_threads = 1).  The
// contract -- the steps, the four quirks of the reference that are reproduced, the random numbers -- is written in include/mi_mcmc.h
// above mi_aees_settings.  One workgroup runs one run at a time on literal.hpp's target_eval / box_log_kernel (every kind it knows,
// MI_TARGET_GAUSS_MIXTURE, and LIT_CALLBACK, the host-callback mailbox), and walks over runs (blockIdx.x, += gridDim.x).
//
// The history.  The reference stores every state of every level (draw_storage) and, at every equi-energy step, sorts the whole window
// of level k-1's T = 1 log kernels from draw (k-1) S to the current one, to read 2 n_rings - 1 order statistics and one rank.  Here a
// workgroup owns one history slot in HBM (AeesLayout), reused by every run it serves:
//   states   level j <= K-2: draws 0 .. n_total - j S - 1 (level j+1 reads at most draw n - j S: quirk 2), d doubles each;
//   kv       level j in 1 .. K-2: the T = 1 log kernels of window positions 0 .. n_total - j S - 1 (position p = draw j S + p);
//            level 0's row is never written by the reference (quirk 1), so level 1 needs no index: rank r IS position r;
//   index    level k >= 2 over level k-1's window: sorted (key, position) pairs, ping-pong.  It is brought up to date LAZILY, at the
//            level's next equi-energy step: the values appended since the last one are rank-sorted in LDS (256 at a time, ties by
//            position), then every old element finds its place by a binary search over the new ones (# new < key) and every new
//            element by a binary search over the old ones (# old <= key: new positions are larger, so they go after equal old
//            keys), and both scatter into the other buffer.  O(window) per step and no full re-sort, ever.
// key(v): the IEEE bits made monotone (-0 mapped to +0, every NaN to the largest key): the order pinned by quirk 4.
//
// Every level caches the log kernel of its current state (the target is deterministic): the reference's re-evaluations of v(X_prev)
// (aees.ipp:47) and of kernel_vals (aees.cpp:260) give the same bits, so they are read from the cache.
#pragma once

#include "literal.hpp"

namespace mi {

constexpr uint32_t AEES_CHUNK = 256;          // new window values sorted per pass (one per thread)

struct AeesParams {
    lit::LitParams lit;          // the target (lit.t), the bounds (vals_bound / btype / lb / ub), the per-workgroup scratch (work)
    uint32_t d, K, n_rings;
    uint32_t S, n_keep, n_total; // S = n_initial_draws + n_burnin_draws, n_total = n_keep + K S
    uint64_t P;                  // runs of the call (the column stride of every output)
    uint64_t r_begin, r_end;     // local runs [r_begin, r_end) in this launch
    uint64_t run0;               // global id of local run 0
    uint64_t seed;
    double ee_prob;
    const double* temp;          // [K] descending, temp[K-1] = 1
    const double* At;            // [K][d][d]: At[(k d + c) d + i] = sqrt(T_k) * (par_scale * CHOL_LOWER(cov)[i][c])
    const double* init;          // [d][P]
    double* draws;               // [n_keep][d][P] or nullptr
    double* fin;                 // [K][d][P] or nullptr
    uint64_t* n_acc;             // [K][P] or nullptr
    uint64_t* n_ee;              // [K][P] or nullptr
    char* hist;                  // history slots, hist_stride bytes each (one per workgroup)
    size_t hist_stride;
    size_t lit_stride;           // doubles of literal.hpp scratch at the start of a workgroup's work area
};

// entries of level j's history (states, kv): draws 0 .. n_total - j S - 1
MI_HD uint64_t aees_len(uint32_t n_total, uint32_t S, uint32_t j) { return (uint64_t)n_total - (uint64_t)j * S; }

// byte offsets inside a history slot
struct AeesLayout {
    size_t states_bytes, kv_bytes, index_bytes;
};
MI_HD AeesLayout aees_layout(uint32_t d, uint32_t K, uint32_t S, uint32_t n_total)
{
    AeesLayout L{0, 0, 0};
    for (uint32_t j = 0; j + 2 <= K; ++j) L.states_bytes += aees_len(n_total, S, j) * d * 8;
    for (uint32_t j = 1; j + 2 <= K; ++j) L.kv_bytes += aees_len(n_total, S, j) * 8;
    for (uint32_t k = 2; k < K; ++k) L.index_bytes += aees_len(n_total, S, k - 1) * 24;       // 2 x (u64 key + u32 position)
    return L;
}
MI_HD size_t aees_slot_bytes(uint32_t d, uint32_t K, uint32_t S, uint32_t n_total)
{
    const AeesLayout L = aees_layout(d, K, S, n_total);
    return (L.states_bytes + L.kv_bytes + L.index_bytes + 255) & ~(size_t)255;
}
MI_HD double* aees_states(const AeesParams& p, char* slot, uint32_t j)
{
    size_t off = 0;
    for (uint32_t i = 0; i < j; ++i) off += aees_len(p.n_total, p.S, i) * p.d * 8;
    return reinterpret_cast<double*>(slot + off);
}
MI_HD double* aees_kv(const AeesParams& p, char* slot, uint32_t j)
{
    size_t off = aees_layout(p.d, p.K, p.S, p.n_total).states_bytes;
    for (uint32_t i = 1; i < j; ++i) off += aees_len(p.n_total, p.S, i) * 8;
    return reinterpret_cast<double*>(slot + off);
}
// level k's index (k >= 2) over level k-1's window of w = aees_len(k-1) entries: keys[2][w], then positions[2][w]
MI_HD char* aees_index(const AeesParams& p, char* slot, uint32_t k)
{
    const AeesLayout L = aees_layout(p.d, p.K, p.S, p.n_total);
    size_t off = L.states_bytes + L.kv_bytes;
    for (uint32_t i = 2; i < k; ++i) off += aees_len(p.n_total, p.S, i - 1) * 24;
    return slot + off;
}
// work doubles per workgroup: literal.hpp's scratch, the K current states, 8 K per-level scalars
MI_HD size_t aees_work_doubles(size_t lit_stride, uint32_t d, uint32_t K) { return lit_stride + (size_t)K * ((size_t)d + 8) + 8 * (size_t)K + 8; }

// the total order of quirk 4 as an unsigned key
MI_HD uint64_t aees_key(double v)
{
    if (v != v) return ~0ull;
    const uint64_t b = (v == 0.0) ? 0ull : d2u(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

// rnorm_vec on the aees normal stream: dimension i = 8b + 4h + j takes component h of Philox slot 4b + j (literal.hpp: normal_vec)
MI_HD void aees_normals(const lit::Par& par, uint64_t seed, uint64_t chain, uint32_t n, uint32_t d, double* z)
{
    const uint32_t n_slots = (d + 7) / 8 * 4;
    LIT_PFOR(s, n_slots) {
        double z0, z1;
        rng_normal_pair(seed, chain, n, s, STREAM_AEES_NORMAL, z0, z1);
        const uint32_t i0 = 8 * (s / 4) + (s % 4), i1 = i0 + 4;
        if (i0 < d) z[i0] = z0;
        if (i1 < d) z[i1] = z1;
    }
    par.sync();
}

// std::min(0.01, x): x when x < 0.01, else (NaN included) 0.01
MI_HD double aees_comp(double x) { return (x < 0.01) ? x : 0.01; }

#if defined(__HIPCC__) && !defined(MI_AEES_PARAMS_ONLY)
// Brings level k's index (k >= 2) over level k-1's window up to m entries; *len: the entries merged so far, *ping: the live buffer.
// Returns (through the same) the new length and buffer.  lk / lp / sk / sp: LDS, AEES_CHUNK entries each.
__device__ void aees_merge(const lit::Par& par, const AeesParams& p, char* slot, uint32_t k, uint32_t m, uint32_t& len, uint32_t& ping,
                           uint64_t* lk, uint32_t* lpos, uint64_t* sk, uint32_t* sp)
{
    const uint64_t w = aees_len(p.n_total, p.S, k - 1);
    char* base = aees_index(p, slot, k);
    uint64_t* keys = reinterpret_cast<uint64_t*>(base);                 // keys[b * w + i]
    uint32_t* pos = reinterpret_cast<uint32_t*>(base + 16 * w);         // pos[b * w + i]
    const double* kv = (k - 1 >= 1) ? aees_kv(p, slot, k - 1) : nullptr;
    while (len < m) {
        const uint32_t a = (m - len < AEES_CHUNK) ? m - len : AEES_CHUNK;
        const uint32_t t = (uint32_t)par.tid;
        if (t < a) { lk[t] = aees_key(kv[len + t]); lpos[t] = len + t; }
        __syncthreads();
        if (t < a) {                                                    // rank sort, ties by position (stable)
            const uint64_t kt = lk[t];
            uint32_t r = 0;
            for (uint32_t u = 0; u < a; ++u) { const uint64_t ku = lk[u]; r += (ku < kt || (ku == kt && u < t)) ? 1u : 0u; }
            sk[r] = kt; sp[r] = lpos[t];
        }
        __syncthreads();
        const uint64_t* ok = keys + (size_t)ping * w;
        const uint32_t* op = pos + (size_t)ping * w;
        uint64_t* nk = keys + (size_t)(ping ^ 1u) * w;
        uint32_t* np = pos + (size_t)(ping ^ 1u) * w;
        LIT_PFOR(i, len) {                                              // old element i: after every new key strictly below it
            const uint64_t key = ok[i];
            uint32_t lo = 0, hi = a;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sk[mid] < key) lo = mid + 1; else hi = mid; }
            nk[i + lo] = key; np[i + lo] = op[i];
        }
        if (t < a) {                                                    // new element t: after every old key <= it
            const uint64_t key = sk[t];
            uint32_t lo = 0, hi = len;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (ok[mid] <= key) lo = mid + 1; else hi = mid; }
            nk[t + lo] = key; np[t + lo] = sp[t];
        }
        __syncthreads();
        len += a;
        ping ^= 1u;
    }
}

// one run on the workgroup; slot: its history, wk: its work area
__device__ void aees_run(const lit::Par& par, const AeesParams& p, uint64_t pl, char* slot, double* wk,
                         uint64_t* lk, uint32_t* lpos, uint64_t* sk, uint32_t* sp, int* s_ring)
{
    const lit::LitParams& lp = p.lit;
    const uint32_t d = p.d, K = p.K, S = p.S;
    const uint64_t run = p.run0 + pl;
    const lit::Vecs v = lit::carve(wk, d, lp.t.n_rows, false);
    double* X = wk + p.lit_stride;                                      // [K][d + 8]: the current states
    double* sc = X + (size_t)K * (d + 8);                               // per-level scalars, K each:
    double* cache = sc;                                                 //   the log kernel of the current state
    double* kvp0 = sc + K;                                              //   kernel_vals_new(0, k), (1, k) of the reference
    double* kvp1 = sc + 2 * K;
    double* kvlast = sc + 3 * K;                                        //   kernel_vals(k, n - 1)
    double* ilen = sc + 4 * K;                                          //   entries merged into level k's index
    double* iping = sc + 5 * K;                                         //   its live buffer
    double* nacc = sc + 6 * K;
    double* nee = sc + 7 * K;
    auto Xk = [&](uint32_t k) { return X + (size_t)k * (d + 8); };
    auto xrow = [&](uint32_t k, uint32_t i) -> double& { return Xk(k)[i]; };

    // the first state (transformed when bounded, aees.cpp:125-129); the other levels start at the zero vector
    LIT_PFOR(i, d) {
        const double x = p.init[(size_t)i * p.P + pl];
        xrow(0, i) = lp.vals_bound ? lit::lit_transform(x, lp.btype[i], lp.lb[i], lp.ub[i]) : x;
        for (uint32_t k = 1; k < K; ++k) xrow(k, i) = 0.0;
        v.cur[i] = xrow(0, i);
    }
    par.sync();
    const double v0 = lit::box_log_kernel(par, lp, v, v.cur);
    double vz = 0.0;
    if (K > 1) {
        LIT_PFOR(i, d) v.cur[i] = 0.0;
        par.sync();
        vz = lit::box_log_kernel(par, lp, v, v.cur);
    }
    if (par.tid == 0)
        for (uint32_t k = 0; k < K; ++k) {
            cache[k] = (k == 0) ? v0 : vz;
            kvp0[k] = kvp1[k] = kvlast[k] = ilen[k] = iping[k] = nacc[k] = nee[k] = 0.0;
        }
    par.sync();

    // one MH step of level k at draw n (aees.ipp:30-70); returns the accepted flag, the state and cache updated
    auto mh = [&](uint32_t k, uint32_t n, double u) -> bool {
        const double T = p.temp[k];
        const double vprev = cache[k];
        aees_normals(par, p.seed, run * K + k, n, d, v.z);
        const double* A = p.At + (size_t)k * d * d;
        LIT_PFOR(i, d) {
            double acc = 0.0;
            for (uint32_t c = 0; c < d; ++c) acc = dfma(A[(size_t)c * d + i], v.z[c], acc);
            v.cur[i] = xrow(k, i) + acc;
        }
        par.sync();
        const double vnew = lit::box_log_kernel(par, lp, v, v.cur);
        const double comp = aees_comp((vnew - vprev) / T);
        const bool acc = u < det_exp(comp);
        if (acc) { LIT_PFOR(i, d) xrow(k, i) = v.cur[i]; }
        par.sync();
        if (acc && par.tid == 0) { cache[k] = vnew; nacc[k] = nacc[k] + 1.0; }
        par.sync();
        return acc;
    };

    for (uint32_t n = 0; n < p.n_total; ++n) {
        for (uint32_t k = 0; k < K; ++k) {
            const bool active = (k == 0) || ((uint64_t)n > (uint64_t)k * S);
            if (active) {
                const u32x4 w0 = rng_block(p.seed, run * K + k, n, 0u, STREAM_AEES);
                const double z_eps = u01(w0.x, w0.y), u = u01(w0.z, w0.w);
                if (k == 0) {
                    (void)mh(0, n, u);
                } else if (z_eps > p.ee_prob) {
                    (void)mh(k, n, u);
                    const double c = cache[k];
                    par.sync();
                    if (par.tid == 0) { kvp0[k] = c / p.temp[k - 1]; kvp1[k] = c / p.temp[k]; }
                    par.sync();
                } else {                                                // the equi-energy step (aees.cpp:206-257)
                    const uint32_t begin = (k - 1) * S;
                    const uint32_t m = n - begin + 1;
                    const uint32_t s = m / p.n_rings;
                    if (s != 0) {
                        const double kl = kvlast[k];
                        uint32_t len = (uint32_t)ilen[k], ping = (uint32_t)iping[k];
                        const double* kvw = (k >= 2) ? aees_kv(p, slot, k - 1) : nullptr;
                        const uint32_t* pw = nullptr;
                        if (k >= 2) {
                            aees_merge(par, p, slot, k, m, len, ping, lk, lpos, sk, sp);
                            const uint64_t wl = aees_len(p.n_total, S, k - 1);
                            pw = reinterpret_cast<const uint32_t*>(aees_index(p, slot, k) + 16 * wl) + (size_t)ping * wl;
                        }
                        // which_ring: the leading ring bounds below kv(k, n-1); level 1's bounds are all 0 (quirk 1)
                        if (par.tid == 0) *s_ring = (int)(p.n_rings - 1);
                        par.sync();
                        LIT_PFOR(i, p.n_rings - 1) {
                            const uint32_t q = (i + 1) * s;
                            const double b = (k >= 2) ? (kvw[pw[q]] + kvw[pw[q - 1]]) / 2.0 : (0.0 + 0.0) / 2.0;
                            if (!(kl > b)) atomicMin(s_ring, (int)i);
                        }
                        par.sync();
                        const uint32_t which_ring = (uint32_t)*s_ring;
                        const u32x4 w1 = rng_block(p.seed, run * K + k, n, 1u, STREAM_AEES);
                        const double z_tmp = u01(w1.x, w1.y);
                        const uint32_t r = s * which_ring + (uint32_t)__builtin_floor(z_tmp * (double)s);
                        const uint32_t ind_mix = (k >= 2) ? pw[r] : r;
                        // the proposal: level k-1's state at ABSOLUTE draw ind_mix (quirk 2); draw n is not stored yet (quirk 3)
                        const double* src = (ind_mix < n) ? aees_states(p, slot, k - 1) + (size_t)ind_mix * d : nullptr;
                        LIT_PFOR(i, d) v.cur[i] = src ? src[i] : 0.0;
                        par.sync();
                        const double val = lit::box_log_kernel(par, lp, v, v.cur);
                        const double new0 = val / p.temp[k - 1], new1 = val / p.temp[k];
                        const double comp = aees_comp((new1 - kvp1[k]) + (kvp0[k] - new0));
                        const bool acc = !(u > det_exp(comp));
                        if (acc) { LIT_PFOR(i, d) xrow(k, i) = v.cur[i]; }
                        par.sync();
                        if (par.tid == 0) {
                            ilen[k] = (double)len; iping[k] = (double)ping;
                            if (acc) { cache[k] = val; kvp0[k] = new0; kvp1[k] = new1; nee[k] = nee[k] + 1.0; }
                        }
                        par.sync();
                    }
                }
            }
            // the history this level leaves for level k+1 (and kv(k, n) for its own next step)
            if (k + 2 <= K) {
                if ((uint64_t)n < aees_len(p.n_total, S, k)) {
                    double* st = aees_states(p, slot, k) + (size_t)n * d;
                    LIT_PFOR(i, d) st[i] = xrow(k, i);
                }
                if (k >= 1 && (uint64_t)n >= (uint64_t)k * S && par.tid == 0) aees_kv(p, slot, k)[n - k * S] = active ? cache[k] : 0.0;
            }
            if (k == K - 1 && (uint64_t)n >= (uint64_t)K * S && p.draws) {  // the kept draws (aees.cpp:271-283)
                const uint32_t row = n - K * S;
                LIT_PFOR(i, d) {
                    const double x = xrow(k, i);
                    p.draws[((size_t)row * d + i) * p.P + pl] = lp.vals_bound ? lit::lit_inv_transform(x, lp.btype[i], lp.lb[i], lp.ub[i]) : x;
                }
            }
            par.sync();
            if (k >= 1 && par.tid == 0) kvlast[k] = active ? cache[k] : 0.0;
            par.sync();
        }
    }
    LIT_PFOR(e, (size_t)K * d) {
        const uint32_t k = (uint32_t)(e / d), i = (uint32_t)(e % d);
        if (p.fin) p.fin[((size_t)k * d + i) * p.P + pl] = xrow(k, i);
    }
    LIT_PFOR(k, K) {
        if (p.n_acc) p.n_acc[(size_t)k * p.P + pl] = (uint64_t)nacc[k];
        if (p.n_ee) p.n_ee[(size_t)k * p.P + pl] = (uint64_t)nee[k];
    }
    par.sync();
}

__global__ __launch_bounds__(256) void aees_literal_kernel(const AeesParams prm)
{
    __shared__ uint64_t lk[AEES_CHUNK], sk[AEES_CHUNK];
    __shared__ uint32_t lpos[AEES_CHUNK], sp[AEES_CHUNK];
    __shared__ int s_ring;
    const lit::Par par{(int)threadIdx.x, (int)blockDim.x};
    char* slot = prm.hist + (size_t)blockIdx.x * prm.hist_stride;
    double* wk = prm.lit.work + (size_t)blockIdx.x * prm.lit.work_stride;
    for (uint64_t pl = prm.r_begin + blockIdx.x; pl < prm.r_end; pl += gridDim.x) {
        aees_run(par, prm, pl, slot, wk, lk, lpos, sk, sp, &s_ring);
        __syncthreads();
    }
}
#endif

}  // namespace mi
