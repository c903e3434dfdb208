// draw_stats.hip -- mi_mcmc_draw_stats and mi_mcmc_draw_stats_lags (include/mi_mcmc.h): the host ladders around the kernels of draw_stats.hpp and
// draw_stats_lags.hpp, which this translation unit alone includes, over the host side the two share (draw_stats_host.hpp: the scratch of a call, the
// centre, the addition of the chain groups, R-hat, Geyer's sum).  Both allocate a device buffer of their own, never the stream's leased workspace:
// mi_mcmc_draw_stats_ranked / _ranked_lags (draws_api.hip) call in through the C ABI while they hold that lease.  Also here: the two route probes and
// the host hook of mi_mcmc_probes.h, and mi_mcmc_draws_to_chain_major_device, whose kernel draw_stats.hpp defines.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "host_common.hpp"
#include "draw_stats.hpp"
#include "draw_stats_lags.hpp"
#include "draw_stats_host.hpp"

using namespace mi::host;       // fail, need_device, DevBuf, stage_slab (host_common.hpp)
using namespace mi::dstats;     // Slab, Scratch, row_mean, two_part_centre, group_sum, geyer_ess, rhat_from_moments (draw_stats_host.hpp)

namespace {

thread_local uint64_t draw_stats_last[8];
thread_local uint64_t lags_last[8];

// ---- mi_mcmc_draw_stats: the slab and what its three routes share.  A route fills ac (the lags it computes), mp and ess_h.
struct StatsCall : Slab {
    size_t nlag_max;                    // lags [0, nlag_max) are all a route computes
    bool acov;                          // the autocovariance itself is asked for: every lag of every dimension
    Scratch S;
    std::vector<double> a_h, e_h;       // the centre (draw_stats_host.hpp)
    std::vector<double> ac;             // ac[k * d + j]: pooled over chains, unbiased per lag
    std::vector<double> mp;             // [G][d][3] moments for R-hat
    std::vector<double> ess_h, ap;
    std::vector<uint32_t> active;       // the dimensions whose Geyer sum is still open
    size_t computed = 0;                // lags [0, computed) are known for the active dimensions

    int fetch(std::vector<double>& dst, size_t off, size_t cnt)
    {
        dst.resize(cnt);
        HIP_TRY(hipMemcpyAsync(dst.data(), S.at(off), cnt * 8, hipMemcpyDeviceToHost, st));
        return MI_OK;
    }
    // adds the G partials in ap of lags [k_lo, k_lo + cnt) of the active dimensions (stride `stride` lags per (group, dimension))
    void collect(size_t stride, size_t k_lo, size_t cnt)
    {
        const size_t nd = active.size();
        for (size_t jj = 0; jj < nd; ++jj)
            for (size_t k = 0; k < cnt && k_lo + k < nlag_max; ++k)
                ac[(k_lo + k) * d + active[jj]] = group_sum(&ap[jj * stride + k], G, nd * stride) / (double)C / (double)(n - (k_lo + k));
    }
    // keep the dimensions whose sum has not ended inside [0, computed): it ends at its first non-positive pair, or when it has run through every
    // lag there is, i.e. more lags would not change it
    void prune()
    {
        std::vector<uint32_t> next;
        for (uint32_t j : active) {
            bool hit;
            ess_h[j] = geyer_ess(ac.data(), d, j, n, computed, &hit);
            if (!(hit || n < 4 || computed >= nlag_max)) next.push_back(j);
        }
        active.swap(next);
    }
    int route_gram();
    int route_window_blocks();
    int route_streamed();
};

// n <= STATS_GRAM_MAX_N: every lag of every dimension in ONE pass over the slab, on the matrix cores (draw_stats.hpp: stats_gram_kernel).  The
// series are centred by the PROVISIONAL centre a_j alone (two_part_centre without its second pass: with e / sigma large the recentring below would
// cancel (e / sigma)^2 ulp of the autocovariances, hence the first, middle and last draw and not the first alone) and the kernel's row
// sums R_t = sum_c (x_t - a) move the centre to the pooled mean afterwards (exactly, in the algebra):  sum_c sum_t (v_t - e)(v_{t+k} - e) = S_k - e (sum_{t < n-k} R_t + sum_{t >= k} R_t) + C (n - k) e^2,
// e = pooled mean - a, which the route leaves in e_h.
int StatsCall::route_gram()
{
    int rc;
    const int nb = (int)((n + 15) / 16);
    const size_t lds = mi::stats_gram_lds_bytes(nb);
    auto launch = [&](auto kern) -> int {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)d, G), dim3(512), lds, st, x, S.at(S.o_mean), (uint32_t)n, (uint32_t)d, (uint64_t)C, G, S.at(S.o_part), S.at(S.o_mom));
        HIP_TRY(hipGetLastError());
        return MI_OK;
    };
    switch (nb) {
    case 1: rc = launch(mi::stats_gram_kernel<1>); break;
    case 2: rc = launch(mi::stats_gram_kernel<2>); break;
    case 3: rc = launch(mi::stats_gram_kernel<3>); break;
    case 4: rc = launch(mi::stats_gram_kernel<4>); break;
    case 5: rc = launch(mi::stats_gram_kernel<5>); break;
    case 6: rc = launch(mi::stats_gram_kernel<6>); break;
    case 7: rc = launch(mi::stats_gram_kernel<7>); break;
    default: rc = launch(mi::stats_gram_kernel<8>); break;
    }
    if (rc) return rc;
    const size_t nr = (size_t)16 * nb;
    if ((rc = fetch(ap, S.o_part, (size_t)G * d * 2 * nr))) return rc;
    if ((rc = fetch(mp, S.o_mom, (size_t)G * d * 3))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    // move the centre from the provisional a_j to the pooled mean (see above); groups added in order
    std::vector<double> R(n);
    for (size_t j = 0; j < d; ++j) {
        const double* const apj = &ap[j * 2 * nr];      // of group 0: [nr] lag sums, [nr] row sums
        double tot = 0.0;
        for (size_t t = 0; t < n; ++t) { R[t] = group_sum(apj + nr + t, G, d * 2 * nr); tot += R[t]; }
        const double e = tot / ((double)n * (double)C);
        double head = tot, tail = tot;                  // sum_{t < n-k} R_t and sum_{t >= k} R_t, k = 0
        for (size_t k = 0; k < n; ++k) {
            if (k > 0) { head -= R[n - k]; tail -= R[k - 1]; }
            const double cen = group_sum(apj + k, G, d * 2 * nr) - e * (head + tail) + (double)C * (double)(n - k) * e * e;
            ac[k * d + j] = cen / (double)C / (double)(n - k);
        }
        e_h[j] = e;
        // (the R-hat moments are sums over chains of the chain mean, its square and the chain variance about the provisional centre:
        //  the variance of the chain means and the within-chain variances do not depend on the centre)
    }
    computed = n;
    prune();
    return MI_OK;
}

// STATS_GRAM_MAX_N < n <= STATS_MAX_N: the lag kernels, which centre as they load, in passes over the dimensions still open
int StatsCall::route_window_blocks()
{
    int rc;
    if (!acov) {
        // ESS / R-hat only: the first 16 lags (and the moments) straight from HBM at stream speed; a dimension whose Geyer sum ends
        // inside them is done
        hipLaunchKernelGGL(mi::stats_window_kernel<16>, dim3((unsigned)d, G), dim3(64), 0, st, x, S.at(S.o_mean), (uint32_t)n, (uint32_t)d,
                           (uint64_t)C, G, S.at(S.o_part), S.at(S.o_mom));
        HIP_TRY(hipGetLastError());
        ++draw_stats_last[4];
        if ((rc = fetch(ap, S.o_part, (size_t)G * d * 16))) return rc;
        if ((rc = fetch(mp, S.o_mom, (size_t)G * d * 3))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        collect(16, 0, 16);
        computed = std::min<size_t>(16, n);
        prune();
    }
    // further lags in passes of up to STATS_PASS_BLOCKS blocks of 16, for the dimensions still open (all of them, every lag, when
    // the autocovariance itself is asked for)
    while (!active.empty() && computed < n) {
        const uint32_t b_lo = (uint32_t)(computed / mi::STATS_LB);
        const uint32_t b_all = (uint32_t)((n + mi::STATS_LB - 1) / mi::STATS_LB);
        // (ESS only: the first pass after the 16 streamed lags takes two blocks -- lags 16..47 end most sums of a sampler that mixes)
        const uint32_t b_hi = std::min<uint32_t>(b_all, b_lo + ((!acov && b_lo == 1) ? 2u : (uint32_t)mi::STATS_PASS_BLOCKS));
        const size_t npl = (size_t)(b_hi - b_lo) * mi::STATS_LB;
        const bool all_dims = active.size() == d;
        const int want_mom = (b_lo == 0) ? 1 : 0;
        if (!all_dims) HIP_TRY(hipMemcpyAsync(S.at(S.o_dims), active.data(), active.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        const size_t lds = (n * 64 + npl * 64) * sizeof(double);
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mi::stats_acov_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(mi::stats_acov_kernel, dim3((unsigned)active.size(), G), dim3(64), lds, st, x, S.at(S.o_mean), (uint32_t)n, (uint32_t)d,
                           (uint64_t)C, G, all_dims ? nullptr : S.dims(), b_lo, b_hi, want_mom, S.at(S.o_part), S.at(S.o_mom));
        HIP_TRY(hipGetLastError());
        ++draw_stats_last[5];
        if (!all_dims) {
            draw_stats_last[7] = draw_stats_last[6] ? std::min<uint64_t>(draw_stats_last[7], active.size()) : active.size();
            ++draw_stats_last[6];
        }
        if ((rc = fetch(ap, S.o_part, (size_t)G * active.size() * npl))) return rc;
        if (want_mom) { if ((rc = fetch(mp, S.o_mom, (size_t)G * d * 3))) return rc; }
        HIP_TRY(hipStreamSynchronize(st));
        collect(npl, (size_t)b_lo * mi::STATS_LB, npl);
        computed = std::min<size_t>(n, (size_t)b_hi * mi::STATS_LB);
        if (!acov) prune();
    }
    if (acov) { computed = n; prune(); }
    return MI_OK;
}

// n > STATS_MAX_N: the lags below STATS_TILED_LAGS, the series streamed through LDS in time tiles
int StatsCall::route_streamed()
{
    int rc;
    const size_t lds = (size_t)(mi::STATS_TILE_T + 2 * mi::STATS_TILED_LAGS) * 64 * sizeof(double);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mi::stats_acov_tiled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mi::stats_acov_tiled_kernel, dim3((unsigned)d, G), dim3(64), lds, st, x, S.at(S.o_mean), (uint32_t)n, (uint32_t)d,
                       (uint64_t)C, G, S.at(S.o_part), S.at(S.o_mom));
    HIP_TRY(hipGetLastError());
    if ((rc = fetch(ap, S.o_part, (size_t)G * d * nlag_max))) return rc;
    if ((rc = fetch(mp, S.o_mom, (size_t)G * d * 3))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    collect(nlag_max, 0, nlag_max);
    computed = nlag_max;
    prune();
    return MI_OK;
}

// ---- mi_mcmc_draw_stats_lags

// The band schedule, a function of ND alone (ND of (n_keep, K)): offsets [0, 8), [8, 16), then bands of 16; mcmc_amd/acov.py::band_plan is its mirror
struct Band { uint32_t lo, hi; };
std::vector<Band> band_plan(uint32_t ND)
{
    std::vector<Band> b;
    for (uint32_t lo = 0; lo < ND;) {
        const uint32_t hi = std::min<uint32_t>(ND, lo + (lo < 16 ? 8u : 16u));
        b.push_back(Band{lo, hi});
        lo = hi;
    }
    return b;
}

int lags_run(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, uint32_t max_lag, double* mean, double* acov, double* rhat,
             double* ess, uint8_t* ended, hipStream_t st)
{
    namespace L = mi::dlags;
    const size_t n = n_keep, C = n_chains;
    const size_t K = std::min<uint64_t>(max_lag, n - 1), nlag = K + 1;
    const uint32_t ND = (uint32_t)((K + 15) / 16 + 1);
    const std::vector<Band> bands = band_plan(ND);
    // chain groups: a function of (d, C); the partials of a band are G d 16 32 doubles at most
    const uint32_t G = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(64, (C + L::LAGS_TC - 1) / L::LAGS_TC), ((uint64_t)1 << 18) / d));
    {
        const uint64_t per = (C + G - 1) / G;
        lags_last[0] = ND; lags_last[1] = bands.size(); lags_last[2] = 0; lags_last[3] = 0; lags_last[4] = (n + L::LAGS_T - 1) / L::LAGS_T;
        lags_last[5] = G; lags_last[6] = std::min<uint64_t>((uint64_t)L::LAGS_TC, std::min<uint64_t>(per, C)); lags_last[7] = K;
    }
    DevBuf staged;
    const double* x = nullptr;
    int rc = stage_slab(draws_kdc, mem, n_keep, d, n_chains, st, staged, &x);
    if (rc) return rc;
    const Slab s{x, n, d, C, G, st};
    const bool stats = acov || ess || ended;
    const size_t part_per = (size_t)16 * L::LAGS_DIAGS;                 // doubles per (group, dimension) of the widest band
    Scratch S;
    HIP_TRY(S.alloc(G, d, stats ? part_per : 0));
    std::vector<double> a_h(d), e_h(d);
    if ((rc = two_part_centre(s, S, true, a_h, e_h))) return rc;
    if (mean) for (size_t j = 0; j < d; ++j) mean[j] = a_h[j] + e_h[j];

    if (rhat) {
        std::vector<double> mp((size_t)G * d * 3);
        hipLaunchKernelGGL(L::stats_moments_kernel, dim3((unsigned)d, G), dim3(64), 0, st, x, S.at(S.o_mean), (uint32_t)n, (uint32_t)d, (uint64_t)C, G, S.at(S.o_mom));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(mp.data(), S.at(S.o_mom), mp.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        rhat_from_moments(mp.data(), G, d, n, C, rhat);
    }
    if (!stats) { HIP_TRY(hipStreamSynchronize(st)); return MI_OK; }

    // the sums of lag k = 16 q + r0 come from offset q (its diagonals col - row = r0) and, for r0 > 0, from offset q + 1 (col - row = r0 - 16)
    std::vector<double> s_lo(nlag * d, 0.0), s_hi(nlag * d, 0.0), ac(nlag * d);
    std::vector<double> ess_h(d, (double)n);
    std::vector<uint8_t> met(d, 0);
    std::vector<uint32_t> active(d);
    for (size_t j = 0; j < d; ++j) active[j] = (uint32_t)j;
    std::vector<double> ap;
    size_t known = 0;                                    // lags [0, known) are complete for the active dimensions
    for (const Band& bd : bands) {
        if (active.empty()) break;
        const int ndb = (bd.hi - bd.lo <= 8) ? 8 : 16;
        const size_t na = active.size();
        const bool all_dims = na == d;
        if (!all_dims) {
            HIP_TRY(hipMemcpyAsync(S.at(S.o_dims), active.data(), na * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            lags_last[3] = lags_last[2] ? std::min<uint64_t>(lags_last[3], na) : na;
            ++lags_last[2];
        }
        const uint32_t* dl = all_dims ? nullptr : S.dims();
        const size_t lds = L::lags_lds_bytes(ndb);
        auto launch = [&](auto kern) -> int {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)na, G), dim3(256), lds, st, x, S.at(S.o_mean), (uint32_t)n, (uint32_t)d, (uint64_t)C, G, dl, bd.lo, S.at(S.o_part));
            return MI_OK;
        };
        if ((rc = (ndb == 8) ? launch(L::stats_band_kernel<8>) : launch(L::stats_band_kernel<16>))) return rc;
        HIP_TRY(hipGetLastError());
        const size_t stride = (size_t)ndb * L::LAGS_DIAGS;
        ap.resize((size_t)G * na * stride);
        HIP_TRY(hipMemcpyAsync(ap.data(), S.at(S.o_part), ap.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));              // (the dimension list of this frame has been read as well)
        for (size_t jj = 0; jj < na; ++jj) {
            const size_t j = active[jj];
            for (uint32_t dlt = bd.lo; dlt < bd.hi; ++dlt)
                for (int r = -15; r <= 15; ++r) {
                    const long long k = 16LL * dlt + r;
                    if (k < 0 || (size_t)k > K || (dlt == 0 && r < 0)) continue;
                    (r >= 0 ? s_lo : s_hi)[(size_t)k * d + j] = group_sum(&ap[jj * stride + (size_t)(dlt - bd.lo) * L::LAGS_DIAGS + (size_t)(r + 15)], G, na * stride);
                }
            const size_t done = std::min<size_t>(nlag, (size_t)16 * (bd.hi - 1) + 1);
            for (size_t k = known; k < done; ++k) {
                const double s_ = (k % 16) ? s_lo[k * d + j] + s_hi[k * d + j] : s_lo[k * d + j];
                ac[k * d + j] = s_ / (double)C / (double)(n - k);
            }
        }
        known = std::min<size_t>(nlag, (size_t)16 * (bd.hi - 1) + 1);
        // with acov == NULL a further band runs only over the dimensions whose sum is still open; the sum of a closed dimension is what the full
        // loop gives: it is the same loop, stopped at the same pair
        std::vector<uint32_t> next;
        for (uint32_t j : active) {
            bool hit;
            ess_h[j] = geyer_ess(ac.data(), d, j, n, known, &hit);
            met[j] = hit ? 1 : 0;
            if (acov || !hit) next.push_back(j);
        }
        active.swap(next);
    }
    if (acov) std::memcpy(acov, ac.data(), ac.size() * 8);
    if (ess) std::memcpy(ess, ess_h.data(), d * 8);
    if (ended) for (size_t j = 0; j < d; ++j) ended[j] = (met[j] || K == n - 1 || n < 4) ? 1 : 0;
    return MI_OK;
}

}  // namespace

extern "C" {

// test hooks, declared in mi_mcmc_probes.h: the host bookkeeping of this thread's last mi_mcmc_draw_stats / mi_mcmc_draw_stats_lags call (nothing
// reads it back), and the host arithmetic the two share, which needs no device
void mi_mcmc_test_draw_stats_last(uint64_t* out8) { if (out8) std::memcpy(out8, draw_stats_last, sizeof draw_stats_last); }
void mi_mcmc_test_draw_stats_lags_last(uint64_t* out8) { if (out8) std::memcpy(out8, lags_last, sizeof lags_last); }
void mi_mcmc_test_stats_host(const double* acov, uint64_t nlag, uint64_t d, uint64_t n, const double* moments, uint32_t G, uint64_t C, double* ess, uint8_t* hit,
                             double* rhat)
{
    bool h;
    for (uint64_t j = 0; acov && j < d; ++j) { ess[j] = geyer_ess(acov, d, j, n, nlag, &h); hit[j] = h ? 1 : 0; }
    if (moments) rhat_from_moments(moments, G, d, n, C, rhat);
}

// Pooled mean, autocovariance, R-hat and ESS of every dimension of a slab [n_keep][d][C] (draw_stats.hpp; the definitions: mcmc_amd/ess.py)
int mi_mcmc_draw_stats(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                       double* mean, double* acov, double* rhat, double* ess, void* stream)
{
    if (!draws_kdc || n_keep == 0 || d == 0 || n_chains == 0) return fail(MI_ERR_BAD_ARG, "draw_stats: empty input");
    (void)hipGetLastError();
    if (n_keep > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "draw_stats: n_keep does not fit 32 bits");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = n_keep, C = n_chains;
    DevBuf staged;
    const double* x = nullptr;
    int rc = stage_slab(draws_kdc, mem, n_keep, d, n_chains, st, staged, &x);
    if (rc) return rc;
    // chain groups (partials are added in order on the host).  The one-pass Gram kernel (n <= 128) wants few, long workgroups -- its
    // prologue (first tile) and epilogue (diagonal sums) are per workgroup, and every group is 16 NB x d doubles to fetch --: about 2 048
    // workgroups in all; the streamed kernels want many short ones.
    const bool gram = n <= (size_t)mi::STATS_GRAM_MAX_N;
    const uint32_t G = gram ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(64, (2048 + d - 1) / d), (C + 63) / 64))
                            : (uint32_t)std::min<uint64_t>(64, (C + 63) / 64);
    const bool tiled = n > (size_t)mi::STATS_MAX_N;                          // long series: lags below STATS_TILED_LAGS, streamed kernel
    const size_t nlag_max = tiled ? (size_t)mi::STATS_TILED_LAGS : n;
    {   // route, NB, G, 64-chain tiles of the largest (first) chain group, window launches, lag passes, lag passes over a subset, smallest subset
        const uint64_t per = (C + G - 1) / G;
        uint64_t* const L = draw_stats_last;
        L[0] = gram ? 0 : (tiled ? 2 : 1); L[1] = gram ? (n + 15) / 16 : 0; L[2] = G; L[3] = (std::min<uint64_t>(per, C) + 63) / 64;
        L[4] = L[5] = L[6] = L[7] = 0;
    }
    StatsCall c{{x, n, d, C, G, st}, nlag_max, acov != nullptr};
    // partials per (group, dimension): max(pass, tiled) lags, or the Gram kernel's lag sums and row sums
    const size_t pass_lags = (size_t)mi::STATS_PASS_BLOCKS * mi::STATS_LB;
    const size_t part_lags = tiled ? nlag_max : std::max<size_t>(std::max<size_t>(pass_lags, 16), gram ? ((n + 15) / 16) * 32 : 0);
    HIP_TRY(c.S.alloc(G, d, part_lags));
    c.a_h.resize(d);
    c.e_h.assign(d, 0.0);
    const bool stats = acov || rhat || ess;
    if (!stats) {                                         // the mean alone: every row, one pass
        if ((rc = row_mean(c, c.S, nullptr, 1u, (uint32_t)n, c.a_h))) return rc;
        if (mean) std::memcpy(mean, c.a_h.data(), d * 8);
        return MI_OK;
    }
    // the Gram route centres by a_j alone and finds e_j from its row sums: ONE pass over the slab; the other routes read it once more for e_j
    if ((rc = two_part_centre(c, c.S, !gram, c.a_h, c.e_h))) return rc;
    if (!gram && mean) for (size_t j = 0; j < d; ++j) mean[j] = c.a_h[j] + c.e_h[j];

    c.ac.assign((size_t)n * d, std::nan(""));
    c.active.resize(d);
    for (size_t j = 0; j < d; ++j) c.active[j] = (uint32_t)j;
    c.ess_h.assign(d, (double)n);
    if ((rc = gram ? c.route_gram() : tiled ? c.route_streamed() : c.route_window_blocks())) return rc;
    if (gram && mean) for (size_t j = 0; j < d; ++j) mean[j] = c.a_h[j] + c.e_h[j];
    if (acov) std::memcpy(acov, c.ac.data(), c.ac.size() * 8);
    if (rhat) rhat_from_moments(c.mp.data(), G, d, n, C, rhat);
    if (ess) std::memcpy(ess, c.ess_h.data(), d * 8);
    return MI_OK;
}

// Pooled mean, every autocovariance lag up to max_lag, R-hat, ESS and whether Geyer's sum ended, of every dimension of a slab [n_keep][d][C]
// (draw_stats_lags.hpp).  Validation first (it needs no device), then the device probe, then lags_run: one launch per band of block offsets.
int mi_mcmc_draw_stats_lags(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, uint32_t max_lag, double* mean, double* acov,
                            double* rhat, double* ess, uint8_t* ended, void* stream)
{
    const char* who = "draw_stats_lags";
    if (!draws_kdc) return fail(MI_ERR_BAD_ARG, "%s: null slab", who);
    if (n_keep == 0 || d == 0 || n_chains == 0) return fail(MI_ERR_BAD_ARG, "%s: empty input", who);
    if (n_keep > 0xffffffffULL || n_chains > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: n_keep / n_chains do not fit 32 bits", who);
    if (d > 65536) return fail(MI_ERR_BAD_ARG, "%s: d = %llu is beyond 65536", who, (unsigned long long)d);
    if (!mean && !acov && !rhat && !ess && !ended) return fail(MI_ERR_BAD_ARG, "%s: all five outputs are NULL, nothing is asked for", who);
    int rc = need_device();
    if (rc) return rc;
    try {
        return lags_run(draws_kdc, mem, n_keep, d, n_chains, max_lag, mean, acov, rhat, ess, ended, static_cast<hipStream_t>(stream));
    } catch (const std::bad_alloc&) {
        return fail(MI_ERR_OOM, "%s: the host arrays of %llu lags x %llu dimensions do not fit", who, (unsigned long long)std::min<uint64_t>(max_lag, n_keep - 1) + 1,
                    (unsigned long long)d);
    }
}

// The device form of mi_mcmc_draws_to_chain_major (stats_collate.hip: the host loops), here with its kernel's header
int mi_mcmc_draws_to_chain_major_device(const double* kdc_dev, uint64_t n_keep, uint64_t d, uint64_t C, double* out_dev, void* stream)
{
    if (!kdc_dev || !out_dev) return fail(MI_ERR_BAD_ARG, "null buffer");
    if (n_keep == 0 || d == 0 || C == 0) return MI_OK;
    if (n_keep > 0xffffffffULL || d > 0x7fffffffULL || (C + 63) / 64 > 65535ULL * 64ULL) return fail(MI_ERR_BAD_ARG, "draws_to_chain_major: shape out of range");
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    // grid.y is limited to 65 535: chains in slices of 65 535 tiles
    const uint64_t tiles = (C + 63) / 64;
    for (uint64_t t0 = 0; t0 < tiles; t0 += 65535) {
        const uint64_t nt = std::min<uint64_t>(65535, tiles - t0);
        const uint64_t c_first = t0 * 64, c_cnt = std::min<uint64_t>(C - c_first, nt * 64);
        // a slice [c_first, c_first + c_cnt) of the slab has the same row stride C: pass the full C and offset pointers
        hipLaunchKernelGGL(mi::draws_to_chain_major_slice_kernel, dim3((unsigned)d, (unsigned)nt), dim3(256), 0, st, kdc_dev, (uint32_t)n_keep, (uint32_t)d, C, c_first, c_cnt, out_dev);
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // extern "C"
