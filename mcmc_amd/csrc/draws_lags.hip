// draws_lags.hip -- mi_mcmc_draw_stats_lags (include/mi_mcmc.h): the host ladder around the banded-Gram kernel of draw_stats_lags.hpp.  Validation first
// (it needs no device), then the device probe, the slab staged where the caller holds it on the host, a device buffer of the call's own (never the
// stream's leased workspace: mi_mcmc_draw_stats_ranked_lags calls in while it holds that lease) and the launches, one per band of block offsets.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "host_common.hpp"
#include "draw_stats_lags.hpp"

using namespace mi::host;       // fail, need_device, DevBuf (host_common.hpp)

namespace {

thread_local uint64_t lags_last[8];

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
    const double* x = draws_kdc;
    if (mem == MI_MEM_HOST) {
        HIP_TRY(staged.alloc(n * d * C * 8));
        HIP_TRY(hipMemcpyAsync(staged.p, draws_kdc, n * d * C * 8, hipMemcpyHostToDevice, st));
        x = staged.as<double>();
    }
    const bool stats = acov || ess || ended;
    const size_t part_per = (size_t)16 * L::LAGS_DIAGS;                 // doubles per (group, dimension) of the widest band
    DevBuf buf;
    const size_t o_sum = 0, o_mean = o_sum + (size_t)G * d, o_dims = o_mean + 2 * d, o_mom = o_dims + d, o_part = o_mom + (size_t)G * d * 3;
    HIP_TRY(buf.alloc((o_part + (stats ? (size_t)G * d * part_per : 0)) * 8));
    double* const B = buf.as<double>();
    // the centre in two parts, as the streamed routes of mi_mcmc_draw_stats have it: a_j, the mean over the chains of the first, middle and last row,
    // and e_j, the mean of x - a_j over the slab; v = (x - a_j) - e_j and mean_j = a_j + e_j
    const uint32_t t_step = (uint32_t)std::max<size_t>(1, (n - 1) / 2);
    const uint32_t n_sum = (uint32_t)((n + t_step - 1) / t_step);
    std::vector<double> part((size_t)G * d), a_h(d), e_h(d);
    auto row_mean = [&](const double* centre, uint32_t step, uint32_t rows, std::vector<double>& dst) -> int {
        hipLaunchKernelGGL(L::stats_lags_sum_kernel, dim3((unsigned)d, G), dim3(64), 0, st, x, centre, (uint32_t)n, step, (uint32_t)d, (uint64_t)C, G, B + o_sum);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(part.data(), B + o_sum, part.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t j = 0; j < d; ++j) {
            double s = 0.0;
            for (uint32_t g = 0; g < G; ++g) s += part[(size_t)g * d + j];
            dst[j] = s / ((double)rows * (double)C);
        }
        return MI_OK;
    };
    int rc;
    if ((rc = row_mean(nullptr, t_step, n_sum, a_h))) return rc;
    HIP_TRY(hipMemcpyAsync(B + o_mean, a_h.data(), d * 8, hipMemcpyHostToDevice, st));
    if ((rc = row_mean(B + o_mean, 1u, (uint32_t)n, e_h))) return rc;
    HIP_TRY(hipMemcpyAsync(B + o_mean + d, e_h.data(), d * 8, hipMemcpyHostToDevice, st));
    if (mean) for (size_t j = 0; j < d; ++j) mean[j] = a_h[j] + e_h[j];

    if (rhat) {
        std::vector<double> mp((size_t)G * d * 3);
        hipLaunchKernelGGL(L::stats_moments_kernel, dim3((unsigned)d, G), dim3(64), 0, st, x, B + o_mean, (uint32_t)n, (uint32_t)d, (uint64_t)C, G, B + o_mom);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(mp.data(), B + o_mom, mp.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t j = 0; j < d; ++j) {                 // the expression of mi_mcmc_draw_stats
            double sm = 0.0, sm2 = 0.0, sv = 0.0;
            for (uint32_t g = 0; g < G; ++g) { const double* o = &mp[((size_t)g * d + j) * 3]; sm += o[0]; sm2 += o[1]; sv += o[2]; }
            const double W = sv / (double)C;
            const double mbar = sm / (double)C;
            const double B_over_n = (C > 1) ? (sm2 - (double)C * mbar * mbar) / (double)(C - 1) : 0.0;
            const double var_plus = ((double)(n - 1) / (double)n) * W + B_over_n;
            rhat[j] = (W > 0.0) ? std::sqrt(var_plus / W) : 1.0;
        }
    }
    if (!stats) { HIP_TRY(hipStreamSynchronize(st)); return MI_OK; }

    // the sums of lag k = 16 q + r0 come from offset q (its diagonals col - row = r0) and, for r0 > 0, from offset q + 1 (col - row = r0 - 16)
    std::vector<double> s_lo(nlag * d, 0.0), s_hi(nlag * d, 0.0), ac(nlag * d);
    std::vector<double> ess_h(d, (double)n);
    std::vector<uint8_t> met(d, 0);
    // Geyer's initial positive sequence over the lags [0, known) (mcmc_amd/ess.py's loop); *hit: the sum met its first non-positive pair
    auto geyer = [&](size_t known, size_t j, bool* hit) -> double {
        *hit = false;
        if (n < 4) return (double)n;
        const double a0 = ac[j];
        const double den = (a0 > 0.0) ? a0 : 1.0;
        double tau = -1.0;
        for (size_t t = 0; t + 1 < known; t += 2) {
            const double pair = ac[t * d + j] / den + ac[(t + 1) * d + j] / den;
            if (pair <= 0.0) { *hit = true; break; }
            tau += 2.0 * pair;
        }
        const double e = (tau > 0.0) ? (double)n / std::max(tau, 1.0 / (double)n) : (double)n;
        return std::min(e, (double)n * 10.0);
    };
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
            HIP_TRY(hipMemcpyAsync(B + o_dims, active.data(), na * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            lags_last[3] = lags_last[2] ? std::min<uint64_t>(lags_last[3], na) : na;
            ++lags_last[2];
        }
        const uint32_t* dl = all_dims ? nullptr : reinterpret_cast<const uint32_t*>(B + o_dims);
        const size_t lds = L::lags_lds_bytes(ndb);
        if (ndb == 8) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(L::stats_band_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(L::stats_band_kernel<8>, dim3((unsigned)na, G), dim3(256), lds, st, x, B + o_mean, (uint32_t)n, (uint32_t)d, (uint64_t)C, G, dl, bd.lo, B + o_part);
        } else {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(L::stats_band_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(L::stats_band_kernel<16>, dim3((unsigned)na, G), dim3(256), lds, st, x, B + o_mean, (uint32_t)n, (uint32_t)d, (uint64_t)C, G, dl, bd.lo, B + o_part);
        }
        HIP_TRY(hipGetLastError());
        const size_t stride = (size_t)ndb * L::LAGS_DIAGS;
        ap.resize((size_t)G * na * stride);
        HIP_TRY(hipMemcpyAsync(ap.data(), B + o_part, ap.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));              // (the dimension list of this frame has been read as well)
        for (size_t jj = 0; jj < na; ++jj) {
            const size_t j = active[jj];
            for (uint32_t dlt = bd.lo; dlt < bd.hi; ++dlt)
                for (int r = -15; r <= 15; ++r) {
                    const long long k = 16LL * dlt + r;
                    if (k < 0 || (size_t)k > K || (dlt == 0 && r < 0)) continue;
                    double s_ = 0.0;                     // the chain groups in ascending order
                    for (uint32_t g = 0; g < G; ++g) s_ += ap[((size_t)g * na + jj) * stride + (size_t)(dlt - bd.lo) * L::LAGS_DIAGS + (size_t)(r + 15)];
                    (r >= 0 ? s_lo : s_hi)[(size_t)k * d + j] = s_;
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
            ess_h[j] = geyer(known, j, &hit);
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

// test hook, declared in mi_mcmc_probes.h: the host bookkeeping of this thread's last mi_mcmc_draw_stats_lags call (nothing reads it back)
void mi_mcmc_test_draw_stats_lags_last(uint64_t* out8)
{
    if (out8) std::memcpy(out8, lags_last, sizeof lags_last);
}

// Pooled mean, every autocovariance lag up to max_lag, R-hat, ESS and whether Geyer's sum ended, of every dimension of a slab [n_keep][d][C]
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

}  // extern "C"
