// draws_api.hip -- the C ABI's reducers over a draws slab [n_keep][d][C] (include/mi_mcmc.h): host drivers around the kernels of
// draws_cov.hip, draws_nested.hip, draws_select.hip, draws_rank.hip, draws_logk.hip, draws_waic.hip, draws_psis.hip, draws_loglik.hip, draws_bridge.hip and draws_predict.hip.  Validation first (it needs no device), then the device probe, then the slab
// staged on the device where the caller holds it on the host, the workspace of the stream (workspace.hpp) and the launches.  No sampler lives here.
// mi_mcmc_draw_stats and mi_mcmc_draw_stats_lags are draw_stats.hip; the ranked drivers below reach them through the C ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "host_common.hpp"
#include "workspace.hpp"
#include "det_math.hpp"
#include "draws_cov.hpp"
#include "draws_nested.hpp"
#include "draws_select.hpp"
#include "draws_rank.hpp"
#include "draws_logk.hpp"
#include "draws_waic.hpp"
#include "draws_psis.hpp"
#include "draws_loglik.hpp"
#include "draws_bridge.hpp"
#include "draws_predict.hpp"
#include "launch_common.hpp"

using namespace mi::host;       // fail, need_device, DevBuf, stage_slab (host_common.hpp); WsLease, ws_get (workspace.hpp)

namespace {

// The type-7 quantile rule, (lo, hi, g) for one probability over S samples and the value from the two order statistics; the arithmetic below IS
// include/mi_mcmc.h's statement (this file is compiled with -ffp-contract=off: nothing is fused)
void type7_ranks(uint64_t S, double prob, uint64_t* lo, uint64_t* hi, double* g)
{
    const double h = prob * (double)(S - 1);
    const double fl = std::floor(h);
    *lo = fl >= (double)(S - 1) ? S - 1 : (uint64_t)fl;
    *g = h - (double)*lo;
    *hi = *lo + 1 < S ? *lo + 1 : S - 1;
}
double type7_value(double x_lo, double x_hi, double g)
{
    if (g == 0.0) return x_lo;
    const double diff = x_hi - x_lo;
    const double prod = g * diff;
    return x_lo + prod;
}

}  // namespace

extern "C" {

// test hooks, declared in mi_mcmc_probes.h: the workspace budget of the rank transform's groups of dimensions (draws_rank.hpp), the host arithmetic
// of its group rule and of the plan of mi_mcmc_draws_log_kernel, which need no device
static std::atomic<uint64_t> g_rank_ws_bytes{0};
void mi_mcmc_test_set_rank_ws_bytes(uint64_t bytes) { g_rank_ws_bytes.store(bytes, std::memory_order_relaxed); }
void mi_mcmc_test_rank_counts(uint64_t* sorts, uint64_t* passes) { mi::drank::rank_counts(sorts, passes); }
uint64_t mi_mcmc_test_rank_dim_bytes(uint64_t n_keep, uint64_t n_chains, uint32_t flags, int stats)
{
    return mi::drank::rank_dim_bytes(n_keep, n_chains, flags, stats != 0);
}
uint64_t mi_mcmc_test_rank_dims_per_group(uint64_t n_keep, uint64_t d, uint64_t n_chains, uint32_t flags, int stats)
{
    return mi::drank::rank_plan(n_keep, d, n_chains, flags, stats != 0, g_rank_ws_bytes.load(std::memory_order_relaxed)).dims_per_group;
}
void mi_mcmc_test_logk_plan(int32_t kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, int slab_host, int target_host, uint64_t* out8)
{
    const mi::dlogk::LogkPlan p = mi::dlogk::logk_plan(kind, d, n_rows, n_keep, n_chains, slab_host != 0, target_host != 0);
    out8[0] = (uint64_t)p.route; out8[1] = p.grid; out8[2] = p.block; out8[3] = p.lds_bytes;
    out8[4] = p.Kp; out8[5] = p.ldA; out8[6] = p.n_row_tiles; out8[7] = p.bytes;
}

// Pooled mean and covariance of the K = n_keep * C columns of a slab [n_keep][d][C] (draws_cov.hip; the arithmetic: include/mi_mcmc.h)
int mi_mcmc_draws_covariance(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, double* mean, double* cov, void* stream)
{
    if (!draws_kdc) return fail(MI_ERR_BAD_ARG, "draws_covariance: null slab");
    if (d == 0) return fail(MI_ERR_BAD_ARG, "draws_covariance: d must be positive");
    if (!mean && !cov) return fail(MI_ERR_BAD_ARG, "draws_covariance: mean and cov are both NULL, nothing is asked for");
    if (n_keep > 0xffffffffULL || n_chains > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "draws_covariance: n_keep / n_chains do not fit 32 bits");
    if (n_keep * n_chains < 2) return fail(MI_ERR_BAD_ARG, "draws_covariance: K = n_keep * n_chains = %llu, at least 2 samples are needed", (unsigned long long)(n_keep * n_chains));
    if (d > mi::dcov::COV_MAX_D) return fail(MI_ERR_BAD_ARG, "draws_covariance: d = %llu is beyond %llu", (unsigned long long)d, (unsigned long long)mi::dcov::COV_MAX_D);
    int rc = need_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf staged;
    const double* x = nullptr;
    if ((rc = stage_slab(draws_kdc, mem, n_keep, d, n_chains, st, staged, &x))) return rc;
    const mi::dcov::CovPlan plan = mi::dcov::cov_plan(n_keep, d, n_chains, cov != nullptr);
    WsLease ws;
    rc = ws_get(st, plan.bytes, ws);
    if (rc) return rc;
    HIP_TRY((hipError_t)mi::dcov::cov_run(x, d, n_chains, plan, ws.p, cov != nullptr, st));
    if (mean) HIP_TRY(hipMemcpyAsync(mean, ws.as<double>() + plan.o_mean, d * 8, hipMemcpyDeviceToHost, st));
    if (cov) HIP_TRY(hipMemcpyAsync(cov, ws.as<double>() + plan.o_cov, d * d * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                   // blocking: the outputs are the caller's host arrays, the staged slab and the workspace are ours
    return MI_OK;
}

// The checks that mi_mcmc_draw_stats_nested and mi_mcmc_draw_stats_nested_ranked share: they need no device
static int nested_check(const char* who, const double* draws_kdc, uint64_t n_keep, uint64_t d, uint64_t n_chains, uint64_t M, bool any_output, const char* n_outputs)
{
    if (!draws_kdc) return fail(MI_ERR_BAD_ARG, "%s: null slab", who);
    if (!any_output) return fail(MI_ERR_BAD_ARG, "%s: all %s outputs are NULL, nothing is asked for", who, n_outputs);
    if (d == 0) return fail(MI_ERR_BAD_ARG, "%s: d must be positive", who);
    if (d > mi::dnest::NESTED_MAX_D) return fail(MI_ERR_BAD_ARG, "%s: d = %llu is beyond %llu", who, (unsigned long long)d, (unsigned long long)mi::dnest::NESTED_MAX_D);
    if (n_keep == 0 || n_chains == 0) return fail(MI_ERR_BAD_ARG, "%s: n_keep and n_chains must be positive", who);
    if (n_keep > 0xffffffffULL || n_chains > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: n_keep / n_chains do not fit 32 bits", who);
    if (M == 0) return fail(MI_ERR_BAD_ARG, "%s: chains_per_super must be positive", who);
    if (n_chains % M != 0)
        return fail(MI_ERR_BAD_ARG, "%s: n_chains = %llu is not a multiple of chains_per_super = %llu", who, (unsigned long long)n_chains, (unsigned long long)M);
    if (n_chains / M < 2) return fail(MI_ERR_BAD_ARG, "%s: K = n_chains / chains_per_super = %llu, at least 2 superchains are needed", who, (unsigned long long)(n_chains / M));
    if (n_keep == 1 && M == 1) return fail(MI_ERR_BAD_ARG, "%s: n_keep = 1 with chains_per_super = 1, the within variance is identically 0", who);
    return MI_OK;
}

// nrhat and mcse_mean from between and within, on the host (the arithmetic: include/mi_mcmc.h)
static double nested_rhat(double between, double within)
{
    const double ratio = between / within;
    const double u = 1.0 + ratio;
    return std::sqrt(u);
}

// Nested R-hat of a slab [n_keep][d][C] whose chains are K = C / M superchains of M consecutive chains (draws_nested.hip; the arithmetic: include/mi_mcmc.h)
int mi_mcmc_draw_stats_nested(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, uint64_t chains_per_super, double* nrhat,
                              double* mean, double* between, double* within, double* mcse_mean, double* super_mean, void* stream)
{
    int rc = nested_check("draw_stats_nested", draws_kdc, n_keep, d, n_chains, chains_per_super, nrhat || mean || between || within || mcse_mean || super_mean, "six");
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf staged;
    const double* x = nullptr;
    if ((rc = stage_slab(draws_kdc, mem, n_keep, d, n_chains, st, staged, &x))) return rc;
    const mi::dnest::NestedPlan plan = mi::dnest::nested_plan(n_keep, d, n_chains, chains_per_super, super_mean != nullptr);
    WsLease ws;
    rc = ws_get(st, plan.bytes, ws);
    if (rc) return rc;
    HIP_TRY((hipError_t)mi::dnest::nested_run(x, plan, ws.p, super_mean != nullptr, st));
    std::vector<double> out(3 * d);
    HIP_TRY(hipMemcpyAsync(out.data(), ws.as<double>() + plan.o_out, 3 * d * 8, hipMemcpyDeviceToHost, st));
    if (super_mean) HIP_TRY(hipMemcpyAsync(super_mean, ws.as<double>() + plan.o_super, plan.K * d * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                   // blocking: the outputs are the caller's host arrays, the staged slab and the workspace are ours
    const double Kd = (double)plan.K;
    for (uint64_t i = 0; i < d; ++i) {
        const double b = out[d + i], w = out[2 * d + i];
        if (mean) mean[i] = out[i];
        if (between) between[i] = b;
        if (within) within[i] = w;
        if (nrhat) nrhat[i] = nested_rhat(b, w);
        if (mcse_mean) mcse_mean[i] = std::sqrt(b / Kd);
    }
    return MI_OK;
}

// The checks that mi_mcmc_draws_order_stats and mi_mcmc_draws_quantiles share: they need no device
static int order_stats_check(const char* who, const double* draws_kdc, uint64_t n_keep, uint64_t d, uint64_t n_chains, const double* out)
{
    if (!draws_kdc) return fail(MI_ERR_BAD_ARG, "%s: null slab", who);
    if (!out) return fail(MI_ERR_BAD_ARG, "%s: out is NULL", who);
    if (d == 0) return fail(MI_ERR_BAD_ARG, "%s: d must be positive", who);
    if (n_keep > 0xffffffffULL || n_chains > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: n_keep / n_chains do not fit 32 bits", who);
    if (n_keep * n_chains == 0) return fail(MI_ERR_BAD_ARG, "%s: K = n_keep * n_chains = 0, at least 1 sample is needed", who);
    if (d > mi::dsel::SEL_MAX_D) return fail(MI_ERR_BAD_ARG, "%s: d = %llu is beyond %llu", who, (unsigned long long)d, (unsigned long long)mi::dsel::SEL_MAX_D);
    return MI_OK;
}

// out [n_ranks][d] on the host <- the order statistics of a checked call (draws_select.hip); blocking
static int order_stats_run(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, const uint64_t* ranks, uint32_t n_ranks, double* out,
                    void* stream)
{
    int rc = need_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf staged;
    const double* x = nullptr;
    if ((rc = stage_slab(draws_kdc, mem, n_keep, d, n_chains, st, staged, &x))) return rc;
    mi::dsel::SelRanks r{};
    for (uint32_t a = 0; a < n_ranks; ++a) r.r[a] = ranks[a];
    const mi::dsel::SelPlan plan = mi::dsel::sel_plan(n_keep, d, n_chains, n_ranks);
    WsLease ws;
    rc = ws_get(st, plan.bytes, ws);
    if (rc) return rc;
    HIP_TRY((hipError_t)mi::dsel::sel_run(x, n_keep, d, n_chains, r, n_ranks, plan, ws.p, st));
    HIP_TRY(hipMemcpyAsync(out, ws.as<char>() + plan.o_out, (size_t)n_ranks * d * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                   // blocking: out is the caller's host array, the staged slab and the workspace are ours
    return MI_OK;
}

// The ranks[a]-th smallest key of every dimension of a slab [n_keep][d][C], as a value (the key, the order: include/mi_mcmc.h)
int mi_mcmc_draws_order_stats(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, const uint64_t* ranks, uint32_t n_ranks,
                              double* out, void* stream)
{
    const char* who = "draws_order_stats";
    int rc = order_stats_check(who, draws_kdc, n_keep, d, n_chains, out);
    if (rc) return rc;
    if (!ranks) return fail(MI_ERR_BAD_ARG, "%s: ranks is NULL", who);
    if (n_ranks == 0 || n_ranks > MI_ORDER_STATS_MAX_RANKS) return fail(MI_ERR_BAD_ARG, "%s: n_ranks = %u, must be 1 .. %d", who, n_ranks, MI_ORDER_STATS_MAX_RANKS);
    const uint64_t K = n_keep * n_chains;
    for (uint32_t a = 0; a < n_ranks; ++a)
        if (ranks[a] >= K) return fail(MI_ERR_BAD_ARG, "%s: ranks[%u] = %llu is not below K = %llu", who, a, (unsigned long long)ranks[a], (unsigned long long)K);
    return order_stats_run(draws_kdc, mem, n_keep, d, n_chains, ranks, n_ranks, out, stream);
}

// Type-7 quantiles from two order statistics per probability (type7_ranks / type7_value above)
int mi_mcmc_draws_quantiles(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, const double* probs, uint32_t n_probs,
                            double* out, void* stream)
{
    const char* who = "draws_quantiles";
    int rc = order_stats_check(who, draws_kdc, n_keep, d, n_chains, out);
    if (rc) return rc;
    if (!probs) return fail(MI_ERR_BAD_ARG, "%s: probs is NULL", who);
    if (n_probs == 0 || n_probs > MI_ORDER_STATS_MAX_RANKS / 2) return fail(MI_ERR_BAD_ARG, "%s: n_probs = %u, must be 1 .. %d", who, n_probs, MI_ORDER_STATS_MAX_RANKS / 2);
    for (uint32_t a = 0; a < n_probs; ++a)
        if (!(probs[a] >= 0.0 && probs[a] <= 1.0)) return fail(MI_ERR_BAD_ARG, "%s: probs[%u] = %g is not in [0, 1]", who, a, probs[a]);
    const uint64_t K = n_keep * n_chains;
    uint64_t ranks[MI_ORDER_STATS_MAX_RANKS];
    double g[MI_ORDER_STATS_MAX_RANKS / 2];
    for (uint32_t a = 0; a < n_probs; ++a) type7_ranks(K, probs[a], &ranks[2 * a], &ranks[2 * a + 1], &g[a]);
    std::vector<double> os((size_t)2 * n_probs * d);
    rc = order_stats_run(draws_kdc, mem, n_keep, d, n_chains, ranks, 2 * n_probs, os.data(), stream);
    if (rc) return rc;
    for (uint32_t a = 0; a < n_probs; ++a) {
        const double* x_lo = os.data() + (size_t)(2 * a) * d;
        const double* x_hi = x_lo + d;
        for (uint64_t i = 0; i < d; ++i) out[(size_t)a * d + i] = type7_value(x_lo[i], x_hi[i], g[a]);
    }
    return MI_OK;
}

// The checks that mi_mcmc_draws_rank_transform and mi_mcmc_draw_stats_ranked share: they need no device
static int rank_check(const char* who, const double* draws_kdc, uint64_t n_keep, uint64_t d, uint64_t n_chains, uint32_t flags)
{
    if (!draws_kdc) return fail(MI_ERR_BAD_ARG, "%s: null slab", who);
    if (d == 0) return fail(MI_ERR_BAD_ARG, "%s: d must be positive", who);
    if (d > mi::drank::RANK_MAX_D) return fail(MI_ERR_BAD_ARG, "%s: d = %llu is beyond %llu", who, (unsigned long long)d, (unsigned long long)mi::drank::RANK_MAX_D);
    if (n_keep > 0xffffffffULL || n_chains > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: n_keep / n_chains do not fit 32 bits", who);
    if (flags & ~(uint32_t)(MI_RANK_SPLIT | MI_RANK_FOLD)) return fail(MI_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", who, flags);
    if ((flags & MI_RANK_SPLIT) && n_keep < 2) return fail(MI_ERR_BAD_ARG, "%s: n_keep = %llu, MI_RANK_SPLIT needs at least 2 draws", who, (unsigned long long)n_keep);
    const uint64_t rows = (flags & MI_RANK_SPLIT) ? 2 * (n_keep / 2) : n_keep;
    // rows, n_chains < 2^32: the product does not wrap
    if (rows * n_chains == 0) return fail(MI_ERR_BAD_ARG, "%s: S = 0 retained samples, at least 1 is needed", who);
    if (rows * n_chains > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: S = %llu retained samples per dimension, must be below 2^32", who, (unsigned long long)(rows * n_chains));
    return MI_OK;
}

// med (and with tails the 5 % and 95 % quantiles) of the group's dimensions out of the sorted image of their un-folded keys, onto the device at
// ws + o_med (+ o_q); nan_dims (may be NULL): whether the dimension holds a NaN (its largest key is the NaN key)
static int rank_group_quantiles(const mi::drank::RankPlan& plan, uint64_t dim0, uint64_t nd, const uint64_t* sorted, bool tails, char* W, hipStream_t st,
                         std::vector<double>& os, std::vector<double>& q, std::vector<uint8_t>* nan_dims)
{
    const double probs[3] = {0.5, 0.05, 0.95};
    uint64_t ranks[8];
    double g[3];
    for (int a = 0; a < 3; ++a) type7_ranks(plan.S, probs[a], &ranks[2 * a], &ranks[2 * a + 1], &g[a]);
    ranks[6] = ranks[7] = plan.S - 1;                    // the largest key: the NaN key if the dimension holds a NaN
    os.resize(8 * nd);
    q.resize(3 * nd);
    HIP_TRY((hipError_t)mi::drank::rank_order_stats_group(plan, nd, sorted, ranks, W, os.data(), st));
    if (nan_dims)
        for (uint64_t j = 0; j < nd; ++j) (*nan_dims)[dim0 + j] = os[6 * nd + j] != os[6 * nd + j];
    for (int a = 0; a < 3; ++a)
        for (uint64_t j = 0; j < nd; ++j) q[a * nd + j] = type7_value(os[(2 * a) * nd + j], os[(2 * a + 1) * nd + j], g[a]);
    HIP_TRY(hipMemcpyAsync(W + plan.o_med + dim0 * 8, q.data(), nd * 8, hipMemcpyHostToDevice, st));
    if (tails) {
        HIP_TRY(hipMemcpyAsync(W + plan.o_q + dim0 * 8, q.data() + nd, nd * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(W + plan.o_q + (plan.d + dim0) * 8, q.data() + 2 * nd, nd * 8, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));                   // q is this frame's: the uploads have read it
    return MI_OK;
}

// Average ranks / normal scores of the retained samples of a slab [n_keep][d][C] (draws_rank.hip; the definitions: include/mi_mcmc.h)
int mi_mcmc_draws_rank_transform(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, int32_t what, uint32_t flags,
                                 double* out, void* stream)
{
    const char* who = "draws_rank_transform";
    int rc = rank_check(who, draws_kdc, n_keep, d, n_chains, flags);
    if (rc) return rc;
    if (!out) return fail(MI_ERR_BAD_ARG, "%s: out is NULL", who);
    if (what != MI_RANK_AVERAGE && what != MI_RANK_NORMAL) return fail(MI_ERR_BAD_ARG, "%s: what = %d is neither MI_RANK_AVERAGE nor MI_RANK_NORMAL", who, what);
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const mi::drank::RankPlan plan = mi::drank::rank_plan(n_keep, d, n_chains, flags, false, g_rank_ws_bytes.load(std::memory_order_relaxed));
    DevBuf staged, out_dev;
    const double* x = nullptr;
    double* o = out;
    if ((rc = stage_slab(draws_kdc, mem, n_keep, d, n_chains, st, staged, &x))) return rc;
    if (mem == MI_MEM_HOST) {
        HIP_TRY(out_dev.alloc(plan.S * d * 8));
        o = out_dev.as<double>();
    }
    WsLease ws;
    rc = ws_get(st, plan.bytes, ws);
    if (rc) return rc;
    char* W = ws.as<char>();
    const bool fold = (flags & MI_RANK_FOLD) != 0;
    std::vector<double> os, q;
    for (uint64_t dim0 = 0; dim0 < d; dim0 += plan.dims_per_group) {
        const uint64_t nd = std::min<uint64_t>(plan.dims_per_group, d - dim0);
        const uint64_t* sorted = nullptr;
        HIP_TRY((hipError_t)mi::drank::rank_sort_group(x, plan, dim0, nd, false, W, st, &sorted));
        if (fold) {                                      // the medians out of the un-folded image, then the sort of |x - med|
            rc = rank_group_quantiles(plan, dim0, nd, sorted, false, W, st, os, q, nullptr);
            if (rc) return rc;
            HIP_TRY((hipError_t)mi::drank::rank_sort_group(x, plan, dim0, nd, true, W, st, &sorted));
        }
        HIP_TRY((hipError_t)mi::drank::rank_lookup_group(x, plan, dim0, nd, fold, what, sorted, W, o, d, dim0, st));
    }
    if (mem == MI_MEM_HOST) HIP_TRY(hipMemcpyAsync(out, o, plan.S * d * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                   // blocking: the staged slab, the staged output and the workspace are ours
    return MI_OK;
}

}  // extern "C"

// Rank-normalised split-R-hat, bulk-ESS and tail-ESS: the pieces above and a reducer of the composed slabs [h][nd][2C] on the device, called as
// reduce(slab, h, nd, C2, rhat or NULL, ess or NULL, ended or NULL) -- mi_mcmc_draw_stats for mi_mcmc_draw_stats_ranked (ended is NULL there),
// mi_mcmc_draw_stats_lags with the caller's max_lag for mi_mcmc_draw_stats_ranked_lags, where ended[j] = 1 only if all three ESS sums ended
template <class Reduce>
static int draw_stats_ranked_run(const char* who, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, double* rhat, double* rhat_bulk,
                                 double* rhat_tail, double* ess_bulk, double* ess_tail, uint8_t* ended, bool has_ended, void* stream, Reduce reduce)
{
    int rc = rank_check(who, draws_kdc, n_keep, d, n_chains, MI_RANK_SPLIT);
    if (rc) return rc;
    if (!rhat && !rhat_bulk && !rhat_tail && !ess_bulk && !ess_tail && !ended)
        return fail(MI_ERR_BAD_ARG, has_ended ? "%s: all six outputs are NULL, nothing is asked for" : "%s: all five outputs are NULL, nothing is asked for", who);
    if (n_keep < 4) return fail(MI_ERR_BAD_ARG, "%s: n_keep = %llu, at least 4 draws are needed (two halves of two)", who, (unsigned long long)n_keep);
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const mi::drank::RankPlan plan = mi::drank::rank_plan(n_keep, d, n_chains, MI_RANK_SPLIT, true, g_rank_ws_bytes.load(std::memory_order_relaxed));
    DevBuf staged;
    const double* x = nullptr;
    if ((rc = stage_slab(draws_kdc, mem, n_keep, d, n_chains, st, staged, &x))) return rc;
    WsLease ws;
    rc = ws_get(st, plan.bytes, ws);
    if (rc) return rc;
    char* W = ws.as<char>();
    double* slab = reinterpret_cast<double*>(W + plan.o_slab);
    const bool want_bulk = rhat || rhat_bulk || ess_bulk || ended, want_fold = rhat || rhat_tail, want_tail = ess_tail || ended;
    std::vector<double> rb(d), rt(d), eb(d), et(d), e05, e95, os, q;
    std::vector<uint8_t> has_nan(d, 0), en_b, en_05, en_95;
    if (ended) { en_b.resize(d); std::memset(ended, 1, d); }
    const uint64_t h = plan.h, C2 = 2 * n_chains;
    for (uint64_t dim0 = 0; dim0 < d; dim0 += plan.dims_per_group) {
        const uint64_t nd = std::min<uint64_t>(plan.dims_per_group, d - dim0);
        const uint64_t* sorted = nullptr;
        HIP_TRY((hipError_t)mi::drank::rank_sort_group(x, plan, dim0, nd, false, W, st, &sorted));
        rc = rank_group_quantiles(plan, dim0, nd, sorted, true, W, st, os, q, &has_nan);
        if (rc) return rc;
        if (want_bulk) {
            HIP_TRY((hipError_t)mi::drank::rank_lookup_group(x, plan, dim0, nd, false, MI_RANK_NORMAL, sorted, W, slab, nd, 0, st));
            rc = reduce(slab, h, nd, C2, rb.data() + dim0, (ess_bulk || ended) ? eb.data() + dim0 : nullptr, ended ? en_b.data() + dim0 : nullptr);
            if (rc) return rc;
        }
        if (want_tail) {
            e05.resize(nd); e95.resize(nd);
            if (ended) { en_05.resize(nd); en_95.resize(nd); }
            HIP_TRY((hipError_t)mi::drank::rank_indicator_group(x, plan, dim0, nd, 0, W, slab, st));
            rc = reduce(slab, h, nd, C2, nullptr, e05.data(), ended ? en_05.data() : nullptr);
            if (rc) return rc;
            HIP_TRY((hipError_t)mi::drank::rank_indicator_group(x, plan, dim0, nd, 1, W, slab, st));
            rc = reduce(slab, h, nd, C2, nullptr, e95.data(), ended ? en_95.data() : nullptr);
            if (rc) return rc;
            for (uint64_t j = 0; j < nd; ++j) et[dim0 + j] = e95[j] < e05[j] ? e95[j] : e05[j];
            if (ended) for (uint64_t j = 0; j < nd; ++j) ended[dim0 + j] = (en_b[dim0 + j] && en_05[j] && en_95[j]) ? 1 : 0;
        }
        if (want_fold) {
            HIP_TRY((hipError_t)mi::drank::rank_sort_group(x, plan, dim0, nd, true, W, st, &sorted));
            HIP_TRY((hipError_t)mi::drank::rank_lookup_group(x, plan, dim0, nd, true, MI_RANK_NORMAL, sorted, W, slab, nd, 0, st));
            rc = reduce(slab, h, nd, C2, rt.data() + dim0, nullptr, nullptr);
            if (rc) return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    const double nan = std::nan("");
    for (uint64_t i = 0; i < d; ++i) {
        const bool bad = has_nan[i] != 0;                // a NaN among the retained samples: every output of the dimension is NaN
        if (rhat_bulk) rhat_bulk[i] = bad ? nan : rb[i];
        if (rhat_tail) rhat_tail[i] = bad ? nan : rt[i];
        if (rhat) rhat[i] = (bad || rb[i] != rb[i] || rt[i] != rt[i]) ? nan : (rb[i] > rt[i] ? rb[i] : rt[i]);
        if (ess_bulk) ess_bulk[i] = bad ? nan : eb[i];
        if (ess_tail) ess_tail[i] = bad ? nan : et[i];
    }
    return MI_OK;
}

extern "C" {

int mi_mcmc_draw_stats_ranked(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, double* rhat, double* rhat_bulk,
                              double* rhat_tail, double* ess_bulk, double* ess_tail, void* stream)
{
    return draw_stats_ranked_run("draw_stats_ranked", draws_kdc, mem, n_keep, d, n_chains, rhat, rhat_bulk, rhat_tail, ess_bulk, ess_tail, nullptr, false, stream,
                                 [&](const double* slab, uint64_t h, uint64_t nd, uint64_t C2, double* r, double* e, uint8_t*) {
                                     return mi_mcmc_draw_stats(slab, MI_MEM_DEVICE, h, nd, C2, nullptr, nullptr, r, e, stream);
                                 });
}

// ... with every lag up to max_lag of the half-chains (mi_mcmc_draw_stats_lags, draw_stats.hip)
int mi_mcmc_draw_stats_ranked_lags(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, uint32_t max_lag, double* rhat,
                                   double* rhat_bulk, double* rhat_tail, double* ess_bulk, double* ess_tail, uint8_t* ended, void* stream)
{
    return draw_stats_ranked_run("draw_stats_ranked_lags", draws_kdc, mem, n_keep, d, n_chains, rhat, rhat_bulk, rhat_tail, ess_bulk, ess_tail, ended, true, stream,
                                 [&](const double* slab, uint64_t h, uint64_t nd, uint64_t C2, double* r, double* e, uint8_t* en) {
                                     return mi_mcmc_draw_stats_lags(slab, MI_MEM_DEVICE, h, nd, C2, max_lag, nullptr, nullptr, r, e, en, stream);
                                 });
}

// Rank-normalised nested R-hat: the normal scores of x and of |x - med| (draws_rank.hip, no split: the diagnostic is defined at n_keep = 1) composed
// group by group of dimensions into a slab [n_keep][nd][C], and draws_nested.hip's reducer over it.  Every step is per dimension, so the grouping
// decides memory only.
int mi_mcmc_draw_stats_nested_ranked(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, uint64_t chains_per_super,
                                     double* nrhat, double* nrhat_bulk, double* nrhat_tail, void* stream)
{
    const char* who = "draw_stats_nested_ranked";
    int rc = nested_check(who, draws_kdc, n_keep, d, n_chains, chains_per_super, nrhat || nrhat_bulk || nrhat_tail, "three");
    if (rc) return rc;
    if ((rc = rank_check(who, draws_kdc, n_keep, d, n_chains, 0))) return rc;
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const mi::drank::RankPlan plan = mi::drank::rank_plan(n_keep, d, n_chains, 0, true, g_rank_ws_bytes.load(std::memory_order_relaxed));
    const mi::dnest::NestedPlan nplan = mi::dnest::nested_plan(n_keep, plan.dims_per_group, n_chains, chains_per_super, false);
    DevBuf staged;
    const double* x = nullptr;
    if ((rc = stage_slab(draws_kdc, mem, n_keep, d, n_chains, st, staged, &x))) return rc;
    const size_t o_nested = (plan.bytes + 255) & ~(size_t)255;      // the reducer's workspace behind the rank transform's
    WsLease ws;
    rc = ws_get(st, o_nested + nplan.bytes, ws);
    if (rc) return rc;
    char* W = ws.as<char>();
    double* slab = reinterpret_cast<double*>(W + plan.o_slab);
    const bool want_bulk = nrhat || nrhat_bulk, want_fold = nrhat || nrhat_tail;
    std::vector<double> bw_bulk(3 * d), bw_fold(3 * d), os, q;      // per group [3][nd] at 3 * dim0: mean, between, within of the composed slab
    for (uint64_t dim0 = 0; dim0 < d; dim0 += plan.dims_per_group) {
        const uint64_t nd = std::min<uint64_t>(plan.dims_per_group, d - dim0);
        const mi::dnest::NestedPlan gp = mi::dnest::nested_plan(n_keep, nd, n_chains, chains_per_super, false);      // within nplan.bytes: nd <= dims_per_group
        const uint64_t* sorted = nullptr;
        HIP_TRY((hipError_t)mi::drank::rank_sort_group(x, plan, dim0, nd, false, W, st, &sorted));
        if (want_bulk) {
            HIP_TRY((hipError_t)mi::drank::rank_lookup_group(x, plan, dim0, nd, false, MI_RANK_NORMAL, sorted, W, slab, nd, 0, st));
            HIP_TRY((hipError_t)mi::dnest::nested_run(slab, gp, W + o_nested, false, st));
            HIP_TRY(hipMemcpyAsync(bw_bulk.data() + 3 * dim0, reinterpret_cast<double*>(W + o_nested) + gp.o_out, 3 * nd * 8, hipMemcpyDeviceToHost, st));
        }
        if (want_fold) {                                 // the medians out of the un-folded image, then the sort of |x - med|
            rc = rank_group_quantiles(plan, dim0, nd, sorted, false, W, st, os, q, nullptr);
            if (rc) return rc;
            HIP_TRY((hipError_t)mi::drank::rank_sort_group(x, plan, dim0, nd, true, W, st, &sorted));
            HIP_TRY((hipError_t)mi::drank::rank_lookup_group(x, plan, dim0, nd, true, MI_RANK_NORMAL, sorted, W, slab, nd, 0, st));
            HIP_TRY((hipError_t)mi::dnest::nested_run(slab, gp, W + o_nested, false, st));
            HIP_TRY(hipMemcpyAsync(bw_fold.data() + 3 * dim0, reinterpret_cast<double*>(W + o_nested) + gp.o_out, 3 * nd * 8, hipMemcpyDeviceToHost, st));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    const double nan = std::nan("");
    for (uint64_t dim0 = 0; dim0 < d; dim0 += plan.dims_per_group) {
        const uint64_t nd = std::min<uint64_t>(plan.dims_per_group, d - dim0);
        for (uint64_t j = 0; j < nd; ++j) {
            const double* gb = bw_bulk.data() + 3 * dim0;
            const double* gf = bw_fold.data() + 3 * dim0;
            const double rb = want_bulk ? nested_rhat(gb[nd + j], gb[2 * nd + j]) : 0.0;
            const double rt = want_fold ? nested_rhat(gf[nd + j], gf[2 * nd + j]) : 0.0;
            if (nrhat_bulk) nrhat_bulk[dim0 + j] = rb;
            if (nrhat_tail) nrhat_tail[dim0 + j] = rt;
            if (nrhat) nrhat[dim0 + j] = (rb != rb || rt != rt) ? nan : (rb > rt ? rb : rt);
        }
    }
    return MI_OK;
}

int mi_mcmc_norm_ppf(const double* p, uint64_t n, double* z)
{
    if (n && (!p || !z)) return fail(MI_ERR_BAD_ARG, "norm_ppf: null array");
    for (uint64_t k = 0; k < n; ++k) z[k] = mi::norm_ppf(p[k]);
    return MI_OK;
}

// The checks that mi_mcmc_draws_log_kernel, mi_mcmc_draws_waic, mi_mcmc_draws_psis_loo and mi_mcmc_draws_predict share, in the order in which a call that fails several reports them; they need no
// device.  nothing_asked: NULL, or what to say of the call's outputs; the call needs at least min_K samples.  The two targets that carry
// observations are checked here (logistic_y_optional: a logistic target may come without y -- mi_mcmc_draws_predict at new covariates); what an entry
// point makes of the other kinds is its own, after this
static int target_slab_check(const char* who, const mi_target* t, const double* draws_kdc, uint64_t n_keep, uint64_t n_chains, const char* nothing_asked,
                             uint64_t min_K, uint64_t max_d, bool logistic_y_optional = false)
{
    if (!t) return fail(MI_ERR_BAD_ARG, "%s: null target", who);
    if (!draws_kdc) return fail(MI_ERR_BAD_ARG, "%s: null slab", who);
    if (nothing_asked) return fail(MI_ERR_BAD_ARG, "%s: %s", who, nothing_asked);
    if (t->struct_size != sizeof(mi_target)) return fail(MI_ERR_BAD_ARG, "%s: struct_size mismatch (header / library version skew)", who);
    if (t->d == 0) return fail(MI_ERR_BAD_ARG, "%s: d must be positive", who);
    if (n_keep > 0xffffffffULL || n_chains > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: n_keep / n_chains do not fit 32 bits", who);
    if (n_keep * n_chains < min_K) {
        char need[48];
        if (min_K == 1) std::snprintf(need, sizeof need, "1 sample is");
        else std::snprintf(need, sizeof need, "%llu samples are", (unsigned long long)min_K);
        return fail(MI_ERR_BAD_ARG, "%s: K = n_keep * n_chains = %llu, at least %s needed", who, (unsigned long long)(n_keep * n_chains), need);
    }
    if (t->d > max_d) return fail(MI_ERR_BAD_ARG, "%s: d = %llu is beyond %llu", who, (unsigned long long)t->d, (unsigned long long)max_d);
    if (t->kind == MI_TARGET_LOGISTIC && logistic_y_optional) {
        if (!t->X || t->n_rows == 0) return fail(MI_ERR_BAD_ARG, "%s: the logistic target needs X and n_rows > 0", who);
    } else if (t->kind == MI_TARGET_LOGISTIC && (!t->X || !t->y || t->n_rows == 0)) return fail(MI_ERR_BAD_ARG, "%s: the logistic target needs X, y and n_rows > 0", who);
    if (t->kind == MI_TARGET_NORMAL_MODEL) {
        if (t->d != 2) return fail(MI_ERR_BAD_ARG, "%s: MI_TARGET_NORMAL_MODEL has d = 2 (mu, sigma), not %llu", who, (unsigned long long)t->d);
        if (!t->y || t->n_rows == 0) return fail(MI_ERR_BAD_ARG, "%s: MI_TARGET_NORMAL_MODEL needs its observations in y and n_rows > 0", who);
    }
    return MI_OK;
}

// What the two calls stage into the workspace W of their plan (its areas o_mat, o_y, o_slab): the arrays of a host target (mat_doubles of mat -- prec or
// X --, y_doubles of y) and a host slab, the copies enqueued on st.  *x, *mat, *y: the caller's pointers on entry, the device's on return
static int stage_target_slab(char* W, size_t o_mat, size_t o_y, size_t o_slab, size_t mat_doubles, size_t y_doubles, bool target_host, bool slab_host, size_t slab_doubles,
                             hipStream_t st, const double** x, const double** mat, const double** y)
{
    if (target_host && mat_doubles) { HIP_TRY(hipMemcpyAsync(W + o_mat, *mat, mat_doubles * 8, hipMemcpyHostToDevice, st)); *mat = reinterpret_cast<const double*>(W + o_mat); }
    if (target_host && y_doubles) { HIP_TRY(hipMemcpyAsync(W + o_y, *y, y_doubles * 8, hipMemcpyHostToDevice, st)); *y = reinterpret_cast<const double*>(W + o_y); }
    if (slab_host) { HIP_TRY(hipMemcpyAsync(W + o_slab, *x, slab_doubles * 8, hipMemcpyHostToDevice, st)); *x = reinterpret_cast<const double*>(W + o_slab); }
    return MI_OK;
}

// out[t][c] = log K(x[t][:][c]) of every column of a slab [n_keep][d][C] (draws_logk.hip; the arithmetic: include/mi_mcmc.h).  The slab and the
// target's arrays are staged into the workspace by the plan, not by stage_slab.
int mi_mcmc_draws_log_kernel(const mi_target* target, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t n_chains, double* out, void* stream)
{
    const char* who = "draws_log_kernel";
    int rc = target_slab_check(who, target, draws_kdc, n_keep, n_chains, out ? nullptr : "out is NULL", 1, mi::dlogk::LOGK_MAX_D);
    if (rc) return rc;
    switch (target->kind) {
    case MI_TARGET_GAUSS_ISO: case MI_TARGET_LOGISTIC: case MI_TARGET_NORMAL_MODEL: break;
    case MI_TARGET_GAUSS_DIAG:
    case MI_TARGET_GAUSS_DENSE:
        if (!target->prec) return fail(MI_ERR_BAD_ARG, "%s: target.prec is NULL", who);
        break;
    case MI_TARGET_GAUSS_MIXTURE:
        return fail(MI_ERR_UNSUPPORTED, "%s: MI_TARGET_GAUSS_MIXTURE is not implemented by this reducer", who);
    default:
        return fail(MI_ERR_BAD_ARG, "%s: unknown target kind %d", who, target->kind);
    }
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t d = target->d, K = n_keep * n_chains;
    // 2^38 columns are 2 TB of results alone: beyond any device, and what keeps the grid and every byte count below inside their types
    const bool has_rows = target->kind == MI_TARGET_LOGISTIC || target->kind == MI_TARGET_NORMAL_MODEL;
    if (K > (1ULL << 38) || (has_rows && target->n_rows > (1ULL << 38))) return fail(MI_ERR_OOM, "%s: K = %llu columns / n_rows = %llu do not fit the device memory", who, (unsigned long long)K, (unsigned long long)target->n_rows);
    const bool slab_host = mem == MI_MEM_HOST, target_host = target->mem == MI_MEM_HOST;
    const mi::dlogk::LogkPlan plan = mi::dlogk::logk_plan(target->kind, d, target->n_rows, n_keep, n_chains, slab_host, target_host);
    WsLease ws;
    rc = ws_get(st, plan.bytes, ws);
    if (rc) return rc;
    char* W = ws.as<char>();
    const double *x = draws_kdc, *mat = target->kind == MI_TARGET_LOGISTIC ? target->X : target->prec, *y = target->y;
    if ((rc = stage_target_slab(W, plan.o_mat, plan.o_y, plan.o_slab, plan.mat_doubles, plan.y_doubles, target_host, slab_host, K * d, st, &x, &mat, &y))) return rc;
    double* o = slab_host ? reinterpret_cast<double*>(W + plan.o_out) : out;
    HIP_TRY((hipError_t)mi::dlogk::logk_run(plan, x, mat, y, W, o, st));
    if (slab_host) {
        HIP_TRY(hipMemcpyAsync(out, o, K * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));               // blocking: out is the caller's host array
    } else if (target_host) {
        HIP_TRY(hipStreamSynchronize(st));               // the caller's host arrays of the target have been read when the call returns
    }
    return MI_OK;
}

// {elpd_waic, p_waic, lppd, se_elpd} of the rows' values (include/mi_mcmc.h; this file is compiled with -ffp-contract=off: nothing is fused)
static void waic_summary(const double* lppd, const double* pw, uint64_t n_rows, double* summary)
{
    double elpd = 0.0, p = 0.0, l = 0.0;
    for (uint64_t r = 0; r < n_rows; ++r) {
        const double e = lppd[r] - pw[r];
        elpd = elpd + e;
        p = p + pw[r];
        l = l + lppd[r];
    }
    const double m = elpd / (double)n_rows;
    double v = 0.0;
    for (uint64_t r = 0; r < n_rows; ++r) {
        const double e = lppd[r] - pw[r];
        const double dv = e - m;
        const double sq = dv * dv;
        v = v + sq;
    }
    const double var = v / (double)(n_rows - 1);          // n_rows = 1: 0 / 0, NaN
    const double nv = (double)n_rows * var;
    summary[0] = elpd; summary[1] = p; summary[2] = l; summary[3] = std::sqrt(nv);
}

void mi_mcmc_test_waic_plan(int32_t kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, int slab_host, int target_host, int want_loglik, uint64_t* out10)
{
    const mi::dwaic::WaicPlan p = mi::dwaic::waic_plan(kind, d, n_rows, n_keep, n_chains, slab_host != 0, target_host != 0, want_loglik != 0);
    out10[0] = (uint64_t)p.route; out10[1] = mi::dwaic::WAIC_CHUNK; out10[2] = p.n_chunks; out10[3] = p.grid; out10[4] = p.block;
    out10[5] = p.lds_bytes; out10[6] = p.ldR; out10[7] = p.Kp; out10[8] = p.merge_grid; out10[9] = p.bytes;
}

// Pointwise log-likelihood, lppd and p_waic per data row of a slab [n_keep][d][C], and the WAIC summary (draws_waic.hip; the arithmetic: include/mi_mcmc.h).
// The slab and the target's arrays are staged into the workspace by the plan, as mi_mcmc_draws_log_kernel stages them.
int mi_mcmc_draws_waic(const mi_target* target, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t n_chains, double* lppd_out, double* p_waic_out,
                       double* loglik_out, double* summary, void* stream)
{
    const char* who = "draws_waic";
    const bool any_out = lppd_out || p_waic_out || loglik_out || summary;
    int rc = target_slab_check(who, target, draws_kdc, n_keep, n_chains, any_out ? nullptr : "lppd_out, p_waic_out, loglik_out and summary are all NULL, nothing is asked for",
                               2, mi::dwaic::WAIC_MAX_D);
    if (rc) return rc;
    switch (target->kind) {
    case MI_TARGET_LOGISTIC: case MI_TARGET_NORMAL_MODEL: break;
    case MI_TARGET_GAUSS_ISO:
    case MI_TARGET_GAUSS_DIAG:
    case MI_TARGET_GAUSS_DENSE:
    case MI_TARGET_GAUSS_MIXTURE:
        return fail(MI_ERR_UNSUPPORTED, "%s: target kind %d has no observations: only MI_TARGET_LOGISTIC and MI_TARGET_NORMAL_MODEL have a pointwise log-likelihood", who, target->kind);
    default:
        return fail(MI_ERR_BAD_ARG, "%s: unknown target kind %d", who, target->kind);
    }
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t d = target->d, K = n_keep * n_chains, n_rows = target->n_rows;
    const bool slab_host = mem == MI_MEM_HOST, target_host = target->mem == MI_MEM_HOST;
    // what keeps the grids and every byte count inside their types: 2^38 columns or rows are beyond any device
    if (K > (1ULL << 38) || n_rows > (1ULL << 38)) return fail(MI_ERR_OOM, "%s: K = %llu columns / n_rows = %llu do not fit the device memory", who, (unsigned long long)K, (unsigned long long)n_rows);
    const mi::dwaic::WaicPlan plan = mi::dwaic::waic_plan(target->kind, d, n_rows, n_keep, n_chains, slab_host, target_host, loglik_out != nullptr);
    if (plan.grid >= (1ULL << 31)) return fail(MI_ERR_OOM, "%s: %llu chunks x %llu rows do not fit the device memory", who, (unsigned long long)plan.n_chunks, (unsigned long long)n_rows);
    WsLease ws;
    rc = ws_get(st, plan.bytes, ws);
    if (rc) return rc;
    char* W = ws.as<char>();
    const double *x = draws_kdc, *mat = target->X, *y = target->y;
    if ((rc = stage_target_slab(W, plan.o_mat, plan.o_y, plan.o_slab, plan.mat_doubles, plan.y_doubles, target_host, slab_host, K * d, st, &x, &mat, &y))) return rc;
    double* ll = (slab_host && loglik_out) ? reinterpret_cast<double*>(W + plan.o_ll) : loglik_out;
    HIP_TRY((hipError_t)mi::dwaic::waic_run(plan, x, mat, y, W, ll, st));
    const hipMemcpyKind back = slab_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (lppd_out) HIP_TRY(hipMemcpyAsync(lppd_out, W + plan.o_lppd, n_rows * 8, back, st));
    if (p_waic_out) HIP_TRY(hipMemcpyAsync(p_waic_out, W + plan.o_pw, n_rows * 8, back, st));
    if (slab_host && loglik_out) HIP_TRY(hipMemcpyAsync(loglik_out, ll, K * n_rows * 8, hipMemcpyDeviceToHost, st));
    if (summary) {
        std::vector<double> lp(n_rows), pw(n_rows);
        HIP_TRY(hipMemcpyAsync(lp.data(), W + plan.o_lppd, n_rows * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pw.data(), W + plan.o_pw, n_rows * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));               // blocking: summary is written on the host
        waic_summary(lp.data(), pw.data(), n_rows, summary);
    } else if (slab_host || target_host) {
        HIP_TRY(hipStreamSynchronize(st));               // the outputs are the caller's host arrays / the target's host arrays have been read
    }
    return MI_OK;
}

// test hooks, declared in mi_mcmc_probes.h: the budget of a row group's block ll and the LDS capacity of the tail of mi_mcmc_draws_psis_loo
// (draws_psis.hpp), and the host arithmetic of its plan under them and under the rank budget above
static std::atomic<uint64_t> g_psis_ll_bytes{0};
static std::atomic<uint32_t> g_psis_lds_tail{0};
void mi_mcmc_test_set_psis_ll_bytes(uint64_t bytes) { g_psis_ll_bytes.store(bytes, std::memory_order_relaxed); }
void mi_mcmc_test_set_psis_lds_tail(uint32_t n_doubles) { g_psis_lds_tail.store(n_doubles, std::memory_order_relaxed); }
static mi::dpsis::PsisPlan psis_plan_now(int32_t kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, bool slab_host, bool target_host)
{
    return mi::dpsis::psis_plan(kind, d, n_rows, n_keep, n_chains, slab_host, target_host, g_psis_ll_bytes.load(std::memory_order_relaxed),
                                g_psis_lds_tail.load(std::memory_order_relaxed), g_rank_ws_bytes.load(std::memory_order_relaxed));
}
void mi_mcmc_test_psis_plan(int32_t kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, int slab_host, int target_host, uint64_t* out12)
{
    const mi::dpsis::PsisPlan p = psis_plan_now(kind, d, n_rows, n_keep, n_chains, slab_host != 0, target_host != 0);
    out12[0] = p.M; out12[1] = p.m; out12[2] = p.G; out12[3] = p.n_groups; out12[4] = n_rows - (p.n_groups - 1) * p.G; out12[5] = (uint64_t)p.tail_route;
    out12[6] = p.lds_bytes; out12[7] = p.n_pieces; out12[8] = mi::dpsis::PSIS_BODY_PIECE; out12[9] = p.rank.dims_per_group; out12[10] = p.o_rank - p.o_ll;
    out12[11] = p.bytes;
}

// {elpd_loo, p_loo, lppd, se_elpd_loo, n_bad} of the rows' values (include/mi_mcmc.h; nothing is fused)
static void psis_summary(const double* elpd, const double* pk, const double* lppd, uint64_t n_rows, double* summary)
{
    double e = 0.0, l = 0.0, bad = 0.0;
    for (uint64_t r = 0; r < n_rows; ++r) {
        e = e + elpd[r];
        l = l + lppd[r];
        if (!(pk[r] <= 0.7)) bad = bad + 1.0;
    }
    const double m = e / (double)n_rows;
    double v = 0.0;
    for (uint64_t r = 0; r < n_rows; ++r) {
        const double dv = elpd[r] - m;
        const double sq = dv * dv;
        v = v + sq;
    }
    const double var = v / (double)(n_rows - 1);          // n_rows = 1: 0 / 0, NaN
    const double nv = (double)n_rows * var;
    summary[0] = e; summary[1] = l - e; summary[2] = l; summary[3] = std::sqrt(nv); summary[4] = bad;
}

// PSIS-LOO and Pareto k per data row of a slab [n_keep][d][C] (draws_psis.hip; the arithmetic: include/mi_mcmc.h).  The rows go in groups: the block ll
// of a group by draws_waic.hip, its rows sorted by draws_rank.hip, the tail fit and the folds by draws_psis.hip.  Always blocking.
int mi_mcmc_draws_psis_loo(const mi_target* target, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t n_chains, double* elpd_loo_out,
                           double* pareto_k_out, double* lppd_out, double* summary, void* stream)
{
    const char* who = "draws_psis_loo";
    const bool any_out = elpd_loo_out || pareto_k_out || lppd_out || summary;
    int rc = target_slab_check(who, target, draws_kdc, n_keep, n_chains,
                               any_out ? nullptr : "elpd_loo_out, pareto_k_out, lppd_out and summary are all NULL, nothing is asked for", mi::dpsis::PSIS_MIN_K,
                               mi::dwaic::WAIC_MAX_D);
    if (rc) return rc;
    if (n_keep * n_chains > 0xffffffffULL)
        return fail(MI_ERR_BAD_ARG, "%s: K = n_keep * n_chains = %llu samples per row, must be below 2^32", who, (unsigned long long)(n_keep * n_chains));
    switch (target->kind) {
    case MI_TARGET_LOGISTIC: case MI_TARGET_NORMAL_MODEL: break;
    case MI_TARGET_GAUSS_ISO:
    case MI_TARGET_GAUSS_DIAG:
    case MI_TARGET_GAUSS_DENSE:
    case MI_TARGET_GAUSS_MIXTURE:
        return fail(MI_ERR_UNSUPPORTED, "%s: target kind %d has no observations: only MI_TARGET_LOGISTIC and MI_TARGET_NORMAL_MODEL have a pointwise log-likelihood", who, target->kind);
    default:
        return fail(MI_ERR_BAD_ARG, "%s: unknown target kind %d", who, target->kind);
    }
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t d = target->d, K = n_keep * n_chains, n_rows = target->n_rows;
    const bool slab_host = mem == MI_MEM_HOST, target_host = target->mem == MI_MEM_HOST;
    if (n_rows > (1ULL << 38)) return fail(MI_ERR_OOM, "%s: n_rows = %llu do not fit the device memory", who, (unsigned long long)n_rows);
    const mi::dpsis::PsisPlan plan = psis_plan_now(target->kind, d, n_rows, n_keep, n_chains, slab_host, target_host);
    if (plan.waic.grid >= (1ULL << 31)) return fail(MI_ERR_OOM, "%s: %llu chunks x %llu rows of a group do not fit the device memory", who, (unsigned long long)plan.waic.n_chunks, (unsigned long long)plan.G);
    WsLease ws;
    rc = ws_get(st, plan.bytes, ws);
    if (rc) return rc;
    char* W = ws.as<char>();
    const double *x = draws_kdc, *mat = target->X, *y = target->y;
    if ((rc = stage_target_slab(W, plan.o_mat, plan.o_y, plan.o_slab, plan.mat_doubles, plan.y_doubles, target_host, slab_host, K * d, st, &x, &mat, &y))) return rc;
    double* const elpd = reinterpret_cast<double*>(W + plan.o_elpd);
    double* const pk = reinterpret_cast<double*>(W + plan.o_k);
    double* const lppd = reinterpret_cast<double*>(W + plan.o_lppd);
    double* const part = reinterpret_cast<double*>(W + plan.o_part);
    double* const ll = reinterpret_cast<double*>(W + plan.o_ll);
    const bool logistic = target->kind == MI_TARGET_LOGISTIC;
    for (uint64_t r0 = 0; r0 < n_rows; r0 += plan.G) {
        const uint64_t g = std::min<uint64_t>(plan.G, n_rows - r0);
        // the sub-target: rows r0 .. r0 + g of the row-major X are contiguous
        const mi::dwaic::WaicPlan wp = g == plan.G ? plan.waic : mi::dwaic::waic_plan(target->kind, d, g, n_keep, n_chains, false, false, true);
        HIP_TRY((hipError_t)mi::dwaic::waic_run(wp, x, logistic ? mat + r0 * d : mat, y + r0, W + plan.o_waic, ll, st));
        HIP_TRY(hipMemcpyAsync(lppd + r0, W + plan.o_waic + wp.o_lppd, g * 8, hipMemcpyDeviceToDevice, st));
        // the block [g][K] is a slab [1][g][K]: every row sorted, in the rank plan's own groups
        for (uint64_t dim0 = 0; dim0 < g; dim0 += plan.rank.dims_per_group) {
            const uint64_t nd = std::min<uint64_t>(plan.rank.dims_per_group, g - dim0);
            const uint64_t* sorted = nullptr;
            HIP_TRY((hipError_t)mi::drank::rank_sort_group(ll, plan.rank, dim0, nd, false, W + plan.o_rank, st, &sorted));
            HIP_TRY((hipError_t)mi::dpsis::psis_run_group(plan, sorted, nd, part, elpd + r0 + dim0, pk + r0 + dim0, st));
        }
    }
    const hipMemcpyKind back = slab_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (elpd_loo_out) HIP_TRY(hipMemcpyAsync(elpd_loo_out, elpd, n_rows * 8, back, st));
    if (pareto_k_out) HIP_TRY(hipMemcpyAsync(pareto_k_out, pk, n_rows * 8, back, st));
    if (lppd_out) HIP_TRY(hipMemcpyAsync(lppd_out, lppd, n_rows * 8, back, st));
    if (summary) {
        std::vector<double> h(3 * n_rows);
        HIP_TRY(hipMemcpyAsync(h.data(), elpd, n_rows * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h.data() + n_rows, pk, n_rows * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h.data() + 2 * n_rows, lppd, n_rows * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        psis_summary(h.data(), h.data() + n_rows, h.data() + 2 * n_rows, n_rows, summary);
    }
    HIP_TRY(hipStreamSynchronize(st));                   // always blocking: the sorts have waited already, and the workspace is read until here
    return MI_OK;
}

// The plan of the two entries below under the hooks of the LDS tail and the rank budget, and its test hook (mi_mcmc_probes.h)
static mi::dloglik::LoglikPlan loglik_plan_now(int32_t layout, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, bool mat_host, bool psis)
{
    return mi::dloglik::loglik_plan(layout, n_rows, n_keep, n_chains, mat_host, psis, g_psis_lds_tail.load(std::memory_order_relaxed),
                                    g_rank_ws_bytes.load(std::memory_order_relaxed));
}
void mi_mcmc_test_loglik_plan(int32_t layout, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, int mat_host, int psis, uint64_t* out8)
{
    const mi::dloglik::LoglikPlan p = loglik_plan_now(layout, n_rows, n_keep, n_chains, mat_host != 0, psis != 0);
    out8[0] = p.n_chunks; out8[1] = p.fold_grid; out8[2] = p.psis.M; out8[3] = p.psis.m; out8[4] = p.psis.rank.dims_per_group; out8[5] = p.psis.rank.n_groups;
    out8[6] = (uint64_t)p.psis.tail_route; out8[7] = p.bytes;
}

// The checks that mi_mcmc_loglik_waic and mi_mcmc_loglik_psis_loo share, in the order in which a call that fails several reports them; they need no device
static int loglik_check(const char* who, const double* loglik, const char* nothing_asked, int32_t layout, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains,
                        uint64_t min_K, bool psis)
{
    if (!loglik) return fail(MI_ERR_BAD_ARG, "%s: null matrix", who);
    if (nothing_asked) return fail(MI_ERR_BAD_ARG, "%s: %s", who, nothing_asked);
    if (layout != MI_LOGLIK_ROWS && layout != MI_LOGLIK_SLAB) return fail(MI_ERR_BAD_ARG, "%s: layout = %d is neither MI_LOGLIK_ROWS nor MI_LOGLIK_SLAB", who, layout);
    if (n_rows == 0) return fail(MI_ERR_BAD_ARG, "%s: n_rows must be positive", who);
    if (n_keep > 0xffffffffULL || n_chains > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: n_keep / n_chains do not fit 32 bits", who);
    if (n_keep * n_chains < min_K)
        return fail(MI_ERR_BAD_ARG, "%s: K = n_keep * n_chains = %llu, at least %llu samples are needed", who, (unsigned long long)(n_keep * n_chains), (unsigned long long)min_K);
    if (psis && n_keep * n_chains > 0xffffffffULL)
        return fail(MI_ERR_BAD_ARG, "%s: K = n_keep * n_chains = %llu samples per row, must be below 2^32", who, (unsigned long long)(n_keep * n_chains));
    if (layout == MI_LOGLIK_SLAB && n_rows > mi::drank::RANK_MAX_D)
        return fail(MI_ERR_BAD_ARG, "%s: MI_LOGLIK_SLAB with n_rows = %llu is beyond %llu", who, (unsigned long long)n_rows, (unsigned long long)mi::drank::RANK_MAX_D);
    return MI_OK;
}

// After the device probe: what does not fit any device (and would leave a byte count or a grid outside its type), the plan, the workspace, a host
// matrix staged into it.  *mat: the caller's pointer on entry, the device's on return
static int loglik_begin(const char* who, int32_t layout, int32_t mem, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, bool psis, hipStream_t st,
                        mi::dloglik::LoglikPlan& plan, WsLease& ws, const double** mat)
{
    const uint64_t K = n_keep * n_chains;
    if (K > (1ULL << 38) || n_rows > (1ULL << 38) || n_rows > mi::dloglik::LOGLIK_MAX_ELEMS / K)
        return fail(MI_ERR_OOM, "%s: K = %llu columns x n_rows = %llu do not fit the device memory", who, (unsigned long long)K, (unsigned long long)n_rows);
    const bool mat_host = mem == MI_MEM_HOST;
    plan = loglik_plan_now(layout, n_rows, n_keep, n_chains, mat_host, psis);
    if (plan.fold_grid >= (1ULL << 31)) return fail(MI_ERR_OOM, "%s: %llu chunks x %llu rows do not fit the device memory", who, (unsigned long long)plan.n_chunks, (unsigned long long)n_rows);
    int rc = ws_get(st, plan.bytes, ws);
    if (rc) return rc;
    if (mat_host) {
        char* W = ws.as<char>();
        HIP_TRY(hipMemcpyAsync(W + plan.o_mat, *mat, n_rows * K * 8, hipMemcpyHostToDevice, st));
        *mat = reinterpret_cast<const double*>(W + plan.o_mat);
    }
    return MI_OK;
}

// lppd, p_waic and the WAIC summary of a caller-supplied matrix ll (draws_loglik.hip; the order: mi_mcmc_draws_waic's in include/mi_mcmc.h)
int mi_mcmc_loglik_waic(const double* loglik, int32_t layout, int32_t mem, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, double* lppd_out, double* p_waic_out,
                        double* summary, void* stream)
{
    const char* who = "loglik_waic";
    const bool any_out = lppd_out || p_waic_out || summary;
    int rc = loglik_check(who, loglik, any_out ? nullptr : "lppd_out, p_waic_out and summary are all NULL, nothing is asked for", layout, n_rows, n_keep, n_chains, 2, false);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    mi::dloglik::LoglikPlan plan;
    WsLease ws;
    const double* mat = loglik;
    if ((rc = loglik_begin(who, layout, mem, n_rows, n_keep, n_chains, false, st, plan, ws, &mat))) return rc;
    char* W = ws.as<char>();
    HIP_TRY((hipError_t)mi::dloglik::loglik_fold(plan, mat, W, st));
    const bool mat_host = mem == MI_MEM_HOST;
    const hipMemcpyKind back = mat_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (lppd_out) HIP_TRY(hipMemcpyAsync(lppd_out, W + plan.o_lppd, n_rows * 8, back, st));
    if (p_waic_out) HIP_TRY(hipMemcpyAsync(p_waic_out, W + plan.o_pw, n_rows * 8, back, st));
    if (summary) {
        std::vector<double> lp(n_rows), pw(n_rows);
        HIP_TRY(hipMemcpyAsync(lp.data(), W + plan.o_lppd, n_rows * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pw.data(), W + plan.o_pw, n_rows * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));               // blocking: summary is written on the host
        waic_summary(lp.data(), pw.data(), n_rows, summary);
    } else if (mat_host) {
        HIP_TRY(hipStreamSynchronize(st));               // the matrix and the outputs are the caller's host arrays
    }
    return MI_OK;
}

// PSIS-LOO and Pareto k of a caller-supplied matrix ll: the matrix is the slab the sorter takes (draws_loglik.hip, draws_rank.hip, draws_psis.hip; the
// arithmetic: mi_mcmc_draws_psis_loo's in include/mi_mcmc.h).  Always blocking.
int mi_mcmc_loglik_psis_loo(const double* loglik, int32_t layout, int32_t mem, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, double* elpd_loo_out,
                            double* pareto_k_out, double* lppd_out, double* summary, void* stream)
{
    const char* who = "loglik_psis_loo";
    const bool any_out = elpd_loo_out || pareto_k_out || lppd_out || summary;
    int rc = loglik_check(who, loglik, any_out ? nullptr : "elpd_loo_out, pareto_k_out, lppd_out and summary are all NULL, nothing is asked for", layout, n_rows, n_keep,
                          n_chains, mi::dpsis::PSIS_MIN_K, true);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    mi::dloglik::LoglikPlan plan;
    WsLease ws;
    const double* mat = loglik;
    if ((rc = loglik_begin(who, layout, mem, n_rows, n_keep, n_chains, true, st, plan, ws, &mat))) return rc;
    char* W = ws.as<char>();
    if (lppd_out || summary) HIP_TRY((hipError_t)mi::dloglik::loglik_fold(plan, mat, W, st));
    HIP_TRY((hipError_t)mi::dloglik::loglik_psis(plan, mat, W, st));
    const hipMemcpyKind back = mem == MI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (elpd_loo_out) HIP_TRY(hipMemcpyAsync(elpd_loo_out, W + plan.o_elpd, n_rows * 8, back, st));
    if (pareto_k_out) HIP_TRY(hipMemcpyAsync(pareto_k_out, W + plan.o_k, n_rows * 8, back, st));
    if (lppd_out) HIP_TRY(hipMemcpyAsync(lppd_out, W + plan.o_lppd, n_rows * 8, back, st));
    if (summary) {
        std::vector<double> h(3 * n_rows);
        HIP_TRY(hipMemcpyAsync(h.data(), W + plan.o_elpd, n_rows * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h.data() + n_rows, W + plan.o_k, n_rows * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h.data() + 2 * n_rows, W + plan.o_lppd, n_rows * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        psis_summary(h.data(), h.data() + n_rows, h.data() + 2 * n_rows, n_rows, summary);
    }
    HIP_TRY(hipStreamSynchronize(st));                   // always blocking: the sorts have waited already, and the workspace is read until here
    return MI_OK;
}

// ---- bridge sampling (draws_bridge.hip; the arithmetic: include/mi_mcmc.h) ----
// test hook, declared in mi_mcmc_probes.h: the budget of one group of proposal columns
static std::atomic<uint64_t> g_bridge_prop_bytes{0};
void mi_mcmc_test_set_bridge_prop_bytes(uint64_t bytes) { g_bridge_prop_bytes.store(bytes, std::memory_order_relaxed); }

extern "C++" {
namespace {

using mi::dprod::align256;
const double BRIDGE_NAN = std::nan("");

// steps A and B of mi_mcmc_bridge_proposal, on the host once the pooled moments are back
struct BridgeFit {
    std::vector<double> mu, S, L, Pg;
    double ldh = 0.0;
    int status = 0;
};

bool all_finite(const std::vector<double>& v)
{
    for (double x : v)
        if (!std::isfinite(x)) return false;
    return true;
}

// (mu, S) of the prefix slab [n_fit][d][C] by the covariance reducer under a lease of its own (the routines of INV / CHOL_LOWER may use the device), then B
int bridge_fit(const double* x, uint64_t n_fit, uint64_t d, uint64_t C, hipStream_t st, BridgeFit& f)
try {
    f.mu.assign(d, 0.0);
    f.S.assign(d * d, 0.0);
    {
        const mi::dcov::CovPlan plan = mi::dcov::cov_plan(n_fit, d, C, true);
        WsLease ws;
        int rc = ws_get(st, plan.bytes, ws);
        if (rc) return rc;
        HIP_TRY((hipError_t)mi::dcov::cov_run(x, d, C, plan, ws.p, true, st));
        HIP_TRY(hipMemcpyAsync(f.mu.data(), ws.as<double>() + plan.o_mean, d * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(f.S.data(), ws.as<double>() + plan.o_cov, d * d * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    f.status = 1;
    f.ldh = BRIDGE_NAN;
    if (!all_finite(f.S)) return MI_OK;
    f.L.assign(d * d, 0.0);
    f.Pg.assign(d * d, 0.0);
    int rc = mi_mcmc_mat_cholesky_lower(f.S.data(), d, f.L.data());
    if (rc) return rc;
    if ((rc = mi_mcmc_mat_inverse(f.S.data(), d, f.Pg.data()))) return rc;
    if (!all_finite(f.L) || !all_finite(f.Pg)) return MI_OK;
    double s = 0.0;
    for (uint64_t a = 0; a < d; ++a) {
        const double laa = f.L[a * d + a];
        if (!(laa > 0.0)) return MI_OK;
        s = s + mi::det_log(laa);
    }
    for (uint64_t a = 0; a < d; ++a)                   // the chain over b = 0 .. a: what lies above the diagonal is zero
        for (uint64_t b = a + 1; b < d; ++b) f.L[a * d + b] = 0.0;
    const double half_d = 0.5 * (double)d;
    const double c = half_d * mi::dprod::LOG_2PI;
    f.ldh = s + c;
    f.status = 0;
    return MI_OK;
} catch (const std::bad_alloc&) {                      // S, L and Pg are d x d doubles each on the host
    return fail(MI_ERR_OOM, "bridge sampling: the host has no memory for the %llu x %llu matrices of the fit", (unsigned long long)d, (unsigned long long)d);
}

// The workspace of steps C and D: the two packed matrices, mu, one d x d upload area, and the block of proposal columns ([d][N2] where the caller wants
// prop_out, else one group)
struct BridgePropWs {
    mi::dbridge::MatPlan mp;
    uint64_t g = 0;                                    // columns of a group
    size_t o_packL = 0, o_packP = 0, o_mu = 0, o_tmp = 0, o_y = 0, bytes = 0;
};
BridgePropWs bridge_prop_ws(uint64_t d, uint64_t N2, bool whole, bool y_in_ws)
{
    BridgePropWs w;
    w.mp = mi::dbridge::mat_plan(d);
    w.g = whole ? N2 : std::min<uint64_t>(N2, mi::dbridge::group_cols(d, N2, g_bridge_prop_bytes.load(std::memory_order_relaxed)));
    w.o_packL = 0;
    w.o_packP = w.o_packL + w.mp.pack_bytes;
    w.o_mu = w.o_packP + w.mp.pack_bytes;
    w.o_tmp = w.o_mu + align256(d * 8);
    w.o_y = w.o_tmp + align256(d * d * 8);
    w.bytes = w.o_y + (y_in_ws ? align256((size_t)d * w.g * 8) : 0);
    return w;
}

// Steps C and D of a fit with status 0, enqueued on st.  suffix: the iteration part [n_it][d][C]; y_whole: where the whole block [d][N2] goes (the caller's
// prop_out or its staged image), or NULL: groups in the workspace.  logg_post / logg_prop (device, may be NULL).  per_group(y, col0, g): what else
// consumes a group, a slab [1][d][g] (may be empty)
template <class F>
int bridge_prop_device(const BridgeFit& f, const double* suffix, uint64_t n_it, uint64_t d, uint64_t C, uint64_t N2, uint64_t seed, char* W, const BridgePropWs& w,
                       double* y_whole, double* logg_post, double* logg_prop, F per_group, hipStream_t st)
{
    double* const packL = reinterpret_cast<double*>(W + w.o_packL);
    double* const packP = reinterpret_cast<double*>(W + w.o_packP);
    double* const mu = reinterpret_cast<double*>(W + w.o_mu);
    double* const tmp = reinterpret_cast<double*>(W + w.o_tmp);
    HIP_TRY(hipMemcpyAsync(mu, f.mu.data(), d * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(tmp, f.L.data(), d * d * 8, hipMemcpyHostToDevice, st));
    HIP_TRY((hipError_t)mi::dbridge::pack_run(w.mp, tmp, packL, st));
    HIP_TRY(hipMemcpyAsync(tmp, f.Pg.data(), d * d * 8, hipMemcpyHostToDevice, st));
    HIP_TRY((hipError_t)mi::dbridge::pack_run(w.mp, tmp, packP, st));
    mi::host::last_kernel() = "bridge_propose_kernel, bridge_logg_kernel";
    if (logg_post) HIP_TRY((hipError_t)mi::dbridge::logg_run(w.mp, packP, mu, f.ldh, suffix, n_it, C, logg_post, st));
    for (uint64_t col0 = 0; col0 < N2; col0 += w.g) {
        const uint64_t g = std::min<uint64_t>(w.g, N2 - col0);
        double* const y = y_whole ? y_whole : reinterpret_cast<double*>(W + w.o_y);      // (y_whole: one group, g = N2)
        HIP_TRY((hipError_t)mi::dbridge::propose_run(w.mp, packL, mu, seed, col0, g, g, y, st));
        if (logg_prop) HIP_TRY((hipError_t)mi::dbridge::logg_run(w.mp, packP, mu, f.ldh, y, 1, g, logg_prop + col0, st));
        const int rc = per_group(y, col0, g);
        if (rc) return rc;
    }
    return MI_OK;
}

// The checks the two slab entries of bridge sampling share; they need no device.  *n_fit, *N2: 0 on entry is the default
int bridge_shape_check(const char* who, uint64_t n_keep, uint64_t d, uint64_t n_chains, uint64_t* n_fit, uint64_t* N2)
{
    if (d == 0) return fail(MI_ERR_BAD_ARG, "%s: d must be positive", who);
    if (d > mi::dbridge::BRIDGE_MAX_D) return fail(MI_ERR_BAD_ARG, "%s: d = %llu is beyond %llu", who, (unsigned long long)d, (unsigned long long)mi::dbridge::BRIDGE_MAX_D);
    if (n_keep > 0xffffffffULL || n_chains > 0xffffffffULL || *N2 > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: n_keep / n_chains / n_prop do not fit 32 bits", who);
    if (n_keep < 2) return fail(MI_ERR_BAD_ARG, "%s: n_keep = %llu, at least 2 draws are needed (a fit part and an iteration part)", who, (unsigned long long)n_keep);
    if (*n_fit == 0) *n_fit = n_keep / 2;
    if (*n_fit >= n_keep) return fail(MI_ERR_BAD_ARG, "%s: n_fit = %llu is not below n_keep = %llu", who, (unsigned long long)*n_fit, (unsigned long long)n_keep);
    const uint64_t K0 = *n_fit * n_chains, N1 = (n_keep - *n_fit) * n_chains;
    if (K0 < 2 || N1 < 2) return fail(MI_ERR_BAD_ARG, "%s: K0 = %llu fit samples, N1 = %llu iteration samples: at least 2 of each are needed", who, (unsigned long long)K0, (unsigned long long)N1);
    if (N1 > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: N1 = %llu iteration samples, must be below 2^32", who, (unsigned long long)N1);
    if (*N2 == 0) *N2 = N1;
    if (*N2 < 2) return fail(MI_ERR_BAD_ARG, "%s: n_prop = %llu, at least 2 proposal draws are needed", who, (unsigned long long)*N2);
    return MI_OK;
}

int bridge_param_check(const char* who, double n_eff, double tol)
{
    if (!(tol >= 0.0)) return fail(MI_ERR_BAD_ARG, "%s: tol = %g is negative or NaN", who, tol);
    if (!(n_eff >= 0.0)) return fail(MI_ERR_BAD_ARG, "%s: n_eff = %g is negative or NaN", who, n_eff);
    return MI_OK;
}

// The workspace of the estimate: l1 -> b [N1], l2 -> a [N2], the selection's own, the pieces' sums, the chunks' (shift, S1, S2)
struct BridgeEstWs {
    mi::dsel::SelPlan sel;
    size_t o_b = 0, o_a = 0, o_sel = 0, o_part = 0, o_stat = 0, bytes = 0;
};
BridgeEstWs bridge_est_ws(uint64_t n_it, uint64_t C, uint64_t N2)
{
    BridgeEstWs w;
    const uint64_t N1 = n_it * C;
    w.sel = mi::dsel::sel_plan(n_it, 1, C, 2);
    w.o_b = 0;
    w.o_a = w.o_b + align256(N1 * 8);
    w.o_sel = w.o_a + align256(N2 * 8);
    w.o_part = w.o_sel + align256(w.sel.bytes);
    w.o_stat = w.o_part + align256((mi::dbridge::n_pieces(N1) + mi::dbridge::n_pieces(N2)) * 8);
    w.bytes = w.o_stat + align256((mi::dbridge::n_chunks(N1) + mi::dbridge::n_chunks(N2)) * 24);
    return w;
}

// (mean, M2) of n values from their chunks' (shift, S1, S2): the chunk moments and the merge of mi_mcmc_draws_waic (nothing is fused)
void bridge_merge(const double* stat, uint64_t n, double* mean_out, double* M2_out)
{
    double cnt = 0.0, mean = 0.0, M2 = 0.0;
    const uint64_t Q = mi::dbridge::n_chunks(n);
    for (uint64_t b = 0; b < Q; ++b) {
        const double nb = (double)std::min<uint64_t>(mi::dbridge::BRIDGE_CHUNK, n - b * mi::dbridge::BRIDGE_CHUNK);
        const double sh = stat[3 * b], S1 = stat[3 * b + 1], S2 = stat[3 * b + 2];
        const double q1 = S1 / nb;
        const double mb = sh + q1;
        const double sq = S1 * S1;
        const double q2 = sq / nb;
        const double M2b = S2 - q2;
        if (b == 0) { cnt = nb; mean = mb; M2 = M2b; continue; }
        const double delta = mb - mean;
        const double nn = cnt + nb;
        const double wgt = nb / nn;
        const double step = delta * wgt;
        mean = mean + step;
        const double both = M2 + M2b;
        const double d2 = delta * delta;
        const double prod = cnt * nb;
        const double frac = prod / nn;
        const double corr = d2 * frac;
        M2 = both + corr;
        cnt = nn;
    }
    *mean_out = mean;
    *M2_out = M2;
}

// The estimate from four device arrays; f2 (device, may be NULL); summary: 8 doubles on the host.  Blocks: the iteration lives on the host
int bridge_estimate_device(const double* lp1, const double* lg1, const double* lp2, const double* lg2, uint64_t n_it, uint64_t C, uint64_t N2, double n_eff, double tol,
                           uint64_t max_iter, char* W, const BridgeEstWs& w, double* f2, double* summary, hipStream_t st)
{
    const uint64_t N1 = n_it * C;
    double* const b = reinterpret_cast<double*>(W + w.o_b);
    double* const a = reinterpret_cast<double*>(W + w.o_a);
    double* const part = reinterpret_cast<double*>(W + w.o_part);
    double* const stat = reinterpret_cast<double*>(W + w.o_stat);
    if (n_eff == 0.0) n_eff = (double)N1;
    if (tol == 0.0) tol = 1e-10;
    if (max_iter == 0) max_iter = 1000;
    mi::host::last_kernel() = "bridge_pieces_kernel, bridge_moments_kernel";
    HIP_TRY((hipError_t)mi::dbridge::diff_run(lp1, lg1, N1, b, st));
    HIP_TRY((hipError_t)mi::dbridge::diff_run(lp2, lg2, N2, a, st));
    // l*: the two order statistics of the type-7 median of the slab [n_it][1][C]
    mi::dsel::SelRanks ranks{};
    double g = 0.0, os[2];
    type7_ranks(N1, 0.5, &ranks.r[0], &ranks.r[1], &g);
    HIP_TRY((hipError_t)mi::dsel::sel_run(b, n_it, 1, C, ranks, 2, w.sel, W + w.o_sel, st));
    HIP_TRY(hipMemcpyAsync(os, W + w.o_sel + w.sel.o_out, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const double lstar = type7_value(os[0], os[1], g);
    HIP_TRY((hipError_t)mi::dbridge::exp_shift_run(b, N1, lstar, st));
    HIP_TRY((hipError_t)mi::dbridge::exp_shift_run(a, N2, lstar, st));
    const double n2 = (double)N2, n1 = (double)N1;
    const double tot = n_eff + n2;
    const double s1 = n_eff / tot, s2 = n2 / tot;
    const uint64_t P2 = mi::dbridge::n_pieces(N2), P1 = mi::dbridge::n_pieces(N1);
    std::vector<double> ph(P2 + P1);
    double r = 1.0, rel = BRIDGE_NAN;
    uint64_t it = 0;
    int status = 0;
    for (;;) {
        HIP_TRY((hipError_t)mi::dbridge::pieces_run(a, N2, b, N1, s1, s2, r, part, st));
        HIP_TRY(hipMemcpyAsync(ph.data(), part, ph.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        double sa = 0.0, sb = 0.0;
        for (uint64_t p = 0; p < P2; ++p) sa = sa + ph[p];
        for (uint64_t p = 0; p < P1; ++p) sb = sb + ph[P2 + p];
        const double num = sa / n2, den = sb / n1;
        const double rn = num / den;
        ++it;
        const double diff = rn - r;
        rel = std::fabs(diff) / std::fabs(rn);
        r = rn;
        if (!(std::isfinite(r) && r > 0.0)) { status = 3; break; }
        if (rel <= tol) { status = 0; break; }
        if (it == max_iter) { status = 2; break; }
    }
    HIP_TRY((hipError_t)mi::dbridge::moments_run(a, N2, b, N1, s1, s2, r, stat, f2, st));
    const uint64_t Q2 = mi::dbridge::n_chunks(N2), Q1 = mi::dbridge::n_chunks(N1);
    std::vector<double> sh((Q2 + Q1) * 3);
    HIP_TRY(hipMemcpyAsync(sh.data(), stat, sh.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double m1, M21, m2, M22;
    bridge_merge(sh.data(), N2, &m1, &M21);
    bridge_merge(sh.data() + 3 * Q2, N1, &m2, &M22);
    const double v1 = M21 / (double)(N2 - 1), v2 = M22 / (double)(N1 - 1);
    const double mm1 = m1 * m1, mm2 = m2 * m2;
    const double d1 = mm1 * n2, d2 = mm2 * n1;
    if (summary) {
        summary[0] = mi::det_log(r) + lstar;
        summary[1] = (double)status; summary[2] = (double)it; summary[3] = rel; summary[4] = lstar;
        summary[5] = v1 / d1; summary[6] = v2 / d2; summary[7] = n2;
    }
    return MI_OK;
}

}  // namespace
}  // extern "C++"

int mi_mcmc_bridge_proposal(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, uint64_t n_fit, uint64_t n_prop, uint64_t seed,
                            double* prop_out, double* logg_post_out, double* logg_prop_out, double* mean_out, double* cov_out, double* info, void* stream)
{
    const char* who = "bridge_proposal";
    if (!draws_kdc) return fail(MI_ERR_BAD_ARG, "%s: null slab", who);
    if (!prop_out && !logg_post_out && !logg_prop_out && !mean_out && !cov_out && !info) return fail(MI_ERR_BAD_ARG, "%s: all six outputs are NULL, nothing is asked for", who);
    uint64_t N2 = n_prop;
    int rc = bridge_shape_check(who, n_keep, d, n_chains, &n_fit, &N2);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t C = n_chains, n_it = n_keep - n_fit, N1 = n_it * C;
    const bool host = mem == MI_MEM_HOST;
    DevBuf staged;
    const double* x = nullptr;
    if ((rc = stage_slab(draws_kdc, mem, n_keep, d, C, st, staged, &x))) return rc;
    BridgeFit f;
    if ((rc = bridge_fit(x, n_fit, d, C, st, f))) return rc;
    const bool ok = f.status == 0;
    if (mean_out) for (uint64_t a = 0; a < d; ++a) mean_out[a] = ok ? f.mu[a] : BRIDGE_NAN;
    if (cov_out) for (uint64_t a = 0; a < d * d; ++a) cov_out[a] = ok ? f.S[a] : BRIDGE_NAN;
    if (info) { info[0] = (double)f.status; info[1] = f.ldh; }
    if (!prop_out && !logg_post_out && !logg_prop_out) { HIP_TRY(hipStreamSynchronize(st)); return MI_OK; }
    if (!ok) {
        if (host) {
            if (prop_out) std::fill(prop_out, prop_out + d * N2, BRIDGE_NAN);
            if (logg_post_out) std::fill(logg_post_out, logg_post_out + N1, BRIDGE_NAN);
            if (logg_prop_out) std::fill(logg_prop_out, logg_prop_out + N2, BRIDGE_NAN);
        } else {
            if (prop_out) HIP_TRY((hipError_t)mi::dbridge::fill_nan_run(prop_out, d * N2, st));
            if (logg_post_out) HIP_TRY((hipError_t)mi::dbridge::fill_nan_run(logg_post_out, N1, st));
            if (logg_prop_out) HIP_TRY((hipError_t)mi::dbridge::fill_nan_run(logg_prop_out, N2, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        return MI_OK;
    }
    const bool whole = prop_out != nullptr;
    const BridgePropWs w = bridge_prop_ws(d, N2, whole, !whole || host);
    // behind the proposal's own areas: the staged results of a host call
    const size_t o_lg1 = w.bytes, o_lg2 = o_lg1 + (host && logg_post_out ? align256(N1 * 8) : 0);
    const size_t bytes = o_lg2 + (host && logg_prop_out ? align256(N2 * 8) : 0);
    WsLease ws;
    if ((rc = ws_get(st, bytes, ws))) return rc;
    char* W = ws.as<char>();
    double* const y_whole = !whole ? nullptr : (host ? reinterpret_cast<double*>(W + w.o_y) : prop_out);
    double* const lg1 = !logg_post_out ? nullptr : (host ? reinterpret_cast<double*>(W + o_lg1) : logg_post_out);
    double* const lg2 = !logg_prop_out ? nullptr : (host ? reinterpret_cast<double*>(W + o_lg2) : logg_prop_out);
    rc = bridge_prop_device(f, x + n_fit * d * C, n_it, d, C, N2, seed, W, w, y_whole, lg1, lg2, [](const double*, uint64_t, uint64_t) { return (int)MI_OK; }, st);
    if (rc) return rc;
    if (host) {
        if (prop_out) HIP_TRY(hipMemcpyAsync(prop_out, y_whole, d * N2 * 8, hipMemcpyDeviceToHost, st));
        if (logg_post_out) HIP_TRY(hipMemcpyAsync(logg_post_out, lg1, N1 * 8, hipMemcpyDeviceToHost, st));
        if (logg_prop_out) HIP_TRY(hipMemcpyAsync(logg_prop_out, lg2, N2 * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));                   // always blocking: the fit's host arrays, the staged slab and the workspace are ours
    return MI_OK;
}

int mi_mcmc_bridge_estimate(const double* logp_post, const double* logg_post, const double* logp_prop, const double* logg_prop, int32_t mem, uint64_t n_it,
                            uint64_t n_chains, uint64_t n_prop, double n_eff, double tol, uint64_t max_iter, double* f2_out, double* summary, void* stream)
{
    const char* who = "bridge_estimate";
    if (!logp_post || !logg_post || !logp_prop || !logg_prop) return fail(MI_ERR_BAD_ARG, "%s: null input", who);
    if (!f2_out && !summary) return fail(MI_ERR_BAD_ARG, "%s: f2_out and summary are both NULL, nothing is asked for", who);
    if (n_it > 0xffffffffULL || n_chains > 0xffffffffULL || n_prop > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: n_it / n_chains / n_prop do not fit 32 bits", who);
    const uint64_t C = n_chains, N1 = n_it * C, N2 = n_prop ? n_prop : N1;
    if (N1 < 2) return fail(MI_ERR_BAD_ARG, "%s: N1 = n_it * n_chains = %llu, at least 2 samples are needed", who, (unsigned long long)N1);
    if (N1 > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: N1 = %llu iteration samples, must be below 2^32", who, (unsigned long long)N1);
    if (N2 < 2) return fail(MI_ERR_BAD_ARG, "%s: n_prop = %llu, at least 2 proposal draws are needed", who, (unsigned long long)N2);
    int rc = bridge_param_check(who, n_eff, tol);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool host = mem == MI_MEM_HOST;
    const BridgeEstWs w = bridge_est_ws(n_it, C, N2);
    // behind the estimate's own areas: the staged inputs and f2 of a host call
    const size_t a1 = align256(N1 * 8), a2 = align256(N2 * 8);
    const size_t o_in = w.bytes, o_f2 = o_in + (host ? 2 * a1 + 2 * a2 : 0);
    const size_t bytes = o_f2 + (host && f2_out ? a1 : 0);
    WsLease ws;
    if ((rc = ws_get(st, bytes, ws))) return rc;
    char* W = ws.as<char>();
    const double *lp1 = logp_post, *lg1 = logg_post, *lp2 = logp_prop, *lg2 = logg_prop;
    if (host) {
        double* in = reinterpret_cast<double*>(W + o_in);
        HIP_TRY(hipMemcpyAsync(in, logp_post, N1 * 8, hipMemcpyHostToDevice, st)); lp1 = in; in += a1 / 8;
        HIP_TRY(hipMemcpyAsync(in, logg_post, N1 * 8, hipMemcpyHostToDevice, st)); lg1 = in; in += a1 / 8;
        HIP_TRY(hipMemcpyAsync(in, logp_prop, N2 * 8, hipMemcpyHostToDevice, st)); lp2 = in; in += a2 / 8;
        HIP_TRY(hipMemcpyAsync(in, logg_prop, N2 * 8, hipMemcpyHostToDevice, st)); lg2 = in;
    }
    double* const f2 = !f2_out ? nullptr : (host ? reinterpret_cast<double*>(W + o_f2) : f2_out);
    double sum8[8];
    if ((rc = bridge_estimate_device(lp1, lg1, lp2, lg2, n_it, C, N2, n_eff, tol, max_iter, W, w, f2, sum8, st))) return rc;
    if (summary) std::memcpy(summary, sum8, sizeof sum8);
    if (host && f2_out) HIP_TRY(hipMemcpyAsync(f2_out, f2, N1 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_mcmc_draws_bridge(const mi_target* target, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t n_chains, uint64_t n_fit, uint64_t n_prop,
                         uint64_t seed, double n_eff, double tol, uint64_t max_iter, double* f2_out, double* mean_out, double* cov_out, double* summary, void* stream)
{
    const char* who = "draws_bridge";
    const bool any_out = f2_out || mean_out || cov_out || summary;
    int rc = target_slab_check(who, target, draws_kdc, n_keep, n_chains, any_out ? nullptr : "f2_out, mean_out, cov_out and summary are all NULL, nothing is asked for", 1,
                               mi::dbridge::BRIDGE_MAX_D);
    if (rc) return rc;
    uint64_t N2 = n_prop;
    const uint64_t d = target->d, C = n_chains;
    if ((rc = bridge_shape_check(who, n_keep, d, C, &n_fit, &N2))) return rc;
    if ((rc = bridge_param_check(who, n_eff, tol))) return rc;
    switch (target->kind) {
    case MI_TARGET_GAUSS_ISO: case MI_TARGET_LOGISTIC: break;
    case MI_TARGET_GAUSS_DIAG:
    case MI_TARGET_GAUSS_DENSE:
        if (!target->prec) return fail(MI_ERR_BAD_ARG, "%s: target.prec is NULL", who);
        break;
    case MI_TARGET_NORMAL_MODEL:
        return fail(MI_ERR_UNSUPPORTED, "%s: MI_TARGET_NORMAL_MODEL has sigma > 0: a Gaussian proposal leaves its support", who);
    case MI_TARGET_GAUSS_MIXTURE:
        return fail(MI_ERR_UNSUPPORTED, "%s: MI_TARGET_GAUSS_MIXTURE is not implemented by this reducer", who);
    default:
        return fail(MI_ERR_BAD_ARG, "%s: unknown target kind %d", who, target->kind);
    }
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t n_it = n_keep - n_fit, N1 = n_it * C;
    if (target->kind == MI_TARGET_LOGISTIC && target->n_rows > (1ULL << 38)) return fail(MI_ERR_OOM, "%s: n_rows = %llu do not fit the device memory", who, (unsigned long long)target->n_rows);
    const bool host = mem == MI_MEM_HOST, target_host = target->mem == MI_MEM_HOST;
    DevBuf staged;
    const double* x = nullptr;
    if ((rc = stage_slab(draws_kdc, mem, n_keep, d, C, st, staged, &x))) return rc;
    BridgeFit f;
    if ((rc = bridge_fit(x, n_fit, d, C, st, f))) return rc;
    const bool ok = f.status == 0;
    if (mean_out) for (uint64_t a = 0; a < d; ++a) mean_out[a] = ok ? f.mu[a] : BRIDGE_NAN;
    if (cov_out) for (uint64_t a = 0; a < d * d; ++a) cov_out[a] = ok ? f.S[a] : BRIDGE_NAN;
    if (!ok) {
        if (summary) { for (int a = 0; a < 8; ++a) summary[a] = BRIDGE_NAN; summary[1] = 1.0; summary[7] = (double)N2; }
        if (f2_out && host) std::fill(f2_out, f2_out + N1, BRIDGE_NAN);
        if (f2_out && !host) HIP_TRY((hipError_t)mi::dbridge::fill_nan_run(f2_out, N1, st));
        HIP_TRY(hipStreamSynchronize(st));
        return MI_OK;
    }
    // the workspace: the proposal's, the estimate's, the log-kernel's packed matrix and staged target (its plan with nothing else staged), the four arrays, f2
    const BridgePropWs pw = bridge_prop_ws(d, N2, false, true);
    const BridgeEstWs ew = bridge_est_ws(n_it, C, N2);
    const mi::dlogk::LogkPlan lk = mi::dlogk::logk_plan(target->kind, d, target->n_rows, n_it, C, false, target_host);
    const size_t a1 = align256(N1 * 8), a2 = align256(N2 * 8);
    const size_t o_est = pw.bytes, o_lk = o_est + ew.bytes, o_arr = o_lk + align256(lk.bytes), o_f2 = o_arr + 2 * a1 + 2 * a2;
    const size_t bytes = o_f2 + (host && f2_out ? a1 : 0);
    WsLease ws;
    if ((rc = ws_get(st, bytes, ws))) return rc;
    char* W = ws.as<char>();
    const double *mat = target->kind == MI_TARGET_LOGISTIC ? target->X : target->prec, *y = target->y, *xs = x;
    if ((rc = stage_target_slab(W + o_lk, lk.o_mat, lk.o_y, lk.o_slab, lk.mat_doubles, lk.y_doubles, target_host, false, 0, st, &xs, &mat, &y))) return rc;
    double* const lp1 = reinterpret_cast<double*>(W + o_arr);
    double* const lg1 = lp1 + a1 / 8;
    double* const lp2 = lg1 + a1 / 8;
    double* const lg2 = lp2 + a2 / 8;
    const double* suffix = x + n_fit * d * C;
    HIP_TRY((hipError_t)mi::dlogk::logk_pack(lk, mat, W + o_lk, st));                       // once: the iteration part and every proposal group read the same packed matrix
    HIP_TRY((hipError_t)mi::dlogk::logk_run_packed(lk, suffix, mat, y, W + o_lk, lp1, st));
    auto logp_group = [&](const double* yg, uint64_t col0, uint64_t g) -> int {
        const mi::dlogk::LogkPlan gp = mi::dlogk::logk_plan(target->kind, d, target->n_rows, 1, g, false, target_host);      // (the areas of lk: the same d and rows)
        HIP_TRY((hipError_t)mi::dlogk::logk_run_packed(gp, yg, mat, y, W + o_lk, lp2 + col0, st));
        return MI_OK;
    };
    if ((rc = bridge_prop_device(f, suffix, n_it, d, C, N2, seed, W, pw, nullptr, lg1, lg2, logp_group, st))) return rc;
    double* const f2 = !f2_out ? nullptr : (host ? reinterpret_cast<double*>(W + o_f2) : f2_out);
    double sum8[8];
    if ((rc = bridge_estimate_device(lp1, lg1, lp2, lg2, n_it, C, N2, n_eff, tol, max_iter, W + o_est, ew, f2, sum8, st))) return rc;
    mi::host::last_kernel() = "bridge_propose_kernel, bridge_logg_kernel, bridge_pieces_kernel, bridge_moments_kernel";
    if (summary) std::memcpy(summary, sum8, sizeof sum8);
    if (host && f2_out) HIP_TRY(hipMemcpyAsync(f2_out, f2, N1 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

// Posterior predictive checks of a slab [n_keep][d][C] under the logistic target (draws_predict.hip; the arithmetic: include/mi_mcmc.h).  The slab and the
// target's arrays are staged into the workspace by the plan, as mi_mcmc_draws_waic stages them.
int mi_mcmc_draws_predict(const mi_target* target, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t n_chains, uint64_t seed, double* p_mean_out,
                          double* p_var_out, double* rep_freq_out, double* prob_out, double* yrep_out, double* t_rep_out, double* ll_rep_out, double* ll_obs_out,
                          double* summary, void* stream)
{
    const char* who = "draws_predict";
    const bool any_out = p_mean_out || p_var_out || rep_freq_out || prob_out || yrep_out || t_rep_out || ll_rep_out || ll_obs_out || summary;
    int rc = target_slab_check(who, target, draws_kdc, n_keep, n_chains, any_out ? nullptr : "all nine outputs are NULL, nothing is asked for", 2, mi::dpred::PRED_MAX_D, true);
    if (rc) return rc;
    switch (target->kind) {
    case MI_TARGET_LOGISTIC: break;
    case MI_TARGET_NORMAL_MODEL:
        return fail(MI_ERR_UNSUPPORTED, "%s: MI_TARGET_NORMAL_MODEL replicates are not implemented by this reducer", who);
    case MI_TARGET_GAUSS_ISO:
    case MI_TARGET_GAUSS_DIAG:
    case MI_TARGET_GAUSS_DENSE:
    case MI_TARGET_GAUSS_MIXTURE:
        return fail(MI_ERR_UNSUPPORTED, "%s: target kind %d has no observations: nothing to predict or replicate", who, target->kind);
    default:
        return fail(MI_ERR_BAD_ARG, "%s: unknown target kind %d", who, target->kind);
    }
    if (!target->y && (ll_obs_out || summary)) return fail(MI_ERR_BAD_ARG, "%s: ll_obs_out and summary need the observations target.y", who);
    if (target->n_rows > 0xffffffffULL) return fail(MI_ERR_BAD_ARG, "%s: n_rows = %llu does not fit 32 bits (the row is a slot of the generator)", who, (unsigned long long)target->n_rows);
    if ((rc = need_device())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t d = target->d, K = n_keep * n_chains, n_rows = target->n_rows;
    const bool slab_host = mem == MI_MEM_HOST, target_host = target->mem == MI_MEM_HOST;
    // what keeps the grids, every byte count and the sum of the replicated successes inside their types: beyond any device
    if (K > (1ULL << 38) || K > (1ULL << 62) / n_rows) return fail(MI_ERR_OOM, "%s: K = %llu columns x n_rows = %llu do not fit the device memory", who, (unsigned long long)K, (unsigned long long)n_rows);
    mi::dpred::PredictWants w;
    w.row_stats = p_mean_out || p_var_out || rep_freq_out;
    w.prob = prob_out != nullptr;
    w.yrep = yrep_out != nullptr;
    w.col_stats = t_rep_out || ll_rep_out || ll_obs_out;
    w.summary = summary != nullptr;
    const mi::dpred::PredictPlan plan = mi::dpred::predict_plan(d, n_rows, n_keep, n_chains, slab_host, target_host, target->y != nullptr, w, mi::test_grid_cap_now());
    if ((plan.rows && plan.rows_grid >= (1ULL << 31)) || (plan.cols && plan.cols_grid >= (1ULL << 31)))
        return fail(MI_ERR_OOM, "%s: %llu chunks x %llu rows do not fit the device memory", who, (unsigned long long)plan.n_chunks, (unsigned long long)n_rows);
    WsLease ws;
    rc = ws_get(st, plan.bytes, ws);
    if (rc) return rc;
    char* W = ws.as<char>();
    const double *x = draws_kdc, *mat = target->X, *y = target->y;
    if ((rc = stage_target_slab(W, plan.o_mat, plan.o_y, plan.o_slab, plan.mat_doubles, plan.y_doubles, target_host, slab_host, K * d, st, &x, &mat, &y))) return rc;
    double* prob = (slab_host && prob_out) ? reinterpret_cast<double*>(W + plan.o_prob) : prob_out;
    double* yrep = (slab_host && yrep_out) ? reinterpret_cast<double*>(W + plan.o_yrep) : yrep_out;
    HIP_TRY((hipError_t)mi::dpred::predict_run(plan, x, mat, y, seed, W, prob, yrep, st));
    mi::host::last_kernel() = plan.rows && plan.cols ? "predict_rows_kernel, predict_cols_kernel" : (plan.rows ? "predict_rows_kernel" : "predict_cols_kernel");
    const hipMemcpyKind back = slab_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    double* const row_out[3] = {p_mean_out, p_var_out, rep_freq_out};
    for (int i = 0; i < 3; ++i)
        if (row_out[i]) HIP_TRY(hipMemcpyAsync(row_out[i], W + plan.o_rowout + (size_t)i * plan.ldR * 8, n_rows * 8, back, st));
    double* const col_out[3] = {t_rep_out, ll_rep_out, ll_obs_out};
    for (int i = 0; i < 3; ++i)
        if (col_out[i]) HIP_TRY(hipMemcpyAsync(col_out[i], W + plan.o_colout + (size_t)i * K * 8, K * 8, back, st));
    if (slab_host && prob_out) HIP_TRY(hipMemcpyAsync(prob_out, prob, K * n_rows * 8, hipMemcpyDeviceToHost, st));
    if (slab_host && yrep_out) HIP_TRY(hipMemcpyAsync(yrep_out, yrep, K * n_rows * 8, hipMemcpyDeviceToHost, st));
    if (summary) {
        // t_obs on the host, from the caller's y or a copy of it; the counts over the columns on the device, one piece per workgroup
        std::vector<double> y_copy;
        const double* yh = target->y;
        if (!target_host) {
            y_copy.resize(n_rows);
            HIP_TRY(hipMemcpyAsync(y_copy.data(), target->y, n_rows * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            yh = y_copy.data();
        }
        double t_obs = 0.0;
        for (uint64_t r = 0; r < n_rows; ++r) t_obs = t_obs + yh[r];
        HIP_TRY((hipError_t)mi::dpred::predict_count(plan, t_obs, W, st));
        std::vector<uint64_t> pieces(3 * plan.count_grid);
        HIP_TRY(hipMemcpyAsync(pieces.data(), W + plan.o_pieces, pieces.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));               // blocking: summary is written on the host
        uint64_t n_t = 0, n_dev = 0, sum_t = 0;
        for (uint64_t g = 0; g < plan.count_grid; ++g) { n_t += pieces[3 * g]; n_dev += pieces[3 * g + 1]; sum_t += pieces[3 * g + 2]; }
        summary[0] = t_obs;
        summary[1] = (double)n_t / (double)K;
        summary[2] = (double)n_dev / (double)K;
        summary[3] = (double)sum_t / (double)K;
    } else if (slab_host || target_host) {
        HIP_TRY(hipStreamSynchronize(st));               // the outputs are the caller's host arrays / the target's host arrays have been read
    }
    return MI_OK;
}

}  // extern "C"
