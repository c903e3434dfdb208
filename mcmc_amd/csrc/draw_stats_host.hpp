// draw_stats_host.hpp -- the host side that mi_mcmc_draw_stats and mi_mcmc_draw_stats_lags share (draw_stats.hip, which includes this file after
// draw_stats.hpp: the centre launches mi::stats_sum_kernel).  First the arithmetic, plain C++ over host arrays, which mi_mcmc_test_stats_host
// (mi_mcmc_probes.h) exports so that tests/test_draw_stats_host_cpu.py holds its bits without a device; then the device scratch of a call and the
// centre of the series.  The library is compiled with -ffp-contract=off: every expression below is evaluated as written.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "host_common.hpp"

namespace mi {
namespace dstats {

// The G partials of one (dimension, slot), first[g * stride], added in ascending g: what makes a result independent of the grid
inline double group_sum(const double* first, uint32_t G, size_t stride)
{
    double s = 0.0;
    for (uint32_t g = 0; g < G; ++g) s += first[(size_t)g * stride];
    return s;
}

// Geyer's initial positive sequence of dimension j over the lags [0, known) of ac[k * d + j] (mcmc_amd/ess.py's loop): the ESS per chain;
// *hit: the sum met its first non-positive pair.  Whether more lags could still change the sum is the caller's rule.
inline double geyer_ess(const double* ac, size_t d, size_t j, size_t n, size_t known, bool* hit)
{
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
}

// R-hat [d] from the moments mp[g][j][0..3): sums over the chains of group g of the chain mean, its square and the chain's unbiased variance
inline void rhat_from_moments(const double* mp, uint32_t G, size_t d, size_t n, size_t C, double* rhat)
{
    for (size_t j = 0; j < d; ++j) {
        const double* o = mp + j * 3;
        const double sm = group_sum(o, G, d * 3), sm2 = group_sum(o + 1, G, d * 3), sv = group_sum(o + 2, G, d * 3);
        const double W = sv / (double)C;                                                  // mean within-chain variance
        const double mbar = sm / (double)C;
        const double B_over_n = (C > 1) ? (sm2 - (double)C * mbar * mbar) / (double)(C - 1) : 0.0;   // variance of the chain means
        const double var_plus = ((double)(n - 1) / (double)n) * W + B_over_n;
        rhat[j] = (W > 0.0) ? std::sqrt(var_plus / W) : 1.0;
    }
}

// The slab of a call on the device, its chain groups (a route's own rule) and the stream
struct Slab {
    const double* x;
    size_t n, d, C;
    uint32_t G;
    hipStream_t st;
};

// The device scratch of a call, one buffer of the call's own (never the stream's leased workspace: the ranked drivers call in while they hold that
// lease, workspace.hpp): [G d] sums, [2 d] the centre in two parts, [d] dimension list, [G d 3] moments, [G d part_per] partials of the route's
// kernels; and the host copy of the sums
struct Scratch {
    host::DevBuf buf;
    size_t o_sum = 0, o_mean = 0, o_dims = 0, o_mom = 0, o_part = 0;
    std::vector<double> sums_h;
    hipError_t alloc(uint32_t G, size_t d, size_t part_per)
    {
        o_mean = o_sum + (size_t)G * d; o_dims = o_mean + 2 * d; o_mom = o_dims + d; o_part = o_mom + (size_t)G * d * 3;
        const hipError_t e = buf.alloc((o_part + (size_t)G * d * part_per) * 8);
        if (e == hipSuccess) sums_h.resize((size_t)G * d);
        return e;
    }
    double* at(size_t off) const { return buf.as<double>() + off; }
    const uint32_t* dims() const { return reinterpret_cast<const uint32_t*>(at(o_dims)); }
};

// dst[j] = the mean over the rows 0, step, 2 step, ... (`rows` of them) and every chain of x - centre[j] (centre == nullptr: of x): the G partials
// added in order.  Blocking.
inline int row_mean(const Slab& s, Scratch& S, const double* centre, uint32_t step, uint32_t rows, std::vector<double>& dst)
{
    hipLaunchKernelGGL(mi::stats_sum_kernel, dim3((unsigned)s.d, s.G), dim3(64), 0, s.st, s.x, centre, (uint32_t)s.n, step, (uint32_t)s.d, (uint64_t)s.C, s.G,
                       S.at(S.o_sum));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(S.sums_h.data(), S.at(S.o_sum), S.sums_h.size() * 8, hipMemcpyDeviceToHost, s.st));
    HIP_TRY(hipStreamSynchronize(s.st));
    for (size_t j = 0; j < s.d; ++j) dst[j] = group_sum(&S.sums_h[j], s.G, s.d) / ((double)rows * (double)s.C);
    return MI_OK;
}

// The centre of the series in TWO parts, v = (x - a_j) - e_j, at S.o_mean: a_j, a PROVISIONAL centre -- the mean over the chains of the FIRST,
// MIDDLE and LAST kept draw (rows 0, (n-1)/2, 2 ((n-1)/2) [= n-1 or n-2]), 3 / n of the slab; the first draw alone can sit far from the pooled
// mean when n_burnin is 0 and the chains share a start far from the mode --, and with `both` e_j = the mean of x - a_j over the whole slab, so
// that mean_j = a_j + e_j.  One double cannot hold the pooled mean to better than |mean| 2^-53 -- 1e-8 standard deviations at mean = 1e8,
// sd = 1 --, and series centred that far off carry the error, times their partial sums, into every autocovariance; x - a_j is exact where it
// matters (x near a_j) and e_j is small.  Without `both` (the Gram route of mi_mcmc_draw_stats) the second pass over the slab does not run.
inline int two_part_centre(const Slab& s, Scratch& S, bool both, std::vector<double>& a_h, std::vector<double>& e_h)
{
    const uint32_t t_step = (uint32_t)std::max<size_t>(1, (s.n - 1) / 2);
    const uint32_t n_sum = (uint32_t)((s.n + t_step - 1) / t_step);
    int rc;
    if ((rc = row_mean(s, S, nullptr, t_step, n_sum, a_h))) return rc;
    HIP_TRY(hipMemcpyAsync(S.at(S.o_mean), a_h.data(), s.d * 8, hipMemcpyHostToDevice, s.st));
    if (!both) return MI_OK;
    if ((rc = row_mean(s, S, S.at(S.o_mean), 1u, (uint32_t)s.n, e_h))) return rc;
    HIP_TRY(hipMemcpyAsync(S.at(S.o_mean) + s.d, e_h.data(), s.d * 8, hipMemcpyHostToDevice, s.st));
    return MI_OK;
}

}  // namespace dstats
}  // namespace mi
