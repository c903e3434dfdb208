// de.hpp -- mcmc::de (/root/reference/src/de.cpp:28-232) for many populations at once.
//
// A population is one call of mcmc::de: n_pop members of d values, swept member by member, in order and in place, once per
// generation (the reference with omp_n_threads = 1: its only deterministic reading).  Member i proposes
//     X_prop = (X_i + (X_c1 - X_c2) gamma) + r,   r_k = -b + (b + b) u_k          (de.cpp:167-169; no fma: -ffp-contract=off)
// and is replaced iff box_log_kernel(X_prop) - tv_i > log(z) (:176-183, de_cooling_schedule = 1).  The random numbers follow the
// counter-based contract of include/mi_mcmc.h (partners c1, c2 and z from block 0 of the member's slots, u_k from blocks 1..).
//
// Two kernels, same bits:
//   de_literal_kernel     one workgroup per population on literal.hpp's target_eval / box_log_kernel: every target kind the literal
//                         kernels know (and LIT_CALLBACK, the host-callback mailbox).  The correctness backbone.
//   de_gauss_mfma_kernel  iso / diag / dense Gaussians with d <= 128: the wave mapping of rwmh_gauss_mfma_kernel with ONE POPULATION
//                         PER COLUMN of the 16-wide tile; the 16 populations of a wave sweep their members in lock-step.  P is staged
//                         in LDS; a proposal is one matvec_mfma and one dot4 (the oracle's W = 4 orders).  The rows live in HBM
//                         ([n_pop][d][P], population index contiguous); each lane gathers its dimensions of rows i, c1(p), c2(p) and
//                         is the only lane that ever reads or writes those dimensions of its population, so the in-place sweep needs
//                         no synchronisation beyond program order.
#pragma once

#include "hmc_dense.hpp"
#include "literal.hpp"

namespace mi {

struct DeParams {
    lit::LitParams lit;          // the target (lit.t), the bounds (vals_bound / btype / lb / ub), the literal kernel's workspace
    const double* P;             // tile kernel: the d x d precision (device, row-major; ISO / DIAG expanded to a diagonal)
    uint32_t d, n_pop;
    uint64_t NP, pop0;           // populations in this launch, global id of local population 0
    double* X;                   // [n_pop][d][NP] in (draw0 > 0) / out, sampler (transformed) space
    double* tv;                  // [n_pop][NP] workspace: box_log_kernel of every member
    double* draws;               // [n_keep][n_pop][d][NP] or nullptr
    uint64_t* n_accept;          // [NP] or nullptr
    const double* init_vals;     // [d][NP]: initial_vals of every population (draw0 == 0, box side without a table)
    const double* box_lb;        // [d] de_settings.initial_lb, or nullptr: initial_vals - 0.5
    const double* box_ub;
    uint64_t seed;
    uint32_t n_burnin, n_keep, draw0;
    double gamma, gamma_jump, b;
    int jumps;
};

// slots per member of one generation: block 0 (partners, z) and one block per pair of dimensions
MI_HD uint32_t de_blocks(uint32_t d) { return 1u + (d + 1u) / 2u; }

// block 0: c1 uniform over {0..n_pop-1} \ {i}, c2 over {0..n_pop-1} \ {i, c1} -- integer maps, no rejection loop
MI_HD void de_partners(const u32x4& w, uint32_t i, uint32_t n_pop, uint32_t& c1, uint32_t& c2)
{
    c1 = (uint32_t)(((uint64_t)w.x * (uint64_t)(n_pop - 1u)) >> 32);
    c1 += (c1 >= i) ? 1u : 0u;
    const uint32_t lo = (i < c1) ? i : c1, hi = (i < c1) ? c1 : i;
    c2 = (uint32_t)(((uint64_t)w.y * (uint64_t)(n_pop - 2u)) >> 32);
    c2 += (c2 >= lo) ? 1u : 0u;
    c2 += (c2 >= hi) ? 1u : 0u;
}

// the uniform of dimension `dim` of member i's blocks in generation gen
MI_HD double de_u(uint64_t seed, uint64_t pop, uint32_t gen, uint32_t member, uint32_t nblk, uint32_t dim, uint32_t tag)
{
    const u32x4 w = rng_block(seed, pop, gen, member * nblk + 1u + dim / 2u, tag);
    return (dim & 1u) ? u01(w.z, w.w) : u01(w.x, w.y);
}

// the initial box of dimension dim (de.cpp:65-68): de_settings' table or initial_vals -/+ 0.5, then sampling_bounds_check
// (bounds_check.hpp:37-48: std::max / std::min against the hard bounds)
MI_HD void de_box(const DeParams& p, uint64_t pl, uint32_t dim, double& lo, double& hi)
{
    lo = p.box_lb ? p.box_lb[dim] : p.init_vals[(size_t)dim * p.NP + pl] + -0.5;
    hi = p.box_ub ? p.box_ub[dim] : p.init_vals[(size_t)dim * p.NP + pl] + 0.5;
    if (p.lit.vals_bound) {
        const int bt = p.lit.btype[dim];
        if (bt == 4 || bt == 2) lo = (p.lit.lb[dim] < lo) ? lo : p.lit.lb[dim];       // std::max(hard, sampling)
        if (bt == 4 || bt == 3) hi = (hi < p.lit.ub[dim]) ? hi : p.lit.ub[dim];       // std::min(hard, sampling)
    }
}

MI_HD double de_gamma(const DeParams& p, uint32_t gen) { return (p.jumps && (gen + 1u) % 10u == 0u) ? p.gamma_jump : p.gamma; }

MI_HD size_t de_row(const DeParams& p, uint32_t m, uint32_t dim, uint64_t pl) { return ((size_t)m * p.d + dim) * p.NP + pl; }
MI_HD size_t de_draw(const DeParams& p, uint32_t row, uint32_t m, uint32_t dim, uint64_t pl)
{
    return (((size_t)row * p.n_pop + m) * p.d + dim) * p.NP + pl;
}

// ---- one population on a workgroup (literal.hpp's target evaluation)
MI_HD void de_population(const lit::Par& par, const DeParams& p, uint64_t pl, double* wk)
{
    const lit::LitParams& lp = p.lit;
    const uint32_t d = p.d, n_pop = p.n_pop, nb = de_blocks(d);
    const uint64_t pop = p.pop0 + pl;
    const lit::Vecs v = lit::carve(wk, d, lp.t.n_rows, false);
    for (uint32_t i = 0; i < n_pop; ++i) {                  // de.cpp:126-147: the initial population and its target values
        LIT_PFOR(k, d) {
            double x;
            if (p.draw0 == 0) {
                double lo, hi;
                de_box(p, pl, k, lo, hi);
                x = lo + (hi - lo) * de_u(p.seed, pop, 0u, i, nb, k, STREAM_DE_INIT);
                p.X[de_row(p, i, k, pl)] = x;
            } else x = p.X[de_row(p, i, k, pl)];             // a continuation: the population of the call before
            v.cur[k] = x;
        }
        par.sync();
        double val = lit::box_log_kernel(par, lp, v, v.cur);
        if (!is_finite(val)) val = -INF;                    // :140-142
        if (par.tid == 0) p.tv[(size_t)i * p.NP + pl] = val;
        par.sync();
    }
    uint64_t n_acc = 0;
    const uint32_t n_total = p.n_burnin + p.n_keep;
    for (uint32_t g = 0; g < n_total; ++g) {
        const uint32_t gen = p.draw0 + g;
        const double gam = de_gamma(p, gen);                // :156-158, :202-204
        for (uint32_t i = 0; i < n_pop; ++i) {
            const u32x4 w = rng_block(p.seed, pop, gen, i * nb, STREAM_DE);
            uint32_t c1, c2;
            de_partners(w, i, n_pop, c1, c2);               // :174-180
            const double z = u01(w.z, w.w);
            const double tvi = p.tv[(size_t)i * p.NP + pl];  // read before the barriers ahead of thread 0's store below
            LIT_PFOR(k, d) {
                const double xi = p.X[de_row(p, i, k, pl)];
                const double r = -p.b + (p.b + p.b) * de_u(p.seed, pop, gen, i, nb, k, STREAM_DE);    // runif_vec_inplace(-b, b)
                v.prev[k] = xi;
                v.cur[k] = (xi + (p.X[de_row(p, c1, k, pl)] - p.X[de_row(p, c2, k, pl)]) * gam) + r;   // :169
            }
            par.sync();
            double prop = lit::box_log_kernel(par, lp, v, v.cur);     // :171
            if (!is_finite(prop)) prop = -INF;              // :173-175
            const bool accept = prop - tvi > det_log(z);    // :179-180 (a NaN difference rejects)
            const bool kept = g >= p.n_burnin;
            LIT_PFOR(k, d) {
                const double x = accept ? v.cur[k] : v.prev[k];
                if (accept) p.X[de_row(p, i, k, pl)] = x;
                if (kept && p.draws)                        // row i is final for this generation: draws_out.mat(g) = X (:196-198)
                    p.draws[de_draw(p, g - p.n_burnin, i, k, pl)] = lp.vals_bound ? lit::lit_inv_transform(x, lp.btype[k], lp.lb[k], lp.ub[k]) : x;
            }
            if (accept && par.tid == 0) p.tv[(size_t)i * p.NP + pl] = prop;
            if (accept && kept) ++n_acc;
            par.sync();
        }
    }
    if (par.tid == 0 && p.n_accept) p.n_accept[pl] = n_acc;
    par.sync();
}

// (mi_mcmc.hip reads the parameter block only: MI_DE_PARAMS_ONLY keeps the kernels in de_launch.hip's translation unit)
#if defined(__HIPCC__) && !defined(MI_DE_PARAMS_ONLY)
__global__ __launch_bounds__(256) void de_literal_kernel(const DeParams prm)
{
    const lit::Par par{(int)threadIdx.x, (int)blockDim.x};
    double* wk = prm.lit.work + (size_t)blockIdx.x * prm.lit.work_stride;
    for (uint64_t pl = blockIdx.x; pl < prm.NP; pl += gridDim.x) {
        de_population(par, prm, pl, wk);
        __syncthreads();
    }
}

// ---- 16 populations per wave on the matrix cores (iso / diag / dense Gaussians, d <= 128).  GENERAL: settings.vals_bound.
template <int NT, bool GENERAL>
__global__ MI_NO_DS_MERGE __launch_bounds__(256, 1) void de_gauss_mfma_kernel(const DeParams prm)
{
    constexpr int NS = 4 * NT;
    extern __shared__ __attribute__((aligned(16))) double lds_P[];
    double* const lds_lb = lds_P + (size_t)NT * 4 * NT * 64;
    double* const lds_ub = lds_lb + 16 * NT;
    int* const lds_bt = reinterpret_cast<int*>(lds_ub + 16 * NT);
    const lit::LitParams& lp = prm.lit;
    if constexpr (GENERAL) {
        for (int i = threadIdx.x; i < 16 * NT; i += blockDim.x) {
            const bool in = (uint32_t)i < prm.d;
            lds_lb[i] = in ? lp.lb[i] : 0.0;
            lds_ub[i] = in ? lp.ub[i] : 0.0;
            lds_bt[i] = in ? lp.btype[i] : 1;
        }
    }
    stage_precision<NT>(prm.P, prm.d, lds_P);           // ends with a barrier

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane >> 4;
    const uint64_t cl = ((uint64_t)blockIdx.x * 4 + wave) * 16 + (lane & 15);
    const bool live = cl < prm.NP;
    const uint64_t pl = live ? cl : prm.NP - 1;          // a dead lane shadows the last population and writes nothing
    const uint64_t pop = prm.pop0 + pl;
    const uint32_t d = prm.d, n_pop = prm.n_pop, nb = de_blocks(d);
    const double* afrag = lds_P + lane;
    const bool vb = GENERAL && lp.vals_bound != 0;

    double th[NS], tp[NS], xp[NS], wp[NS];
    // box_log_kernel (de.cpp:101-112) of tt: the same operations as rwmh_gauss_mfma_kernel's
    auto log_kernel = [&](const double (&tt)[NS]) __attribute__((always_inline)) -> double {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int dim = 4 * s + j;
            if constexpr (GENERAL) xp[s] = vb ? (((uint32_t)dim < d) ? box_inv_transform(tt[s], lds_bt[dim], lds_lb[dim], lds_ub[dim]) : 0.0) : tt[s];
            else xp[s] = tt[s];
        }
        matvec_mfma<NT>(afrag, xp, wp);
        double val = -0.5 * dot4<NS>(xp, wp);
        if constexpr (GENERAL) {
            if (vb) {
                double lj = 0.0;                             // log_jacobian.hpp:36-57: scalar loop, i ascending
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int i0 = 4 * s;
                    const double term = box_log_jacobian_term(tt[s], lds_bt[i0 + j], lds_lb[i0 + j], lds_ub[i0 + j]);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const double tg = __shfl(term, (lane & 15) + 16 * g);
                        if ((uint32_t)(i0 + g) < d && lds_bt[i0 + g] != 1) lj = lj + tg;
                    }
                }
                val = val + lj;
            }
        }
        return is_finite(val) ? val : -INF;              // de.cpp:140-142, :173-175
    };
    auto outv = [&](double v, uint32_t dim) __attribute__((always_inline)) -> double {
        if constexpr (GENERAL) { if (vb) return box_inv_transform(v, lds_bt[dim], lds_lb[dim], lds_ub[dim]); }
        return v;
    };

#pragma unroll 1
    for (uint32_t i = 0; i < n_pop; ++i) {              // the initial population (de.cpp:126-147) or the one handed over
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uint32_t dim = 4 * s + j;
            double x = 0.0;
            if (dim < d) {
                if (prm.draw0 == 0) {
                    double lo, hi;
                    de_box(prm, pl, dim, lo, hi);
                    x = lo + (hi - lo) * de_u(prm.seed, pop, 0u, i, nb, dim, STREAM_DE_INIT);
                    if (live) prm.X[de_row(prm, i, dim, pl)] = x;
                } else x = prm.X[de_row(prm, i, dim, pl)];
            }
            th[s] = x;
        }
        const double val = log_kernel(th);
        if (live) prm.tv[(size_t)i * prm.NP + pl] = val;   // (the four lanes of the column store the same value)
    }

    uint64_t n_acc = 0;
    const uint32_t n_total = prm.n_burnin + prm.n_keep;
#pragma unroll 1
    for (uint32_t g = 0; g < n_total; ++g) {
        const uint32_t gen = prm.draw0 + g;
        const double gam = de_gamma(prm, gen);
        const bool kept = g >= prm.n_burnin;
#pragma unroll 1
        for (uint32_t i = 0; i < n_pop; ++i) {
            const u32x4 w = rng_block(prm.seed, pop, gen, i * nb, STREAM_DE);
            uint32_t c1, c2;
            de_partners(w, i, n_pop, c1, c2);
            const double z = u01(w.z, w.w);
            const double tvi = prm.tv[(size_t)i * prm.NP + pl];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const uint32_t dim = 4 * s + j;
                double xi = 0.0, a = 0.0, bb = 0.0, u = 0.5;
                if (dim < d) {
                    xi = prm.X[de_row(prm, i, dim, pl)];
                    a = prm.X[de_row(prm, c1, dim, pl)];
                    bb = prm.X[de_row(prm, c2, dim, pl)];
                    u = de_u(prm.seed, pop, gen, i, nb, dim, STREAM_DE);
                }
                th[s] = xi;
                tp[s] = (dim < d) ? (xi + (a - bb) * gam) + (-prm.b + (prm.b + prm.b) * u) : 0.0;
            }
            const double prop = log_kernel(tp);
            const bool accept = prop - tvi > det_log(z);
            if (live) {
                if (accept) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const uint32_t dim = 4 * s + j;
                        if (dim < d) prm.X[de_row(prm, i, dim, pl)] = tp[s];
                    }
                    prm.tv[(size_t)i * prm.NP + pl] = prop;
                }
                if (kept && prm.draws) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const uint32_t dim = 4 * s + j;
                        if (dim < d) prm.draws[de_draw(prm, g - prm.n_burnin, i, dim, pl)] = outv(accept ? tp[s] : th[s], dim);
                    }
                }
            }
            if (accept && kept) ++n_acc;
        }
    }
    if (live && j == 0 && prm.n_accept) prm.n_accept[cl] = n_acc;
}
#endif

}  // namespace mi
