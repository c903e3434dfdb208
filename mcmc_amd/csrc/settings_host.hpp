// settings_host.hpp -- the ONE host derivation of the per-dimension tables every sampler route reads: from settings.vals_bound / lower_bounds /
// upper_bounds, settings.precond_mat and (mala) settings.step_size to the bounds types, the mass tables, INV / CHOL_LOWER of a dense matrix and
// the constants of Sigma = eps^2 M -- in the operation order, the summation order and with the values the oracle states (host_linalg.hpp,
// det_math.hpp).  Plain host code without a HIP call: the C ABI (mi_mcmc.hip, callback_host.hip), the literal replay's preparation
// (literal_host.hpp) and the host test shim (tests/lit_host.hip) all read these functions, so that no two routes can disagree about a table.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

#include "det_math.hpp"
#include "host_linalg.hpp"

namespace mi {
namespace settings {

constexpr double LOG_2PI = 1.83787706640934548356;       // MCMC_LOG_2PI, stats/mcmc_stats.hpp:28-30

// determine_bounds_type.hpp:27-57: 1 none, 2 lower, 3 upper, 4 both (a NaN bound is not finite); without vals_bound type 1 and zeros
inline void bounds_tables(size_t d, int vals_bound, const double* lower, const double* upper, int* bt, double* lb, double* ub)
{
    for (size_t i = 0; i < d; ++i) {
        bt[i] = 1; lb[i] = 0.0; ub[i] = 0.0;
        if (!vals_bound) continue;
        lb[i] = lower[i]; ub[i] = upper[i];
        const bool fl = std::isfinite(lower[i]), fu = std::isfinite(upper[i]);
        bt[i] = (fl && fu) ? 4 : (fl && !fu) ? 2 : (!fl && fu) ? 3 : 1;
    }
}

// precond_mat (d*d row-major, or nullptr): 0 identity, 1 diagonal, 2 dense (an off-diagonal entry that compares unequal to zero: -0.0 does not, NaN does)
inline int precond_kind(const double* precond_mat, size_t d)
{
    if (!precond_mat) return 0;
    for (size_t i = 0; i < d; ++i)
        for (size_t k = 0; k < d; ++k)
            if (i != k && precond_mat[i * d + k] != 0.0) return 2;
    return 1;
}

// the diagonal of precond_mat with its CHOL_LOWER / INV as the oracle's Cholesky / Gauss-Jordan give them for a diagonal matrix: sqrt(m), 1 / m
inline void diag_mass(const double* precond_mat, size_t d, double* m, double* m_sqrt, double* m_inv)
{
    for (size_t i = 0; i < d; ++i) {
        const double v = precond_mat[i * d + i];
        m[i] = v; m_sqrt[i] = __builtin_sqrt(v); m_inv[i] = 1.0 / v;
    }
}

// INV and CHOL_LOWER of a dense precond_mat, row-major (every consumer converts to its own layout at upload); Minv may be nullptr (mala reads
// CHOL_LOWER(M) alone).  Returns 0, or the status of the (device) factorisation (host_linalg.hpp).
inline int dense_mass(const double* precond_mat, size_t d, std::vector<double>* Minv, std::vector<double>& L)
{
    if (Minv)
        if (int rc = host_inverse(precond_mat, d, *Minv)) return rc;
    return host_cholesky_lower(precond_mat, d, L);
}

// unbounded mala: Sigma = eps^2 M is constant (mala.ipp:41,58-64), so dmvnorm's constants come from the host once -- rs = 1 / eps^2, the constant
// term, INV(Sigma) and LOG_DET(Sigma) = sum_i 2 log CHOL_LOWER(Sigma)_ii, i ascending.
// kind (precond_kind) 0: mass unused; 1: mass = m[d], INV(Sigma) in sinv_diag; 2: mass = precond_mat (d*d row-major), INV(Sigma) row-major in Sinv.
struct MalaSigma {
    double rs = 0.0, cons_term = 0.0, log_det = 0.0;
    std::vector<double> sinv_diag, Sinv;
};
inline int mala_sigma(size_t d, double eps, int kind, const double* mass, MalaSigma& o)
{
    const double s2 = eps * eps;
    o.rs = 1.0 / s2;
    o.cons_term = -0.5 * (double)d * LOG_2PI;
    double ld = 0.0;
    if (kind == 0) {
        const double lii = __builtin_sqrt(s2);
        for (size_t i = 0; i < d; ++i) ld = ld + 2.0 * det_log(lii);
    } else if (kind == 1) {
        o.sinv_diag.resize(d);
        for (size_t i = 0; i < d; ++i) {
            const double sig = s2 * mass[i];
            o.sinv_diag[i] = 1.0 / sig;
            ld = ld + 2.0 * det_log(__builtin_sqrt(sig));
        }
    } else {
        std::vector<double> Sigma(d * d), Ls;
        for (size_t i = 0; i < d * d; ++i) Sigma[i] = s2 * mass[i];
        if (int rc = host_inverse(Sigma.data(), d, o.Sinv)) return rc;
        if (int rc = host_cholesky_lower(Sigma.data(), d, Ls)) return rc;
        for (size_t i = 0; i < d; ++i) ld = ld + 2.0 * det_log(Ls[i * d + i]);
    }
    o.log_det = ld;
    return 0;
}

// a table of n entries padded to n_padded with `fill` (what a kernel reads for the dimensions a tile holds beyond d); src may be nullptr with n = 0
template <class T>
inline void pad_table(const T* src, size_t n, size_t n_padded, T fill, T* out)
{
    for (size_t i = 0; i < n; ++i) out[i] = src[i];
    for (size_t i = n; i < n_padded; ++i) out[i] = fill;
}

}  // namespace settings
}  // namespace mi
