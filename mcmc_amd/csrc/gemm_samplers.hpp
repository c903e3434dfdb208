// gemm_samplers.hpp -- interface of the lock-step samplers for dense-gradient Gaussian targets BEYOND d = 512 (gemm_samplers.hip): the state of every
// chain lives in HBM ([dimension][chain], chains contiguous) and one leapfrog step of ALL chains is one fp64 matrix product W = P Theta on the matrix
// cores with the half-kicks and the drift fused into its epilogue.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mi {
namespace gemm {

enum : int { GEMM_HMC = 0, GEMM_MALA = 1, GEMM_RWMH = 3 };     // (the C ABI's algo numbers)

struct GemmRun {
    int algo = GEMM_HMC;
    uint32_t d = 0;
    uint64_t C = 0, chain0 = 0;
    const double* P = nullptr;        // dense Gaussian: d x d row-major precision, device
    const double* X = nullptr;        // logistic regression (when set): n_rows x d row-major design matrix and the labels, device
    const double* y = nullptr;
    uint32_t n_rows = 0;
    double* theta = nullptr;          // [d][C] in: initial values, out: final state (left alone for flagged chains)
    double* draws = nullptr;          // [n_keep][d][C] or nullptr
    uint64_t* n_accept = nullptr;     // [C] or nullptr (left alone for flagged chains)
    uint32_t* nf_flag = nullptr;      // [C + 1], zeroed by the caller: chains whose energies / proposal densities went non-finite (literal.hpp replays them)
    uint64_t seed = 0;
    uint32_t n_burnin = 0, n_keep = 0, n_leap = 0, draw0 = 0;
    double eps = 0.0;                 // step_size (hmc, mala) / par_scale (rwmh)
    double s2 = 0.0, rs = 0.0, log_det = 0.0, cons_term = 0.0;     // mala: dmvnorm's constants for Sigma = eps^2 I (mi_mcmc.hip: as the oracle states them)
    const double* mass_tables = nullptr;   // device, 4 tables of gemm_padded_d(d) doubles: diag(M), its sqrt, its reciprocal, diag(INV(eps^2 M)) (mala) -- ones / 1 / eps^2
                                           // for the identity, ones in the padding
    bool diag_mass = false;                // (for the kernel's name only: the tables decide)
    // a DENSE precond_mat (hmc, mala): d x d TRANSPOSED on the device (M_t[k * d + i] = M[i][k], what literal.hpp reads too) -- hmc: CHOL_LOWER(M), INV(M);
    // mala: M, CHOL_LOWER(M), INV(eps^2 M), with s2 / log_det / cons_term of it above; the mass tables are ones then
    bool dense_mass = false;
    const double *M_t = nullptr, *Lc_t = nullptr, *Minv_t = nullptr, *Sinv_t = nullptr;
    // settings.vals_bound (hmc with the identity / a diagonal precond_mat, rwmh): the chains live in the transformed space, the products are taken at
    // x = inv_transform(theta).  Device tables of gemm_padded_d(d) entries (type 1, bounds 0 in the padding) and, per 16-row block, whether it holds a bounded dimension
    bool bounded = false;
    const int* btype = nullptr;
    const double *lb = nullptr, *ub = nullptr;
    const uint32_t* box_blocks = nullptr;  // [gemm_padded_d(d) / 16]
    void* ws = nullptr;               // gemm_ws_bytes(d, n_rows, C, dense_mass, bounded) bytes of device memory
    bool use_graph = true;            // replay the launches of one draw from a captured hipGraph (the draw index lives in device memory)
};

uint32_t gemm_padded_d(uint32_t d);
size_t gemm_ws_bytes(uint32_t d, uint32_t n_rows, uint64_t C, bool dense_mass = false, bool bounded = false);      // n_rows = 0: the dense Gaussian
// enqueues the whole run on `st`; returns a hipError_t as int (0 = enqueued).  *kernel_name: what ran, for mi_mcmc_last_kernel()
int gemm_run(const GemmRun& r, hipStream_t st, const char** kernel_name);

// ---- mcmc::nuts on this route (gemm_nuts.hpp): identity or a DIAGONAL precond_mat, with or without settings.vals_bound (the caller sends bounded calls of fewer than 16 chains elsewhere), 1 <= max_tree_depth <= 10.  One RANGE of the call's chains per run:
// the caller's arrays are indexed by column c_off + c with the call's chain count C_total as their stride, the random numbers by chain0 + c_off + c.
struct GemmNutsRun {
    uint32_t d = 0;
    uint64_t C = 0, C_total = 0, c_off = 0, chain0 = 0;
    const double* P = nullptr;        // as GemmRun
    const double* X = nullptr;
    const double* y = nullptr;
    uint32_t n_rows = 0;
    double* theta = nullptr;          // [d][C_total] in / out (left alone for flagged chains, like every output below)
    double* draws = nullptr;          // [n_keep][d][C_total] or nullptr
    uint64_t* n_accept = nullptr;     // [C_total] or nullptr
    uint64_t* n_leap = nullptr;       // the REFERENCE's leapfrog count: one per leaf walked plus the search
    uint64_t* n_exec = nullptr;       // the leapfrogs made: one per distinct point plus the search
    double* step = nullptr;           // in (a continuation) / out
    uint32_t* depth = nullptr;        // [n_total][C_total] or nullptr
    double* adapt = nullptr;          // [3][C_total] dual-averaging state, in (a continuation inside the window) / out, or nullptr
    uint32_t* nf_flag = nullptr;      // [C_total + 1], zeroed by the caller
    uint64_t seed = 0;
    uint32_t n_burnin = 0, n_keep = 0, draw0 = 0, n_adapt = 0, max_depth = 0;
    double eps_bar0 = 0.0, delta = 0.0, gamma = 0.0, t0 = 0.0, kappa = 0.0;
    const double* mass_tables = nullptr;   // as GemmRun
    bool diag_mass = false;
    bool bounded = false;             // settings.vals_bound: as GemmRun (the chains live in the transformed space, the products are taken at x = inv_transform(theta))
    const int* btype = nullptr;
    const double *lb = nullptr, *ub = nullptr;
    const uint32_t* box_blocks = nullptr;
    void* ws = nullptr;               // gemm_nuts_fixed_bytes + round_up(C, 128) * gemm_nuts_chain_bytes(.., bounded) bytes
    bool pack = true;                 // pack the matrices into ws (false: a later range of the same call finds them there)
    bool use_graph = true;
    // out
    uint64_t ticks_run = 0, points_taken = 0, still_running = 0;      // still_running != 0: the tick ceiling was reached
};
uint32_t gemm_nuts_points(uint32_t max_depth);
uint64_t gemm_nuts_tick_ceiling(uint32_t max_depth, uint64_t n_total, bool search);
size_t gemm_nuts_chain_bytes(uint32_t d, uint32_t n_rows, uint32_t max_depth, bool bounded = false);      // bounded: one more vector of gemm_padded_d(d) doubles
size_t gemm_nuts_fixed_bytes(uint32_t d, uint32_t n_rows);
uint64_t gemm_nuts_range_chains(uint64_t C, size_t chain_bytes, size_t fixed_bytes, size_t budget);
// runs the range to its end (the host polls the device's counter of running chains: nothing waits on the device); returns a hipError_t as int
int gemm_nuts_run(GemmNutsRun& r, hipStream_t st, const char** kernel_name);

}  // namespace gemm
}  // namespace mi
