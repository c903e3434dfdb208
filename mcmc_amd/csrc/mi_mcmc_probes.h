/* mi_mcmc_probes.h -- TEST / MEASUREMENT infrastructure, not part of the product: the diagnostics of libmi_mcmc_probes.so (probes.hip,
 * probes_kc2.hip; built next to libmi_mcmc.so and linked against it): one MFMA tile, the deterministic math functions, the per-chain RNG, fp64
 * throughput ceilings.  Host pointers, blocking; status codes and mi_mcmc_last_error() as in mi_mcmc.h. */
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int mi_probe_mfma_f64(const double* A16x4, const double* B4x16, const double* C16x16, double* D16x16);
/* fn: 0 exp, 1 log, 2 sincos2pi of x in [0, 1) (out = sin, out2 = cos), 3 softplus, 4 sigmoid, 5 norm_ppf; out2 is 0 for every fn but 2 */
int mi_probe_math(int fn, const double* x, uint64_t n, double* out, double* out2);
/* two operands; fn: 0 det_pow(x, y) */
int mi_probe_math2(int fn, const double* x, const double* y, uint64_t n, double* out);
int mi_probe_normals(uint64_t seed, uint64_t chain, uint32_t draw, uint32_t stream, uint64_t d, double* out);
/* the d normals of one (chain, draw) in the canonical dimension <-> slot map through variant 0 rng_normal_pair (= mi_probe_normals), 1 rng_normal_pair_at,
 * 2 rng_normal_two_pairs, 3 rng_normal_four_pairs; d <= 2^24 */
int mi_probe_normals_variant(int variant, uint64_t seed, uint64_t chain, uint32_t draw, uint32_t stream, uint64_t d, double* out);
/* probes_kc2.hip: the three above from a translation unit that builds det_math.hpp with MI_KC_MODE 2 and MI_RNG_NOINLINE, as the logistic kernels do */
int mi_probe_math_kc2(int fn, const double* x, uint64_t n, double* out, double* out2);
int mi_probe_math2_kc2(int fn, const double* x, const double* y, uint64_t n, double* out);
int mi_probe_normals_kc2(int variant, uint64_t seed, uint64_t chain, uint32_t draw, uint32_t stream, uint64_t d, double* out);
int mi_probe_uniform(uint64_t seed, uint64_t chain, uint32_t draw, uint32_t slot, double* out);
int mi_probe_fp64_peak(int use_mfma, int iters, double* tflops_out);
int mi_probe_mfma_cycles(int waves_per_simd, int use_lds, int iters, double* cycles_per_mfma, double* tflops_out);
/* Defined in libmi_mcmc.so itself (a test hook, not a product entry point: it is declared here, not in mi_mcmc.h): limits the PERSISTENT grids of
 * the NUTS kernels with dynamic chain hand-out (nuts_memo.hpp, nuts_lds.hpp) to max_workgroups (0 = no limit), so that a test with a
 * few hundred chains runs the global counter, slot re-use and retire-on-leave.  The grid-stride grids of the matrix-product route beyond d = 512
 * (gemm_samplers.hip, gemm_nuts.hpp: the packs, the load and store of the state, the logistic row terms, the nuts init) take the same limit, so that a
 * test of a thousand chains runs the later passes of their loops, which otherwise need more than 16.7 M padded elements (65 535 workgroups; the row
 * terms: 2^20).  Kernels that index by workgroup id are not limited.  Process-wide.  Results do not depend on it. */
void mi_mcmc_test_set_grid_cap(uint32_t max_workgroups);
/* Defined in libmi_mcmc.so itself (a test hook like the one above): lowers the staging budget of the device INV / CHOL_LOWER of a dense precond_mat
 * (host_linalg.hpp, linalg_device.hip: 2 d doubles for INV, d for CHOL_LOWER, 60 KB of LDS) to `bytes` (0, or more than the real budget = the real
 * budget), so that a test at d of a few hundred runs what a matrix beyond d = 3840 / 7680 runs: the host loops instead of the device kernels,
 * and, for hmc / mala beyond d = 512, the literal kernel instead of the matrix-product route.  Process-wide; every call empties the memoised
 * factorisations (each thread's at its next use).  Results do not depend on it. */
void mi_mcmc_test_set_linalg_stage_bytes(uint32_t bytes);
/* ... and the number of INV / CHOL_LOWER factorisations this process has COMPUTED so far (on the device or in the host loops), i.e. those the two-entry
 * memo did not answer: what a test of the memo's hits, evictions and emptying reads.  Process-wide, monotonic. */
uint64_t mi_mcmc_test_linalg_computed(void);
/* ... and how many of those ran the device kernels (the others: the host loops -- d < 64, or beyond the staging budget).  The two paths return the same
 * bits, so this count is the only thing that tells a test of the capacity edge which one it ran. */
uint64_t mi_mcmc_test_linalg_computed_on_device(void);
/* Defined in libmi_mcmc.so itself (test hooks like the ones above), for mi_mcmc_nuts_run beyond d = 512 on the matrix-product route (gemm_nuts.hpp):
 * the workspace the route may take for ITSELF -- the packed matrices and one range of chains -- in bytes, as if that were all the free device memory (0 = the real
 * figure), so that a test with a few hundred chains runs what a call beyond the device's memory runs: consecutive ranges of chains in multiples of 128, and,
 * where not even 128 chains fit, the literal kernel.  Process-wide.  Results do not depend on it. */
void mi_mcmc_test_set_gemm_nuts_ws_bytes(uint64_t bytes);
/* ... the ranges of chains the route has run so far (process-wide, monotonic), and of its last call: the ticks run, the (tick, chain) slots in which the
 * chain was not idle, and all (tick, chain) slots. */
uint64_t mi_mcmc_test_gemm_nuts_ranges(void);
void mi_mcmc_test_gemm_nuts_last_ticks(uint64_t* ticks, uint64_t* busy_slots, uint64_t* slots);
/* ... and the host arithmetic of its routing, which needs no device: the tick ceiling of the host loop (search: a fresh run, with the step-size search's
 * allowance), the workspace bytes per chain and independent of the chains (n_rows = 0: the dense Gaussian), the chains per range under a budget. */
uint64_t mi_mcmc_test_gemm_nuts_tick_ceiling(uint32_t max_tree_depth, uint64_t n_draws, int search);
uint64_t mi_mcmc_test_gemm_nuts_chain_bytes(uint32_t d, uint32_t n_rows, uint32_t max_tree_depth);
uint64_t mi_mcmc_test_gemm_nuts_fixed_bytes(uint32_t d, uint32_t n_rows);
/* ... the bytes per chain of a call with settings.vals_bound: one vector of padded d doubles more (theta of the last point next to x) */
uint64_t mi_mcmc_test_gemm_nuts_bounded_chain_bytes(uint32_t d, uint32_t n_rows, uint32_t max_tree_depth);
uint64_t mi_mcmc_test_gemm_nuts_range_chains(uint64_t n_chains, uint64_t chain_bytes, uint64_t fixed_bytes, uint64_t budget);
/* Defined in libmi_mcmc.so itself (test hooks like the ones above), for hmc / mala / rwmh and nuts beyond d = 512 on the matrix-product route:
 * mode 1 never captures the launches of a draw / a tick into a graph -- every draw enqueues them itself, what a call of 65 536 chains does (its launches are long,
 * the rule is work x chains < 3e10) --; mode 0 is the rule as it is.  It skips the capture, nothing else: no environment variable, no runtime setting.  Process-wide,
 * read once per call.  Results do not depend on it. */
void mi_mcmc_test_set_gemm_graph(int mode);
/* ... the device memory the capacity condition of hmc / mala / rwmh on the route sees in place of the free memory plus this stream's cached workspace (0 = the real
 * figure): a call whose need exceeds it stays on the literal kernel, same bits.  Process-wide.  Results do not depend on it. */
void mi_mcmc_test_set_gemm_ws_bytes(uint64_t bytes);
/* ... and that need -- exactly the left-hand side of the condition; host arithmetic, no device: the route's workspace (gemm_ws_bytes) rounded up to 256, with
 * replay != 0 (hmc, mala: always with a dense precond_mat) the non-finite flags and the literal replay's transposed matrix and work areas behind it, and the uploads
 * next to it -- 1 MiB for the tables plus the target's d x d matrix, with a dense precond_mat the replay's four d x d matrices instead.
 * variant: 0 identity / diagonal precond_mat, 1 a dense precond_mat, 2 vals_bound.  n_rows = 0: the dense Gaussian. */
uint64_t mi_mcmc_test_gemm_need_bytes(uint32_t d, uint32_t n_rows, uint64_t n_chains, int variant, int replay);
/* Defined in libmi_mcmc.so itself (test hooks like the ones above), for mi_mcmc_draws_rank_transform / mi_mcmc_draw_stats_ranked (draws_rank.hpp): the
 * workspace budget of one group of dimensions in bytes (0, or more than the real budget = the real budget), so that a test at d = 5 runs the loop over
 * groups that a slab of gigabytes runs.  Process-wide.  Results do not depend on it. */
void mi_mcmc_test_set_rank_ws_bytes(uint64_t bytes);
/* ... and the host arithmetic of the group rule, which needs no device: the bytes a dimension takes (stats != 0: with the composed slab of
 * mi_mcmc_draw_stats_ranked), and the dimensions per group under the budget set above. */
uint64_t mi_mcmc_test_rank_dim_bytes(uint64_t n_keep, uint64_t n_chains, uint32_t flags, int stats);
uint64_t mi_mcmc_test_rank_dims_per_group(uint64_t n_keep, uint64_t d, uint64_t n_chains, uint32_t flags, int stats);
/* ... and the sorts run so far (one per group of dimensions and kind of key: x, |x - med|) and the radix passes they executed, at most eight each: a pass
 * whose digit is one value for every key of the group is skipped, and these counts are the only thing that tells a test so.  Process-wide, monotonic. */
void mi_mcmc_test_rank_counts(uint64_t* sorts, uint64_t* passes);
/* Defined in libmi_mcmc.so itself (a test hook like the ones above), for mi_mcmc_draws_log_kernel (draws_logk.hpp): the plan of a call, host arithmetic that
 * needs no device.  kind: mi_target_kind; slab_host / target_host != 0: the slab (with the result) / the target is staged in the workspace.
 * out8: route (0 one lane per column, 1 the fused matrix product), workgroups, threads per workgroup, LDS bytes per workgroup, the contraction extent Kp,
 * the padded output rows ldA, the row tiles a workgroup walks, the workspace bytes. */
void mi_mcmc_test_logk_plan(int32_t kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, int slab_host, int target_host, uint64_t* out8);
/* Defined in libmi_mcmc.so itself (a test hook like the ones above), for mi_mcmc_draw_stats (draw_stats.hpp, draw_stats.hip): what this thread's last call
 * launched.  out8: the route (0 the one-pass Gram kernel, 1 the window + lag-block ladder, 2 the streamed kernel), NB of the Gram kernel (0 on the other
 * routes), the chain groups G, the 64-chain tiles the largest chain group walked, the window launches, the lag-pass launches (stats_acov_kernel), those of
 * them that ran a subset of the dimensions, and the smallest such subset (0: none).  Host bookkeeping, per thread.  Results do not depend on it. */
void mi_mcmc_test_draw_stats_last(uint64_t* out8);
/* Defined in libmi_mcmc.so itself (a test hook like the ones above), for mi_mcmc_draw_stats_lags (draw_stats_lags.hpp, draw_stats.hip): what this thread's
 * last call launched.  out8: the block offsets ND, the bands of the schedule, the band passes that ran over a subset of the dimensions, the smallest
 * such subset (0: none), the time tiles per series, the chain groups G, the chains per tile (16, or all of a smaller group), the window K.  Host
 * bookkeeping, per thread.  Results do not depend on it. */
void mi_mcmc_test_draw_stats_lags_last(uint64_t* out8);
/* Defined in libmi_mcmc.so itself (a test hook like the ones above), for the host arithmetic that mi_mcmc_draw_stats and mi_mcmc_draw_stats_lags share
 * (draw_stats_host.hpp).  Inputs and outputs are HOST arrays; no device call is made.  acov [nlag][d] (NULL: ess and hit are left alone): ess[j] = Geyer's
 * sum of dimension j of a series of n draws over the lags [0, nlag), hit[j] = 1 where it met its first non-positive pair.  moments [G][d][3] (NULL: rhat is
 * left alone): rhat[j] from the sums over the chains of group g of the chain mean, its square and the chain variance, groups added in ascending order,
 * of C chains of n draws. */
void mi_mcmc_test_stats_host(const double* acov, uint64_t nlag, uint64_t d, uint64_t n, const double* moments, uint32_t G, uint64_t C, double* ess, uint8_t* hit,
                             double* rhat);
/* Defined in libmi_mcmc.so itself (a test hook like the ones above), for mi_mcmc_draws_waic (draws_waic.hpp): the plan of a call, host arithmetic that needs
 * no device.  kind: mi_target_kind (LOGISTIC or NORMAL_MODEL); slab_host / target_host != 0: staged in the workspace; want_loglik != 0: the matrix ll is
 * asked for.  out10: route (0 elementwise, 1 the matrix product), the chunk length in columns, the chunks, workgroups, threads per workgroup, LDS bytes per
 * workgroup, the padded rows ldR, the contraction extent Kp, the merge kernel's workgroups, the workspace bytes. */
void mi_mcmc_test_waic_plan(int32_t kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, int slab_host, int target_host, int want_loglik,
                            uint64_t* out10);
/* Defined in libmi_mcmc.so itself (test hooks like the ones above), for mi_mcmc_draws_psis_loo (draws_psis.hpp): the budget of the block ll [G][K] of one
 * row group in bytes (0, or more than the real budget = the real budget; a group never has fewer than 128 rows), so that a test of 300 rows runs the
 * loop over row groups that a call of terabytes runs; and the values of a row's tail a workgroup keeps in LDS (0, or more than the real capacity = the
 * real capacity), so that a test at M = 260 runs the route that re-reads the tail from the sorted row.  Process-wide.  Results do not depend on them. */
void mi_mcmc_test_set_psis_ll_bytes(uint64_t bytes);
void mi_mcmc_test_set_psis_lds_tail(uint32_t n_doubles);
/* ... and the plan of a call under the two hooks above and mi_mcmc_test_set_rank_ws_bytes, host arithmetic that needs no device.  out12: the tail length M,
 * the fit points m, the rows G of a group, the groups, the rows of the last group, the tail route (0 LDS, 1 re-read), LDS bytes of the tail, the pieces of
 * a row's body fold, the values of a piece, the rows per group of the sort, the bytes of the block ll, the workspace bytes. */
void mi_mcmc_test_psis_plan(int32_t kind, uint64_t d, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, int slab_host, int target_host, uint64_t* out12);
/* Defined in libmi_mcmc.so itself (a test hook like the ones above), for mi_mcmc_loglik_waic (psis == 0) and mi_mcmc_loglik_psis_loo (psis != 0)
 * (draws_loglik.hpp): the plan of a call under mi_mcmc_test_set_psis_lds_tail and mi_mcmc_test_set_rank_ws_bytes, host arithmetic that needs no device.
 * layout: MI_LOGLIK_ROWS / MI_LOGLIK_SLAB; mat_host != 0: the matrix is staged in the workspace.  out8: the chunks of 2 048 columns, the fold kernel's
 * workgroups, the tail length M, the fit points m, the rows per group of the sort, the sort groups, the tail route (0 LDS, 1 re-read), the workspace
 * bytes; M, m, the rows per group, the groups and the route are 0 for psis == 0. */
void mi_mcmc_test_loglik_plan(int32_t layout, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains, int mat_host, int psis, uint64_t* out8);
/* Defined in libmi_mcmc.so itself (a test hook like the ones above), for mi_mcmc_bridge_proposal without prop_out and mi_mcmc_draws_bridge (draws_bridge.hpp):
 * the budget of the block [d][g] of one group of proposal columns in bytes (0, or more than the real budget of 2 GiB = the real budget; a group never has
 * fewer than 16 columns), so that a test of a few hundred proposal draws runs the loop over groups that a call of gigabytes runs.  Process-wide.
 * Results do not depend on it. */
void mi_mcmc_test_set_bridge_prop_bytes(uint64_t bytes);
#ifdef __cplusplus
}
#endif
