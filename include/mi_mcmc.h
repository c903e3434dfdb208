/*
 * mi_mcmc.h -- C ABI of the MI355X many-chain HMC / MALA / NUTS (and RWMH) engine (libmi_mcmc.so).
 *
 * This is the drop-in boundary for the one hot path of kthohr/mcmc that BASELINE.json names.
 * Each entry point replaces, for C independent chains at once, one reference function:
 *
 *   mi_mcmc_hmc_*   <->  mcmc::hmc  -> internal::hmc_impl   /root/reference/include/mcmc/hmc.hpp:42-48,65-72,78-85
 *                                                            /root/reference/src/hmc.cpp:30-227
 *   mi_mcmc_mala_*  <->  mcmc::mala -> internal::mala_impl  /root/reference/include/mcmc/mala.hpp:43-49,66-73,79-86
 *                                                            /root/reference/src/mala.cpp:30-208, include/mcmc/mala.ipp:30-70
 *   mi_mcmc_nuts_*  <->  mcmc::nuts -> internal::nuts_impl  /root/reference/include/mcmc/nuts.hpp:42-48,65-72,78-85
 *                                                            /root/reference/src/nuts.cpp:30-332, include/mcmc/nuts.ipp:30-241
 *   mi_mcmc_rwmh_*  <->  mcmc::rwmh -> internal::rwmh_impl  /root/reference/include/mcmc/rwmh.hpp:42-47,64-70,79-85
 *                                                            /root/reference/src/rwmh.cpp:30-175
 *   mi_mcmc_rmhmc_* <->  mcmc::rmhmc -> internal::rmhmc_impl /root/reference/include/mcmc/rmhmc.hpp, src/rmhmc.cpp:30-287
 *   mi_settings     <->  algo_settings_t + hmc_/mala_/nuts_/rwmh_settings_t
 *                                                            /root/reference/include/misc/mcmc_structs.hpp:66-101,123-134,151-184
 *
 * The reference's std::function callback cannot run on the GPU, so the target density is
 * selected by a tagged descriptor (mi_target).  Plain C types only: no torch, no Eigen.
 * All structs start with their own size so the ABI can grow.
 *
 * Layouts (fp64 everywhere, fp_t = double: /root/reference/include/misc/mcmc_options.hpp:80-81,99):
 *   state  theta  [d][C]          structure-of-arrays, chain index contiguous
 *   draws         [n_keep][d][C]  one kept draw of every chain per slab
 *   n_accept      [C] uint64      post-burn-in accepts per chain (src/hmc.cpp:196-199)
 * Chain c of this call is global chain (chain0 + c): the Philox counter uses the global id, so
 * results do not depend on how chains are sharded over GPUs.
 */
#ifndef MI_MCMC_H
#define MI_MCMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_MCMC_VERSION 0x000600

typedef enum mi_status {
    MI_OK = 0,
    MI_ERR_BAD_ARG = 1,       /* NULL where forbidden, unsupported kind / dimension, struct_size mismatch */
    MI_ERR_HIP = 2,           /* a HIP runtime call failed; see mi_mcmc_last_error() */
    MI_ERR_UNSUPPORTED = 3,   /* valid request the device path does not implement (never falls back to CPU) */
    MI_ERR_OOM = 4,
    MI_ERR_NO_DEVICE = 5
} mi_status;

typedef enum mi_target_kind {
    MI_TARGET_GAUSS_ISO = 1,    /* log K = -1/2 |theta|^2 */
    MI_TARGET_GAUSS_DIAG = 2,   /* log K = -1/2 sum_i prec_i theta_i^2;       prec: d values */
    MI_TARGET_GAUSS_DENSE = 3,  /* log K = -1/2 theta^T P theta;              prec: d*d, symmetric, row-major */
    MI_TARGET_LOGISTIC = 4,     /* log K = sum_r [y_r eta_r - log(1+e^eta_r)] - 1/2 |beta|^2, eta = X beta.  d <= 512 on the LDS-staged MFMA
                                 * kernels: hmc / mala / rwmh / nuts; hmc and nuts also with vals_bound; a diagonal precond_mat (hmc, mala, nuts)
                                 * or, unbounded, a dense one (hmc, mala).  d <= 8: one chain per lane, every setting.  Everything else
                                 * (the remaining combinations, rwmh with a cov_mat or bounds beyond d = 8): the literal kernels -- same bits.  d > 512, hmc / mala / rwmh without
                                 * bounds / precond_mat (round 6): the state in HBM, two fp64 matrix products per gradient for all chains (gemm_samplers.hip);
                                 * hmc / mala there also with a diagonal or a DENSE precond_mat (dense: INV(M), CHOL_LOWER(M), M, INV(eps^2 M) as further products of the
                                 * same kernel, d <= 3840 and a workspace that fits the free device memory; otherwise the literal kernels);
                                 * hmc (identity / diagonal precond_mat) and rwmh (no cov_mat) there also with vals_bound: the chains in the transformed space, the products at
                                 * x = inv_transform(theta), J(theta) g in the product's epilogue (three more state vectors in the workspace; what does not fit the free device
                                 * memory, bounds with a dense precond_mat or chains.mass_diag: the literal kernels; bounded mala beyond d = 512: MI_ERR_UNSUPPORTED);
                                 * nuts there with or without vals_bound, with the identity or a DIAGONAL precond_mat and 1 <= max_tree_depth <= 10: per-chain memoised trees, every chain
                                 * at its own point of its own doubling of its own draw, the gradients of all chains as the products of one TICK (gemm_nuts.hpp); the host
                                 * polls a device counter of running chains -- nothing waits on the device -- up to a tick ceiling computed from the settings
                                 * (beyond it: MI_ERR_HIP).  With vals_bound the chain's last point, prev_draw, the point records and the tree's edges hold theta in the
                                 * transformed space, the products are taken at x = inv_transform(theta), J(theta) g is applied in the product's epilogue (gemm_step_kernel<13, .>)
                                 * and it is x that leaves.  Capacity rule: a chain holds 11 + 2 (1 + (D - 1) D / 2) vectors of d (padded to 16) doubles, D = max_tree_depth,
                                 * with vals_bound ONE more such vector (theta of the last point next to x),
                                 * the logistic target two more of n_rows (padded to 16), and 5.9 KB of scalars (0.85 MB at d = 1024, D = 10); next to the chains the
                                 * call needs the packed matrices, the literal replay's areas and, for chains / a target in host memory, their staged copies, which are
                                 * counted.  Chains that do not fit the free device memory together run as consecutive ranges, in multiples of 128
                                 * (same bits: the random numbers are counter-based on the global chain index); where not even 128 fit, and for a dense
                                 * precond_mat, max_tree_depth > 10, vals_bound with fewer than 16 chains and mi_mcmc_nuts_run_callback: the literal kernels;
                                 * the same for MI_TARGET_GAUSS_DENSE beyond d = 512 (one product per gradient) */
    MI_TARGET_NORMAL_MODEL = 5, /* d = 2, vals = (mu, sigma), observations x_1..x_n in y[0..n_rows): the model of the reference's
                                 * example programs (/root/reference/examples/eigen/rmhmc_normal.cpp:44-106),
                                 * log K = -n (log(2 pi)/2 + log sigma) - sum_r (x_r - mu)^2 / (2 sigma^2); its metric tensor for
                                 * rmhmc is the Fisher information diag(n / sigma^2, 2 n / sigma^2).  hmc, mala, nuts, rwmh, rmhmc (any
                                 * precond_mat / cov_mat, any bounds). */
    MI_TARGET_GAUSS_MIXTURE = 6 /* VALUE ONLY (no gradient): a mixture of M = n_rows isotropic Gaussians, for mi_mcmc_aees_run alone (every other
                                 * sampler returns MI_ERR_UNSUPPORTED).  X: the means, M x d row-major; prec: the variances s2_i (M values);
                                 * y: log c_i (M values), the log of weight_i / (2 pi s2_i)^(d/2), computed by the caller.
                                 *   dist_i = sum_j (x_j - mu_ij)^2          (j ascending, each square rounded, then added: no fma)
                                 *   a_i    = log c_i - (0.5 dist_i) / s2_i
                                 *   m      = max_i a_i                       (i ascending, a later a_i replaces m iff a_i > m)
                                 *   log K  = m + log(sum_i exp(a_i - m))     (i ascending; the engine's exp / log, det_math.hpp)
                                 * Non-finite: any a_i NaN -> NaN; m = -inf (every component underflows) -> -inf; m = +inf -> +inf. */
} mi_target_kind;

typedef enum mi_mem { MI_MEM_HOST = 0, MI_MEM_DEVICE = 1 } mi_mem;

/* Explicit kernel choice (mi_target.kernel_hint).  Every kernel that can serve a request produces the SAME bits, so a hint
 * changes speed only; a hint the request cannot honour is ignored.  The library reads no environment variable. */
typedef enum mi_kernel_hint {
    MI_KERNEL_AUTO = 0,
    MI_KERNEL_ELEMENTWISE_1LANE = 1,  /* hmc, separable Gaussian targets: one lane per chain (default for d > 128, many chains) */
    MI_KERNEL_ELEMENTWISE_4LANE = 2,  /* hmc, separable Gaussian targets: four lanes per chain */
    MI_KERNEL_NUTS_LOCKSTEP = 3,      /* nuts, unbounded Gaussian targets: the lock-step predecessor of the asynchronous kernel -- compiled into the
                                       * A/B library (`make prof`) only; the shipped library runs the tick-local kernel for this hint */
    /* hmc, dense-gradient Gaussian target, 64 < d <= 128, unbounded, identity precond_mat: the launch shape.  AUTO picks it from
     * the number of chains and of compute units (the shapes below are what makes 65 536 chains strong-scale over 8 GPUs). */
    MI_KERNEL_HMC_TWO_WAVES_PER_SIMD = 4,  /* 8 waves per workgroup, one 16-chain tile per wave: enough chains to fill the chip */
    MI_KERNEL_HMC_ONE_WAVE_PER_SIMD = 5,   /* 4 waves per workgroup, one tile per wave */
    MI_KERNEL_HMC_SPLIT2 = 6,              /* two waves share a tile (row halves of the mat-vec, theta exchanged through LDS) */
    MI_KERNEL_HMC_SPLIT4 = 7,              /* four waves share a tile, one wave per SIMD (16 chains per workgroup) */
    MI_KERNEL_HMC_SPLIT4_TWO_WAVES = 8,    /* four waves share a tile, two waves per SIMD (32 chains per workgroup) */
    MI_KERNEL_NUTS_TICK_LOCAL = 9,         /* nuts, unbounded Gaussian targets, identity precond_mat: the asynchronous kernel that executes every leaf and
                                            * reloads its start record (what the bounded / preconditioned variants run) instead of the default
                                            * one on the memoised trajectory -- an independent implementation of the same bits, for A/B runs */
    MI_KERNEL_NUTS_REG = 10,               /* RETIRED (round 5), valid and ignored: the register-carried kernel of rounds 2-4 (one wave per 16-chain tile) */
    MI_KERNEL_NUTS_SPLIT = 11,             /* RETIRED (round 5): the kernel that split every 16-chain tile over two waves (64 < d <= 128, few chains) is gone --
                                            * the memoised kernel is faster at every chain count.  The value stays valid and is ignored (as any hint a request
                                            * cannot honour): the default kernel runs */
    MI_KERNEL_LITERAL = 12,                /* nuts (and hmc with bounds / a diagonal precond_mat; hmc, mala and nuts with a DENSE precond_mat) on the logistic target
                                            * (d <= 512) and on dense Gaussians with 128 < d <= 512: the literal kernel (one workgroup per chain) instead of the tiled kernel on the
                                            * LDS-streamed evaluation -- same bits, for A/B timing.  mi_mcmc_de_run: de_literal_kernel (one workgroup per
                                            * population) instead of de_gauss_mfma_kernel on the Gaussians with d <= 128 -- same bits */
    MI_KERNEL_NUTS_DYN = 13,               /* RETIRED (round 5), valid and ignored: round 4's register-carried tick with dynamic chain hand-out */
    MI_KERNEL_NUTS_MEMO = 14,              /* nuts, same case: every doubling on a MEMOISED trajectory (nuts_memo.hpp) -- the 2^j leaves of a doubling visit only
                                            * 1 + j (j + 1) / 2 distinct states (the reference's crossed edge plumbing, nuts.ipp:195,207), each is computed
                                            * once, the tree is walked on scalars; same bits, ~40 % fewer leapfrogs executed on BASELINE configs[3]; chains
                                            * handed out dynamically -- THE kernel of the plain case (AUTO) */
    MI_KERNEL_NUTS_MEMO_INTICK = 15        /* the same kernel generating every draw's momentum INSIDE the tick (rounds 2-5).  AUTO instead fills a table of
                                            * all momenta of the run with a pre-pass kernel at full occupancy (16 NT + 2 doubles per chain and draw;
                                            * nuts_memo.hpp: nuts_momenta_kernel) and falls back to this form when the table would not fit.  Same bits */
} mi_kernel_hint;

typedef struct mi_target {
    uint32_t      struct_size;
    int32_t       kind;        /* mi_target_kind */
    uint64_t      d;           /* n_vals of one chain (BMO_MATOPS_SIZE(initial_vals), src/hmc.cpp:40) */
    const double* prec;        /* see mi_target_kind */
    const double* X;           /* LOGISTIC: n_rows x d row-major */
    const double* y;           /* LOGISTIC: n_rows */
    uint64_t      n_rows;
    int32_t       mem;         /* mi_mem: where prec / X / y live */
    int32_t       kernel_hint; /* mi_kernel_hint, 0 = automatic */
} mi_target;

/* POD mirror of algo_settings_t restricted to what hmc / mala / nuts read.
 * Field names and defaults follow mcmc_structs.hpp; mi_settings_default() fills them. */
typedef struct mi_settings {
    uint32_t struct_size;
    int32_t  vals_bound;          /* algo_settings_t::vals_bound (mcmc_structs.hpp:159) */
    uint64_t rng_seed_value;      /* algo_settings_t::rng_seed_value (:155) -> Philox key */
    const double* lower_bounds;   /* d values or NULL (host memory) */
    const double* upper_bounds;
    uint64_t n_burnin_draws;      /* default 1000 (:68) */
    uint64_t n_keep_draws;        /* default 1000 (:69) */
    uint64_t n_leap_steps;        /* hmc_settings_t::n_leap_steps, default 1 (:73) */
    double   step_size;           /* default 1.0 (:74, :94, :130); nuts: epsilon_bar_0; rwmh: par_scale (:145) */
    const double* precond_mat;    /* d*d (host) or NULL = identity (src/hmc.cpp:57); rwmh: cov_mat (:146, src/rwmh.cpp:58) */
    uint64_t n_adapt_draws;       /* nuts, default 1000 (:89) */
    double   target_accept_rate;  /* nuts, default 0.55 (:90) */
    uint64_t max_tree_depth;      /* nuts, default 10 (:92) */
    double   gamma_val;           /* 0.05 (:95) */
    double   t0_val;              /* 10 (:96) */
    double   kappa_val;           /* 0.75 (:97) */
    uint64_t n_fp_steps;          /* rmhmc_settings_t::n_fp_steps, default 5 (:116) */
} mi_settings;

/* One shard of chains. All pointers live in `mem` (host or device). */
typedef struct mi_chains {
    uint32_t  struct_size;
    int32_t   mem;            /* mi_mem of theta / draws / n_accept / step_size / n_leapfrogs */
    uint64_t  n_chains;       /* C: chains in this call */
    uint64_t  chain0;         /* global index of local chain 0 */
    double*   theta;          /* in: initial_vals [d][C]; out: last state of every chain */
    double*   draws;          /* out [n_keep][d][C], may be NULL (draws discarded) */
    uint64_t* n_accept;       /* out [C], may be NULL */
    double*   step_size;      /* nuts out [C]: adapted step size per chain (in: see draw0), may be NULL; other samplers leave it unchanged */
    uint64_t* n_leapfrogs;    /* out [C]: leapfrog steps per chain AS THE REFERENCE EXECUTES THEM (0 for mala / rwmh), may be NULL.  nuts: one per leaf of
                               * every tree (nuts.ipp:132) -- see n_leapfrogs_executed */
    uint32_t* nuts_depth;     /* nuts out [n_burnin+n_keep][C]: tree depth reached per draw, may be NULL */
    uint64_t  draw0;          /* index of this call's first draw in every chain's random stream: 0 for a fresh run; the
                               * n_burnin+n_keep of the call(s) before to CONTINUE them from their final theta -- the
                               * concatenation is then bit-identical to one long run (checkpoint / resume, chunked output).
                               * nuts: a continuation takes the step sizes back in through step_size; n_adapt_draws must be the
                               * same in every call of one run (it is the RUN's window); a continuation that starts at
                               * draw0 <= n_adapt_draws (draw n_adapt_draws itself still uses the last dual-averaging step, not
                               * epsilon_bar) also needs nuts_adapt_state below. */
    double*   nuts_adapt_state; /* nuts, may be NULL: the dual-averaging state [3][C] (h, epsilon_bar, mu: src/nuts.cpp:174-176,294-302), written
                               * at the end of every call.  With it (and step_size) a run can be cut ANYWHERE: a continuation that starts
                               * inside or at the end of the adaptation window (0 < draw0 <= n_adapt_draws) reads it back and continues the
                               * adaptation on the run's own schedule (draw indices are global: draw0 + i); the concatenation is
                               * bit-identical to one long run.  Without it a continuation must start after the window, as before. */
    const double* mass_diag;  /* hmc only, may be NULL: PER-CHAIN diagonal mass matrices [d][C] (same memory space as theta) -- NOT a
                               * reference mode (the reference has one precond_mat per call, i.e. per chain: this is C calls of
                               * mcmc::hmc with precond_mat = diag(mass_diag[:, c]) in one launch).  settings.precond_mat must be
                               * NULL.  Separable Gaussian targets without bounds run on the elementwise kernels (any d), everything
                               * else on the literal kernels.  See mi_mcmc_hmc_run_mass_adapted_per_chain. */
    uint64_t* n_leapfrogs_executed; /* out [C], may be NULL (needs n_leapfrogs next to it): the leapfrog steps the device really computed.
                               * Equal to n_leapfrogs except for nuts on the MEMOISED ticks -- the default of the plain and diagonal-mass
                               * Gaussian case, of the built-in Gaussian with vals_bound, of nuts on tile targets and (round 6) of nuts on the
                               * LDS-streamed evaluation (logistic d <= 512, dense Gaussians 128 < d <= 512) and on the matrix-product route (both beyond
                               * d = 512: one per distinct point of a doubling plus the step-size search) -- which compute every
                               * distinct state of a doubling once (same draws, fewer steps).  (MI_KERNEL_NUTS_MEMO is accepted and
                               * equivalent to MI_KERNEL_AUTO: the memoised tick is what runs unless MI_KERNEL_NUTS_TICK_LOCAL or
                               * MI_KERNEL_NUTS_LOCKSTEP asks for the kernel that executes every leaf.) */
} mi_chains;

void        mi_settings_default(mi_settings* s);
const char* mi_mcmc_last_error(void);
/* Name of the kernel the calling thread's last mi_mcmc_*_run spent its time in, as rocprofv3 prints it (e.g.
 * "hmc_gauss_mfma_kernel<8, 8, false, false, false>"); "" before the first call.  Kernel choice is automatic (mi_target.kernel_hint
 * overrides it): this is how a measurement names what actually ran. */
const char* mi_mcmc_last_kernel(void);
int         mi_mcmc_version(void);
int         mi_mcmc_device_count(void);

/* User-defined device targets (the reference's callback contract, hmc.hpp:42-48, as a compile-time __device__ functor; see
 * include/mi_mcmc_target.hpp): the generic host driver of the one-chain-per-lane engine.  A target library built with
 * MI_MCMC_DEFINE_TARGET calls this with its own `launch` function, which instantiates the kernels for its target type;
 * this validates, stages the chains (host or device memory) and packs the launch parameters.  algo: 0 hmc, 1 mala, 2 nuts,
 * 3 rwmh, 4 rmhmc; d <= 8; target_pod is handed through to `launch`. */
typedef int (*mi_small_launch_fn)(int algo, const void* small_params, const void* target_pod, void* stream);
int mi_mcmc_run_user_target(int algo, uint64_t d, mi_small_launch_fn launch, const void* target_pod, uint64_t small_params_bytes,
                            const mi_settings* settings, mi_chains* chains, void* stream);
/* What MI_MCMC_DEFINE_TARGET calls: the same with the MI_MCMC_VERSION of the headers the target library was compiled against.  A
 * target library instantiates engine kernels from those headers; one built against another version is refused (MI_ERR_BAD_ARG)
 * instead of running kernels whose parameter struct may mean something else at the same size. */
int mi_mcmc_run_user_target_v(int algo, uint64_t d, mi_small_launch_fn launch, const void* target_pod, uint64_t small_params_bytes,
                              int header_version, const mi_settings* settings, mi_chains* chains, void* stream);
/* The same for TILE targets (include/mi_mcmc_tile_target.hpp): value + gradient for 16 chains at once in the MFMA register layout,
 * d <= 16 nt, hmc (algo 0) and mala (1) with the identity precond_mat and no bounds.  wpb: waves per workgroup the target's kernels
 * are built for (4 or 8); lds_bytes: what the target stages; header_version: MI_MCMC_VERSION of the headers the target library was
 * compiled against -- it instantiates engine kernels from them, so a library built against other headers is refused (MI_ERR_BAD_ARG). */
typedef int (*mi_tile_launch_fn)(int algo, const void* tile_params, const void* target_pod, uint64_t lds_bytes, void* stream);
int mi_mcmc_run_tile_target(int algo, uint64_t d, int nt, int wpb, uint64_t lds_bytes, mi_tile_launch_fn launch, const void* target_pod,
                            uint64_t tile_params_bytes, int header_version, const mi_settings* settings, mi_chains* chains, void* stream);

/* Kernel workspaces are cached per (device, stream) and reused by later calls on that stream (NUTS at BASELINE configs[3]
 * holds 4 GiB).  This frees the cache of the CURRENT device for `stream` (all_streams != 0: for every stream, e.g. before
 * destroying streams); it synchronises first.  bytes_freed may be NULL.  Safe to call concurrently with runs. */
int mi_mcmc_release_workspace(void* stream, int all_streams, uint64_t* bytes_freed);

/* Blocking calls. `stream` is a hipStream_t (NULL = default stream); with mem == MI_MEM_DEVICE the
 * kernels are enqueued on it and the call returns after enqueueing (asynchronous), so inputs can be
 * resident in HBM and timed with events.  With MI_MEM_HOST buffers are staged and the call blocks.
 * Also blocking with MI_MEM_DEVICE: every configuration that owns temporary device tables for the call -- settings.vals_bound or
 * settings.precond_mat (bounds / preconditioner tables), a target given in host memory, and the runs that go to the literal kernels
 * with such tables -- ends in a stream synchronisation before those tables are freed.  The plain configurations (no bounds, no
 * precond_mat, target in device memory: every BASELINE config) do return after enqueueing.
 * With MI_MEM_DEVICE every device input (chains, target, mass_diag, the nuts continuation state) is read in the order of `stream` and every
 * output is written in the order of `stream`: work the caller queued on it before the call is seen, work queued after it sees the results. */
int mi_mcmc_hmc_run (const mi_target* target, const mi_settings* settings, mi_chains* chains, void* stream);
int mi_mcmc_mala_run(const mi_target* target, const mi_settings* settings, mi_chains* chains, void* stream);
int mi_mcmc_nuts_run(const mi_target* target, const mi_settings* settings, mi_chains* chains, void* stream);
/* mcmc::rwmh (/root/reference/include/mcmc/rwmh.hpp, src/rwmh.cpp:30-175) for many chains: settings->step_size carries
 * rwmh_settings_t::par_scale (mcmc_structs.hpp:145) and settings->precond_mat carries rwmh_settings_t::cov_mat (:146). */
int mi_mcmc_rwmh_run(const mi_target* target, const mi_settings* settings, mi_chains* chains, void* stream);

/* mcmc::rmhmc (/root/reference/include/mcmc/rmhmc.hpp, src/rmhmc.cpp:30-287) for many chains.  The reference takes the metric
 * tensor as a second callback (tensor_fn); here it is the one tied to the target kind: NORMAL_MODEL (d = 2) its Fisher
 * information; LOGISTIC with d <= 4 the Fisher information X^T diag(s(1-s)) X plus the prior precision I; a user-defined
 * target (mi_mcmc_target.hpp) its own tensor().  Reads
 * n_leap_steps, step_size, n_fp_steps, vals_bound / bounds from the settings; there is no precond_mat in rmhmc. */
int mi_mcmc_rmhmc_run(const mi_target* target, const mi_settings* settings, mi_chains* chains, void* stream);

/* mcmc::hmc with a DIAGONAL mass matrix adapted during burn-in -- NOT a reference mode (kthohr/mcmc has no mass adaptation;
 * SURVEY 8 f-2 asks for it because an ill-conditioned target does not mix with precond_mat = I at any step size).  Many chains
 * make the estimate cheap: the mass is POOLED over the chains, M = diag(1 / var_c(theta_i)), one matrix for all of them, taken
 * from the spread of the chains' current states -- first from initial_vals, then again after each of `n_windows` equal parts
 * of the burn-in.  Each part is an ordinary mi_mcmc_hmc_run call with that diagonal precond_mat (bit-exact against the oracle
 * given the mass, tests/test_gpu_mass_adapt.py) chained through mi_chains.draw0, so the whole run is reproducible; the kept
 * draws use the last estimate, returned in mass_diag_out[d] (host, may be NULL).  step_size is in the preconditioned metric
 * (every dimension near unit scale).  Gaussian targets (any d) and the logistic-regression target; settings->precond_mat
 * must be NULL; a dimension whose pooled variance is 0 or not finite keeps mass 1. */
int mi_mcmc_hmc_run_mass_adapted(const mi_target* target, const mi_settings* settings, mi_chains* chains, uint32_t n_windows,
                                 double* mass_diag_out, void* stream);
/* mcmc::hmc / mcmc::mala with a DENSE mass matrix adapted during burn-in -- NOT a reference mode either.  A diagonal mass cannot whiten a
 * CORRELATED target (a rotated Gaussian defeats it entirely); with many chains the pooled covariance of the chains' current states is a good
 * estimate of the target's and costs one matrix product (mi_mcmc_draws_covariance below).  Schedule, draw0 chaining, n_leapfrogs totals (mala:
 * 0) and argument checks are those of mi_mcmc_hmc_run_mass_adapted: an estimate from initial_vals, then again after each of `n_windows` equal
 * parts of the burn-in; n_windows <= n_burnin_draws; n_chains >= 2; settings->precond_mat and chains->mass_diag must be NULL (all four are
 * MI_ERR_BAD_ARG before any device call).  Each part is an ordinary mi_mcmc_hmc_run / mi_mcmc_mala_run with the dense precond_mat M, so it runs
 * wherever such a call runs today, and given M it has that call's bits.  ISO, DIAG, DENSE Gaussians and LOGISTIC, any d.
 * THE ESTIMATE, element-wise on the host in this order (C = n_chains; every operation rounded once, nothing contracted):
 *   1. S   = cov of mi_mcmc_draws_covariance(chains->theta, n_keep = 1)
 *   2. a   = C / (C + 5.0),  b = 1e-3 * (5.0 / (C + 5.0))                 (Stan's shrinkage of a window's covariance)
 *   3. S'_ij = a * S_ij  (i != j),   S'_ii = a * S_ii + b
 *   4. M0  = INV(S')                                                       (mi_mcmc_mat_inverse's routine)
 *   5. M_ij = 0.5 * (M0_ij + M0_ji)
 * The part runs with M = I instead when S has a non-finite entry or a diagonal entry <= 0, when M has a non-finite entry, or when
 * CHOL_LOWER(M) (mi_mcmc_mat_cholesky_lower's routine) has one: chains that share one start whose pooled variance is exactly 0 begin like
 * the diagonal variant's "mass 1".  precond_out [d*d] (host, row-major, may be NULL) receives the matrix the kept draws ran with.
 * step_size is in the preconditioned metric. */
int mi_mcmc_hmc_run_mass_adapted_dense(const mi_target* target, const mi_settings* settings, mi_chains* chains, uint32_t n_windows,
                                       double* precond_out, void* stream);
int mi_mcmc_mala_run_mass_adapted_dense(const mi_target* target, const mi_settings* settings, mi_chains* chains, uint32_t n_windows,
                                        double* precond_out, void* stream);
/* The per-chain form SURVEY 8 f-2 words ("per-chain diagonal mass adaptation"; what Stan does for each of its chains): every chain
 * estimates ITS OWN diagonal mass from ITS OWN draws.  The burn-in is cut into n_windows + 1 equal parts; part 0 runs with M = I;
 * the draws of part k are kept in a scratch slab and give, per chain and dimension, the variance over the part's draws (two passes,
 * draws ascending), regularised as Stan does, var' = (n var + 5e-3) / (n + 5), mass = 1 / var' (1 where that is not finite or
 * not positive); part k + 1 and finally the kept draws run with those masses.  Each part is an ordinary mi_mcmc_hmc_run with
 * mi_chains.mass_diag, chained through draw0: given the masses, chain c is bit-identical to mcmc::hmc with
 * precond_mat = diag(mass[:, c]) (tests/test_gpu_mass_adapt.py).  mass_diag_out: [d][C] in the memory space of `chains`, may be
 * NULL.  settings.step_size is in the preconditioned metric (every dimension near unit scale) and drives every part that has
 * masses; part 0 (M = I on the raw target) runs with first_step_size (0: settings.step_size) -- the reference's hmc has no step-size
 * adaptation, so the two scales are the caller's to give.  chains.mass_diag and settings.precond_mat must be NULL; n_windows >= 1;
 * every part needs at least 3 draws.  With >= 10^3
 * chains on one target the pooled estimate above is the better one (each chain sees few draws); this form is for chains that do
 * not share a scale (different data per chain are not expressible through mi_target, so: for parity with per-chain adaptation
 * elsewhere). */
int mi_mcmc_hmc_run_mass_adapted_per_chain(const mi_target* target, const mi_settings* settings, mi_chains* chains, uint32_t n_windows,
                                           double first_step_size, double* mass_diag_out, void* stream);

/* Host-callback form of mcmc::hmc for ONE chain: the reference's own target contract
 * (std::function<fp_t(const ColVec_t& vals_inp, ColVec_t* grad_out, void* target_data)>, hmc.hpp:42-48)
 * flattened to a C function pointer. The callback runs on the host, called exactly where the
 * reference calls it (2 gradient calls per leapfrog step, 1 value call per draw, 1 at setup);
 * everything else of the draw loop runs on the GPU. draws_out: n_keep x d column-major
 * (element (i,j) at i + j*n_keep, as Eigen's Mat_t stores draws_out). */
typedef double (*mi_log_kernel_cb)(const double* vals_inp, double* grad_out /* NULL = value only */, void* target_data);
int mi_mcmc_hmc_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel,
                             void* target_data, const mi_settings* settings, double* draws_out,
                             uint64_t* n_accept_draws);

/* The same for mcmc::mala (mala.hpp:66-73: 3 gradient + 1 value callback per draw, src/mala.cpp:149-186 with
 * include/mcmc/mala.ipp:58-64) and mcmc::nuts (nuts.hpp:65-72: two gradient callbacks per leaf of the recursive
 * nuts_build_tree, one value callback per leaf and per accepted proposal; dual averaging; step_size_out = final step size,
 * may be NULL).  One chain (global chain id 0); bit-identical to the device kernels run on the same target.  With settings.vals_bound
 * and / or settings.precond_mat these calls (and mi_mcmc_hmc_run_callback, mi_mcmc_rwmh_run_callback) run the literal kernel of the sampler
 * with the callback as its target: one device kernel that asks the host for every evaluation (see mi_mcmc_rmhmc_run_callback). */
int mi_mcmc_mala_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel,
                              void* target_data, const mi_settings* settings, double* draws_out,
                              uint64_t* n_accept_draws);
int mi_mcmc_nuts_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel,
                              void* target_data, const mi_settings* settings, double* draws_out,
                              uint64_t* n_accept_draws, double* step_size_out);
/* mcmc::rwmh (ref: include/mcmc/rwmh.hpp:42-47, src/rwmh.cpp:105-151): the callback is asked for the value only (grad_out is
 * always NULL), once per draw and once for the initial point; settings.step_size carries rwmh_settings.par_scale; identity
 * cov_mat, unbounded, one chain. */
int mi_mcmc_rwmh_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel,
                              void* target_data, const mi_settings* settings, double* draws_out,
                              uint64_t* n_accept_draws);

/* mcmc::rmhmc with HOST callbacks (ref: include/mcmc/rmhmc.hpp:44-63, src/rmhmc.cpp:30-287): target_log_kernel as above and the metric
 * tensor tensor_fn(vals_inp, tensor_deriv_out, tensor_data) flattened: tensor_out is d*d row-major, tensor_deriv_out (NULL when not asked
 * for) holds the d matrices dG/dvals_i at + i*d*d.  One chain (global chain id 0), d <= 64, bounds as in settings.  The sampler runs in ONE
 * device kernel (the literal rmhmc of mi_mcmc_rmhmc_run); each callback is a request the kernel posts to a mailbox in pinned memory and
 * this call serves on the calling thread until the kernel ends -- the callbacks are called exactly where the reference calls them
 * (per fixed-point step: 1 gradient; per position fixed-point step: 1 tensor; per leapfrog step 1 tensor + derivative and 1 gradient more;
 * 1 value per draw).  A request the host does not answer within 60 s makes the kernel give up (MI_ERR_HIP), never hang. */
typedef void (*mi_tensor_cb)(const double* vals_inp, double* tensor_out, double* tensor_deriv_out /* NULL = tensor only */, void* tensor_data);
int mi_mcmc_rmhmc_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel, void* target_data,
                               mi_tensor_cb tensor_fn, void* tensor_data, const mi_settings* settings, double* draws_out,
                               uint64_t* n_accept_draws);

/* ---- mcmc::de (ref: include/mcmc/de.hpp, src/de.cpp:28-232): differential-evolution MCMC, MANY populations per call.
 *
 * Each population is one call of mcmc::de: n_pop members of d values.  The initial population is lb + (ub - lb) * u per member
 * (lb / ub: de.initial_lb / initial_ub, or initial_vals -/+ 0.5; with vals_bound clamped to the hard bounds), used as it is in the
 * SAMPLER's space as the reference does (the target sees inv_transform of it).  gamma = 2.38 / sqrt(2 d) (the reference ignores
 * par_gamma); with jumps, generation g (global, burn-in included) uses par_gamma_jump when (g + 1) % 10 == 0.  A generation sweeps the
 * members i = 0 .. n_pop-1 IN ORDER and IN PLACE: X_prop = (X_i + (X_c1 - X_c2) gamma) + r, r_k = -b + (b + b) u_k; accept iff
 * prop - tv_i > log(z) (a NaN difference rejects); later members read the updated rows.  This is the reference run with
 * omp_n_threads = 1, its only deterministic reading.  settings: rng_seed_value, vals_bound / bounds, n_burnin_draws / n_keep_draws
 * (de_settings_t's counts); nothing else of mi_settings is read.
 *
 * RNG contract (counter-based Philox; the reference's per-thread std:: engines are not reproducible): rng_block(seed, pop, gen, slot,
 * tag) with pop the GLOBAL population (population0 + p), gen the GLOBAL generation (draw0 + local), slot = member * B + blk,
 * B = 1 + ceil(d / 2), tag 4 (tag 3 with gen = 0 for the initial population).  Block 0 (w0..w3) of a generation:
 *   c1 = (w0 * (n_pop - 1)) >> 32, c1 += (c1 >= i);
 *   c2 = (w1 * (n_pop - 2)) >> 32, c2 += (c2 >= min(i, c1)), then c2 += (c2 >= max(i, c1));
 *   z  = u01(w2, w3)     (u01(lo, hi) = (2 k + 1) 2^-53, k = the top 52 bits of hi:lo)
 * Blocks 1 .. ceil(d/2): dimension 2 (blk - 1) from u01(w0, w1), dimension 2 (blk - 1) + 1 from u01(w2, w3) -- the u of r above, and of
 * the initial population (tag 3).  n_pop * B must stay below 2^32 (MI_ERR_UNSUPPORTED). */
typedef struct mi_de_settings {
    uint32_t struct_size;
    int32_t  jumps;               /* de_settings_t::jumps, default false */
    uint64_t n_pop;               /* default 100; >= 3 (the reference loops forever below) */
    double   par_b;               /* default 1e-4 */
    double   par_gamma_jump;      /* default 2.0 */
    double   par_gamma;           /* default 1.0: carried, not read (the reference computes 2.38 / sqrt(2 d), src/de.cpp:61-62) */
    const double* initial_lb;     /* d host values or NULL (initial_vals - 0.5) */
    const double* initial_ub;     /* d host values or NULL (initial_vals + 0.5) */
} mi_de_settings;

/* P populations; all pointers in `mem`.  Layouts population-index contiguous, like mi_chains. */
typedef struct mi_populations {
    uint32_t  struct_size;
    int32_t   mem;
    uint64_t  n_populations;      /* P */
    uint64_t  population0;        /* global id of local population 0 (the Philox counter uses it: sharding does not change the bits) */
    const double* initial_vals;   /* [d][P]; read when draw0 == 0 and no initial box is given (may be NULL otherwise) */
    double*   population;         /* [n_pop][d][P] out: the last population in the sampler's (transformed) space; IN when draw0 > 0 */
    double*   draws;              /* [n_keep][n_pop][d][P] out (inverse-transformed when bounded), may be NULL */
    uint64_t* n_accept;           /* [P] out: accepts of the kept generations, summed over the members, may be NULL */
    uint64_t  draw0;              /* global index of this call's first generation: 0 for a fresh run; the generations of the calls
                                   * before to CONTINUE from `population` -- the concatenation is bit-identical to one long run */
} mi_populations;

void mi_de_settings_default(mi_de_settings* s);
/* Dispatch: iso / diag / dense Gaussians with d <= 128 (with or without bounds) on de_gauss_mfma_kernel (16 populations per wave, one
 * per column of the MFMA tile); every other kind target_eval knows (dense d > 128, logistic) on de_literal_kernel (one workgroup per
 * population), which MI_KERNEL_LITERAL also selects -- same bits.  MI_TARGET_NORMAL_MODEL: MI_ERR_UNSUPPORTED. */
int mi_mcmc_de_run(const mi_target* target, const mi_settings* settings, const mi_de_settings* de, mi_populations* pops, void* stream);
/* The reference's own contract, one population: target_log_kernel asked for the value only (grad_out NULL) once per member at setup and
 * once per proposal, served on the calling thread while de_literal_kernel runs (see mi_mcmc_rmhmc_run_callback).  initial_vals: d
 * values; draws_out: [n_keep][n_pop][d], may be NULL when n_keep == 0; n_accept: may be NULL.  Blocking. */
int mi_mcmc_de_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel, void* target_data,
                            const mi_settings* settings, const mi_de_settings* de, double* draws_out, uint64_t* n_accept);

/* ---- mcmc::aees (ref: src/aees.cpp:28-305, include/mcmc/aees.ipp:30-70): adaptive equi-energy sampling, MANY independent runs per call.
 *
 * One run is one call of mcmc::aees.  K = temper_len + 1 levels: temper_vec with 1.0 appended, sorted DESCENDING (level 0 the hottest,
 * level K-1 at T = 1).  S = n_initial_draws + n_burnin_draws, n_total = n_keep + K S.  For every draw n = 0 .. n_total-1 the levels run
 * in order 0 .. K-1 (the reference with omp_n_threads = 1, its only deterministic reading):
 *   level 0: one MH step at T_0.
 *   level k >= 1, active iff n > k S (inactive: its state stays the zero vector, its kernel values 0): with z_eps > ee_prob_par an MH
 *     step at T_k, kv0 = v / T_(k-1), kv1 = v / T_k; otherwise an equi-energy step: begin = (k-1) S, m = n - begin + 1,
 *     s = floor(m / n_rings); s = 0: the level stays put.  Else W = level k-1's T = 1 log kernels of draws begin .. n in ascending
 *     order, ring bounds b_i = (W[i s] + W[i s - 1]) / 2 (i = 1 .. n_rings-1), which_ring = the number of leading bounds with
 *     v_k(n-1) > b_i, r = s which_ring + floor(z_tmp s), ind_mix = the window POSITION of rank r; the proposal is level k-1's state
 *     at ABSOLUTE draw ind_mix, rejected iff z > exp(min(0.01, (new1 - kv1) + (kv0 - new0))).  v_k(n) = the level's log kernel.
 *   MH step: X' = X + (sqrt(T) (par_scale CHOL_LOWER(cov_mat))) z, the matrix product one fma chain per row (columns ascending);
 *     comp = std::min(0.01, (v' - v) / T) (a NaN difference gives 0.01: ACCEPT); accept iff u < exp(comp).  No clamp of non-finite
 *     values (unlike rwmh).
 *   kept draws: level K-1 for n >= K S, inverse-transformed when bounded.
 * The reference's quirks, reproduced as written:
 *   1. row 0 of kernel_vals is never written: level 1's window is all zeros, its ring bounds 0, its rank-r pick window position r;
 *   2. ind_mix is a window position used as an absolute draw index: for k >= 2 it points at early draws of level k-1, often zero
 *      states from before that level became active;
 *   3. a draw-storage entry not yet written reads as zeros (ind_mix = n; every state of an inactive level);
 *   4. the window's order, which get_sort_index leaves unspecified (and std::sort over NaN undefined), is OURS: ascending by value,
 *      ties by window position (a stable sort), -0 equal to +0, NaN after +inf.
 * cov_mat: d*d host values or NULL (the identity).  settings: rng_seed_value, vals_bound / bounds, n_burnin_draws / n_keep_draws (aees_settings_t's
 * counts); nothing else of mi_settings is read.  Refused before the device is touched (MI_ERR_BAD_ARG): n_rings = 0 (the reference's
 * n_rings - 1 wraps), a temperature <= 0 or not finite, n_total >= 2^32.  Continuing a run (a draw0 > 0) is NOT offered: it would need the
 * whole history of every level carried across calls.
 *
 * RNG contract (counter-based Philox): chain id run K + k with run the GLOBAL run (run0 + r), draw n:
 *   normals of an MH step: the engine's normal vector (rnorm_vec_inplace, literal.hpp) on stream tag 5;
 *   uniforms: rng_block(seed, run K + k, n, slot, tag 6); slot 0: z_eps = u01(w0, w1), the accept uniform of whichever test runs
 *   (MH or equi-energy) u01(w2, w3); slot 1: z_tmp = u01(w0, w1).  u01 as for mcmc::de.
 * Counters: n_accept[k] the accepted MH steps of level k over all n_total draws, n_ee_accept[k] the accepted equi-energy moves (0 for
 * level 0); a stay-put step (s = 0) counts as neither. */
typedef struct mi_aees_settings {
    uint32_t struct_size;
    uint32_t n_rings;             /* default 5; >= 1 */
    uint64_t n_initial_draws;     /* default 1000 */
    double   par_scale;           /* default 1.0 */
    const double* cov_mat;        /* d*d host values, row-major, or NULL = identity */
    double   ee_prob_par;         /* default 0.10 */
    const double* temper_vec;     /* temper_len host values (the levels above T = 1, any order), or NULL when temper_len = 0 */
    uint64_t temper_len;          /* default 0: K = 1, a plain MH chain at T = 1 */
} mi_aees_settings;

/* P runs; all pointers in `mem`.  Layouts run-index contiguous, like mi_chains. */
typedef struct mi_aees_runs {
    uint32_t  struct_size;
    int32_t   mem;
    uint64_t  n_runs;             /* P */
    uint64_t  run0;               /* global id of local run 0 (the Philox counter uses it: sharding does not change the bits) */
    const double* initial_vals;   /* [d][P] */
    double*   draws;              /* [n_keep][d][P] out (inverse-transformed when bounded), may be NULL */
    double*   final_states;       /* [K][d][P] out: every level's last state in the sampler's (transformed) space, may be NULL */
    uint64_t* n_accept;           /* [K][P] out, may be NULL */
    uint64_t* n_ee_accept;        /* [K][P] out, may be NULL */
} mi_aees_runs;

void mi_aees_settings_default(mi_aees_settings* s);
/* One workgroup per run on the literal target evaluation (literal.hpp): every kind it knows and MI_TARGET_GAUSS_MIXTURE;
 * MI_TARGET_NORMAL_MODEL: MI_ERR_UNSUPPORTED.  The history (every level's states and T = 1 log kernels, and a sorted index per level
 * k >= 2, merged lazily at the level's equi-energy steps) lives in a device workspace of the per-stream cache; the runs are served in
 * batches that keep it under a budget; MI_ERR_OOM only when one run alone does not fit. */
int mi_mcmc_aees_run(const mi_target* target, const mi_settings* settings, const mi_aees_settings* aees, mi_aees_runs* runs, void* stream);
/* The reference's own contract, one run: target_log_kernel asked for the value only (grad_out NULL), served on the calling thread while
 * the kernel runs.  The kernel keeps the log kernel of every level's current state (the target is deterministic), so it asks
 * 1 (the initial state) + (K > 1 ? 1 : 0) (the zero state of the levels not yet active) + one per MH step + one per equi-energy step
 * with s >= 1 -- the reference asks twice per MH step and once more per level and draw.  initial_vals: d values; draws_out: [n_keep][d],
 * may be NULL when n_keep == 0; final_states [K][d], n_accept [K], n_ee_accept [K]: may be NULL.  Blocking. */
int mi_mcmc_aees_run_callback(const double* initial_vals, uint64_t d, mi_log_kernel_cb target_log_kernel, void* target_data,
                              const mi_settings* settings, const mi_aees_settings* aees, double* draws_out, double* final_states,
                              uint64_t* n_accept, uint64_t* n_ee_accept);

/* ---- the BaseMatrixOps shim's INV and CHOL_LOWER as the engine computes them for a dense precond_mat (ref: src/hmc.cpp:58-59,
 * src/mala.cpp:58, include/stats/dmvnorm.hpp:36-41 through include/mcmc/mala.ipp:63-64): Gauss-Jordan with partial pivoting (first largest
 * magnitude) and column Cholesky, in the operation order the oracle states (oracle/mcmc_oracle.c: orc_inv, orc_chol_lower) -- bit-identical to
 * it.  A, Ainv, L: HOST memory, d x d row-major; A's lower triangle is what CHOL_LOWER reads, L is zero above the diagonal.  d >= 64 runs on
 * the device (one cooperative launch: d pivot / column steps of a parallel update, mcmc_amd/csrc/linalg_device.hip), smaller matrices on the
 * calling thread; no input validation, as in the reference (a singular / non-SPD matrix gives inf / NaN entries, not an error).  Blocking.
 * No limit on d: the device kernels stage the scaled pivot row (INV: 2 d doubles) resp. the finished column (CHOL_LOWER: d doubles) in 60 KB of
 * LDS; a matrix beyond that -- d > 3840 for INV, d > 7680 for CHOL_LOWER -- runs the same statements on the calling thread (one host core, O(d^3):
 * 89 ms measured at d = 512, which extrapolates to roughly 40 s at d = 4000 -- not measured) and returns the same bits, never MI_ERR_UNSUPPORTED.  For the samplers the same edge is a routing condition: hmc /
 * mala with a dense precond_mat beyond d = 3840 run on the literal kernels (MI_TARGET_LOGISTIC above), whose preparation factorises on the host.
 * (ABI 0x000600.  Every sampler call with a dense precond_mat goes through these.) */
int mi_mcmc_mat_inverse(const double* A, uint64_t d, double* Ainv);
int mi_mcmc_mat_cholesky_lower(const double* A, uint64_t d, double* L);

/* ---- multi-GPU: one process per GPU.  Chains are independent (the reference runs one per call), so the path shards with no
 * data-path collective: rank r of world_size runs the global chains [chain0, chain0 + n_local) in its own mi_mcmc_*_run call
 * (mi_chains.chain0 = chain0; the Philox counter uses the global id, so the union of the shards is bit-identical to one call).
 * The one exchange the path has is the collation of draws_out. */
void mi_mcmc_shard_bounds(uint64_t n_chains_total, uint32_t world_size, uint32_t rank, uint64_t* chain0, uint64_t* n_local);
/* All-gather of the kept draws over xGMI: every rank contributes its slab local_draws [n_keep][d][n_local] and receives
 * all_draws [n_keep][d][n_chains_total] (both DEVICE memory).  rccl_comm is the caller's ncclComm_t (one rank per GPU; RCCL is
 * loaded on first use, MI_ERR_UNSUPPORTED if librccl.so is absent).  Equal shards (n_chains_total divisible by world_size: every
 * BASELINE split) are ONE ncclAllGather into a rank-major staging buffer (`scratch`, n_keep * d * n_chains_total doubles on the
 * device); ragged shards need no padding: one grouped broadcast per rank into the same buffer (_ragged, which the first form
 * falls back to).  A merge kernel then interleaves the chain axis.  Enqueued on `stream`; returns after enqueueing. */
int mi_mcmc_allgather_draws(void* rccl_comm, uint32_t world_size, uint32_t rank, const double* local_draws, uint64_t n_keep,
                            uint64_t d, uint64_t n_chains_total, double* scratch, double* all_draws, void* stream);
int mi_mcmc_allgather_draws_ragged(void* rccl_comm, uint32_t world_size, uint32_t rank, const double* local_draws, uint64_t n_keep,
                                   uint64_t d, uint64_t n_chains_total, double* scratch, double* all_draws, void* stream);
/* the merge step alone: rank-major shards [r][n_keep][d][n_local(r)] (device) -> [n_keep][d][n_chains_total] (device) */
int mi_mcmc_merge_shards(const double* rank_major, uint32_t world_size, uint64_t n_keep, uint64_t d, uint64_t n_chains_total,
                         double* all_draws, void* stream);

/* The same collation in SURVEY 8(e)'s own receive layout -- rank-major, all_rank_major [G][n_keep][d][C / G] for equal shards (every
 * BASELINE split): ONE ncclAllGather straight into the caller's buffer, no staging buffer and no merge kernel (half the memory of the
 * form above: at configs[4], n_keep = 8, 64 GiB + the 8 GiB local slab per GPU).  Ragged shards arrive packed: shard r at offset
 * n_keep * d * chain0(r) with its own row length n_local(r) (what mi_mcmc_merge_shards reads), as one grouped broadcast per rank.
 * mi_mcmc_rank_major_index gives the offset of (kept draw i, dimension j, GLOBAL chain c) in either case (~0 if c is out of range). */
int mi_mcmc_allgather_draws_rank_major(void* rccl_comm, uint32_t world_size, uint32_t rank, const double* local_draws, uint64_t n_keep,
                                       uint64_t d, uint64_t n_chains_total, double* all_rank_major, void* stream);
uint64_t mi_mcmc_rank_major_index(uint64_t n_chains_total, uint32_t world_size, uint64_t n_keep, uint64_t d, uint64_t i, uint64_t j, uint64_t c);
/* Collation OVERLAPPED with sampling ("or per kept-draw slab, overlapped with the next trajectory").  _begin takes the
 * slab of kept draws [row0, row0 + n_keep) of a run that keeps n_keep_total (local_draws [n_keep][d][n_local], produced on
 * producer_stream), orders a gather into the run's rank-major buffer behind that stream's work so far, on the library's own
 * communication stream, and returns at once: the caller goes on to enqueue the next chunk of the run (mi_chains.draw0 continues
 * it bit-identically) on producer_stream while the slab travels.  _wait makes consumer_stream wait for the gather (block_host != 0:
 * the calling thread instead) and releases the handle.  Gathers of one communicator must be begun in the same order on every rank.
 * LIFETIME: between _begin and the completion of _wait the gather READS local_draws and WRITES rows [row0, row0 + n_keep) of
 * all_rank_major on the library's stream -- the caller must not overwrite local_draws (give every chunk in flight its own slab, or _wait
 * with block_host before re-using one) nor touch those rows of all_rank_major on any other stream until then.  Nothing enforces it. */
typedef struct mi_collation mi_collation;
int mi_mcmc_allgather_draws_begin(void* rccl_comm, uint32_t world_size, uint32_t rank, const double* local_draws, uint64_t n_keep,
                                  uint64_t d, uint64_t n_chains_total, uint64_t row0, uint64_t n_keep_total, double* all_rank_major,
                                  void* producer_stream, mi_collation** handle);
int mi_mcmc_allgather_draws_wait(mi_collation* handle, void* consumer_stream, int block_host);

/* Layout converters between the engine's [n_keep][d][C] slabs and the reference's per-chain
 * draws_out (n_keep x d, column-major as Eigen stores it: element (i,j) at i + j*n_keep;
 * src/hmc.cpp:138,197). Host memory. */
int mi_mcmc_draws_to_chain_major(const double* draws_kdc, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                                 double* out_c_colmajor /* [C][d][n_keep] */);
/* The same for slabs in HBM: both pointers are device memory, the transpose runs as a kernel on `stream` (LDS-tiled, coalesced
 * on both sides) and the call returns after enqueueing it. */
int mi_mcmc_draws_to_chain_major_device(const double* draws_kdc_dev, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                                        double* out_c_colmajor_dev /* [C][d][n_keep] */, void* stream);


/* Reducers over a draws_out slab [n_keep][d][C] (in `mem`), on the device (the reference has no ESS / R-hat
 * code, definitions as in mcmc_amd/ess.py).  Outputs are HOST arrays, any of them may be NULL:
 *   mean [d]          pooled mean over draws and chains
 *   acov [n_keep][d]  autocovariance at lag k, pooled over chains, unbiased per lag (divided by n_keep - k)
 *   rhat [d]          Gelman-Rubin potential scale reduction over the C chains
 *   ess  [d]          per-chain effective sample size (Geyer's initial positive sequence on acov); the many-chain ESS is
 *                     C times it.
 * Which kernels serve a call depends on n_keep alone:
 *   n_keep <= 128          every lag of every dimension in ONE pass over the slab, on the fp64 matrix cores, with or without acov;
 *   129 <= n_keep <= 160   with acov every lag, in passes of 48 lags; with acov == NULL only as many lags as Geyer's sum needs: the first 16
 *                          straight from HBM, then passes of 32 and of 48 lags over the dimensions whose sum has not met its first
 *                          non-positive pair yet (a slowly mixing series goes through every pass);
 *   n_keep > 160           (the reference's default is 1 000 kept draws) lags 0..127 from a kernel that streams the series through LDS; the
 *                          acov rows beyond hold NaN and Geyer's sum runs over the computed lags (every lag of a long series, and whether
 *                          the sum ended: mi_mcmc_draw_stats_lags below).
 * Accuracy: every output is that of exact arithmetic on the slab to within a few (n_keep + C) units of roundoff of its own terms -- R-hat to a
 * relative (n_keep + C + 64) 2^-52 as long as the spread of the chain means stays below 1e6 within-chain standard deviations, whatever the
 * means themselves are (DESIGN.md states the bounds; tests/draw_stats_ref.py derives them).  Blocking. */
int mi_mcmc_draw_stats(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                       double* mean, double* acov, double* rhat, double* ess, void* stream);

/* The same reducers with EVERY lag of a series of any length, up to a window the caller sets, on the fp64 matrix cores (mcmc_amd/csrc/draw_stats_lags.hpp,
 * draw_stats.hip): K = min(max_lag, n_keep - 1), MI_STATS_ALL_LAGS for every lag.  Outputs are HOST arrays, any of them may be NULL (all NULL:
 * MI_ERR_BAD_ARG):
 *   mean [d], rhat [d]   as mi_mcmc_draw_stats defines them
 *   acov [K + 1][d]      exactly K + 1 rows, acov_k = sum_c sum_{t < n - k} v_t v_{t+k} / (C (n - k)); no row is NaN unless the data are non-finite
 *   ess  [d]             Geyer's initial positive sequence (mcmc_amd/ess.py's loop) over the lags [0, K]: n_keep when n_keep < 4; otherwise
 *                        rho = acov / acov_0 (acov_0 <= 0: / 1), tau = -1 + 2 sum of the adjacent pairs rho_t + rho_{t+1}, t = 0, 2, .. while t + 1 <= K,
 *                        stopping before the first pair <= 0; n / max(tau, 1 / n) if tau > 0, else n; at most 10 n
 *   ended [d]            1: the sum met its non-positive pair inside the window, or K = n_keep - 1, or n_keep < 4 -- more lags would not change ess;
 *                        0: the window cut the sum.
 * Any n_keep >= 1 is served.  MI_ERR_BAD_ARG before any HIP call: a NULL slab, a zero size, n_keep or n_chains beyond 32 bits, d > 65 536; no device:
 * MI_ERR_NO_DEVICE; what does not fit: MI_ERR_OOM.  A host slab is staged.  Blocking.  Device memory: a buffer of the call's own.
 * HOW.  The lags are diagonal sums of the Gram matrix of the centred series over the chains; one 16 x 16 accumulator of v_mfma_f64_16x16x4_f64 per
 * block offset delta (rows 16 tb.. against rows 16 (tb + delta)..) holds the lags 16 delta - 15 .. 16 delta + 15, so lags 0 .. K need the offsets
 * [0, ND), ND = floor((K + 15) / 16) + 1.  BAND SCHEDULE, a function of (n_keep, K) alone: offsets [0, 8), [8, 16), then [16, 32), [32, 48), .. in
 * bands of 16, the last one cut at ND; one launch per band; after the band [a, b) the lags 0 .. 16 (b - 1) are complete (a lag 16 q + r, r > 0, is
 * the sum of its part from offset q and its part from offset q + 1, in that order).  With acov == NULL a further band runs only over the dimensions
 * whose sum has not ended inside the completed lags; with acov every band runs over every dimension.
 * DETERMINISM.  Every output is a function of the slab and (n_keep, d, C, K) alone: inside a workgroup the partial accumulators are added in a fixed
 * order, the host adds the G = max(1, min(64, ceil(C / 16), 2^18 / d)) chain groups in ascending order; no atomics.  The bits of mean, rhat, ess,
 * ended and of every acov_k do not depend on which outputs are NULL nor on which other dimensions are still open.
 * Non-finite samples propagate by the IEEE rules within their own dimension only.  The numpy statement is mcmc_amd/acov.py. */
#define MI_STATS_ALL_LAGS 0xffffffffu
int mi_mcmc_draw_stats_lags(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                            uint32_t max_lag,
                            double* mean /*[d]*/, double* acov /*[K+1][d]*/, double* rhat /*[d]*/, double* ess /*[d]*/,
                            uint8_t* ended /*[d]*/, void* stream);

/* Pooled mean and covariance of a slab [n_keep][d][C] (in `mem`; a host slab is staged), on the device: the samples are the K = n_keep * C
 * columns, ordered k = t * C + c.  The chains' current state mi_chains.theta ([d][C]) is the case n_keep = 1.  Outputs are HOST arrays, one
 * of them may be NULL: mean [d], cov [d*d] row-major.  K < 2, d = 0, a NULL slab or both outputs NULL: MI_ERR_BAD_ARG, before any HIP call
 * (as are n_keep or n_chains beyond 32 bits and d > 65 536).  Blocking.  Workspace: the stream's cached one (mi_mcmc_release_workspace).
 * DEFINITION (fp64, every operation rounded once; the product sums run on v_mfma_f64_16x16x4_f64, an fma chain per element):
 *   mu_i   = (sum_k x_ik) / K
 *   e_ik   = x_ik - mu_i
 *   cov_ij = (sum_k e_ik * e_jk) / (K - 1)
 * Every reduction order is a function of (n_keep, d, C) alone -- not of the CU count, the grid, timing or atomics:
 *   mean   G = min(max(1, 4096 / d), ceil(K / 4096)) groups (integer division), seg = 256 * ceil(ceil(K / G) / 256) samples each, then
 *          G = ceil(K / seg); in group g, s = 0 .. 255 adds the samples g * seg + s + 256 m, m ascending, from +0; the 256 sums are added by
 *          the halving tree (r[s] += r[s + h], h = 128, 64, .., 1); the group sums are added in ascending g from +0; one division by K.
 *   cov    CHUNKING RULE: T = ceil(d / 128) tile rows, P = T (T + 1) / 2 tiles with tj <= ti, n = max(1, 1024 / P) (integer division),
 *          KC = max(512, 16 * ceil(ceil(K / n) / 16)); chunk q holds the samples [q * KC, min(K, (q + 1) * KC)).  Inside a chunk an element
 *          is ONE fma chain over k ascending from +0; the chunk partials of an element are added in ascending q from +0; one division by
 *          K - 1.  Only elements with tile tj <= ti (inside a diagonal tile: j <= i) are computed; (j, i) is a copy of (i, j), so cov is
 *          symmetric bit for bit.
 * A non-finite sample propagates by the IEEE rules into the mean of its dimension and into that dimension's row and column of cov, and
 * nowhere else; nothing is flagged. */
int mi_mcmc_draws_covariance(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                             double* mean /* [d] host, may be NULL */, double* cov /* [d*d] host, row-major, may be NULL */,
                             void* stream);

/* Nested R-hat of a slab [n_keep][d][C] (in `mem`; a host slab is staged), on the device: the convergence diagnostic of MANY SHORT chains (Margossian,
 * Hoffman, Sountsov, Riou-Durand, Vehtari and Gelman, "Nested R-hat: assessing the convergence of Markov chain Monte Carlo when running many short
 * chains", Bayesian Analysis 2024).  The C = n_chains chains are K = C / M superchains of M = chains_per_super chains each, whose members were
 * started from one point: chain c is member m = c mod M of superchain k = c / M (integer division), so a superchain is a contiguous range of chains
 * and survives mi_mcmc_shard_bounds sharding whenever M divides the shard.  The variance of the superchain means (between) is compared with the
 * variance inside the superchains (within).  Defined for N = n_keep = 1: the chains' current state mi_chains.theta ([d][C]) is that case, no draws
 * slab is needed.  between / K is the Monte Carlo variance of the pooled mean.  Outputs are HOST arrays, any of them may be NULL (not all):
 * nrhat, mean, between, within, mcse_mean [d], super_mean [K][d].  Blocking.  Workspace: the stream's cached one (mi_mcmc_release_workspace).  No CPU
 * path: no device is MI_ERR_NO_DEVICE.  MI_ERR_BAD_ARG, before any HIP call: a NULL slab; all six outputs NULL; d = 0 or d > 65 536; n_keep or
 * n_chains 0 or beyond 32 bits; M = 0; C mod M != 0; K < 2; N = 1 together with M = 1 (within is identically 0).
 * DEFINITION (fp64, every operation rounded once, nothing fused).  SUM64(u_0 .. u_{n-1}): r[s] = sum_j u[s + 64 j], j ascending from +0.0, for
 * s = 0 .. 63 (a lane without elements stays +0.0); then r[s] = r[s] + r[s + h] for h = 32, 16, .., 1; the result is r[0].
 *   per column (i, c):                    s = sum_t x[t][i][c], t ascending from +0.0;  a = s / N
 *                                         N >= 2:  e = x - a,  p = e * e,  q = sum_t p ascending from +0.0,  v = q / (N - 1);   N = 1:  v = +0.0
 *   per (i, k), the members m ascending:  A_k = SUM64(a) / M
 *                                         M >= 2:  Bt_k = SUM64((a - A_k) * (a - A_k)) / (M - 1);   M = 1:  Bt_k = +0.0
 *                                         Wt_k = SUM64(v) / M;   w_k = Bt_k + Wt_k
 *   per dimension i, k ascending:         mean = SUM64(A) / K;   between = SUM64((A_k - mean) * (A_k - mean)) / (K - 1);   within = SUM64(w) / K
 *   on the host (sqrt correctly rounded): nrhat = sqrt(1.0 + between / within);   mcse_mean = sqrt(between / K);   super_mean[k][i] = A_k
 * The bits of every output depend on (slab, N, d, C, M) alone -- not on which outputs are NULL, on `mem`, the grid, timing or atomics (there are
 * none).  Non-finite samples propagate by the IEEE rules inside their own dimension and nowhere else; a constant dimension gives whatever 0 / 0 or
 * x / 0 gives; nothing is clamped or flagged.  For stationary superchains with independent members between / within is about
 * 1 / (M * ESS of one chain's N draws): a threshold on nrhat is a statement about M, and the choice stays with the caller.  The numpy statement is
 * mcmc_amd/nested_rhat.py. */
int mi_mcmc_draw_stats_nested(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                              uint64_t chains_per_super /* M */,
                              double* nrhat /*[d]*/, double* mean /*[d]*/, double* between /*[d]*/, double* within /*[d]*/,
                              double* mcse_mean /*[d]*/, double* super_mean /*[K][d]*/, void* stream);
/* The rank-normalised form, composed of mi_mcmc_draws_rank_transform (below) and the reducer above (outputs: HOST arrays [d], any may be NULL, not all):
 *   nrhat_bulk   nrhat of the MI_RANK_NORMAL slab with flags 0
 *   nrhat_tail   nrhat of the MI_RANK_NORMAL slab with MI_RANK_FOLD
 *   nrhat        the larger of the two, NaN if either is NaN
 * There is no MI_RANK_SPLIT: the diagnostic is defined at n_keep = 1.  Argument checks: those of mi_mcmc_draw_stats_nested (all three outputs NULL),
 * and n_keep * n_chains below 2^32 as the transform asks. */
int mi_mcmc_draw_stats_nested_ranked(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                                     uint64_t chains_per_super,
                                     double* nrhat, double* nrhat_bulk, double* nrhat_tail, /* host [d], any may be NULL, not all */
                                     void* stream);

/* Exact pooled order statistics and quantiles of a slab [n_keep][d][C] (in `mem`; a host slab is staged), on the device: the samples of
 * dimension i are the K = n_keep * C values x[t][i][c], pooled over draws and chains.  Outputs are HOST arrays.  Blocking.  Workspace: the
 * stream's cached one (mi_mcmc_release_workspace).  No CPU path: no device is MI_ERR_NO_DEVICE.  MI_ERR_BAD_ARG, before any HIP call: a NULL
 * slab, ranks, probs or out; d = 0; K = 0; n_keep or n_chains beyond 32 bits; d > 65 536; n_ranks = 0 or > MI_ORDER_STATS_MAX_RANKS; n_probs = 0
 * or > 16; a rank >= K; a probability outside [0, 1] or NaN.
 * ORDER.  Values are ordered by a 64-bit key; with u the bits of x:
 *   key(x) = 0xFFFFFFFFFFFFFFFF   for any NaN, of either sign and any payload
 *          = ~u                   if the sign bit of u is set
 *          = u | 2^63             otherwise
 * that is -inf < negatives < -0.0 < +0.0 < positives < +inf < NaN: numpy's sort order with the sign of zero made definite.
 * ORDER STATISTIC.  out[a][i] is the value whose key is the ranks[a]-th smallest (0-based) of dimension i's K keys -- exact, by a radix
 * selection on the keys (mcmc_amd/csrc/draws_select.hip) whose counts are integers: the result depends on no grid, timing or atomic order.  A
 * NaN comes back as the canonical quiet NaN 0x7FF8000000000000.  ranks may be unsorted and may repeat.
 * QUANTILE (Hyndman-Fan type 7, numpy's method="linear"), on the host from two order statistics per probability, fp64, every operation
 * rounded once, nothing contracted:
 *   h  = p * (double)(K - 1)
 *   lo = floor(h)                 (and at most K - 1: p = 1 with a K - 1 that the conversion rounded up)
 *   g  = h - (double)lo
 *   hi = min(lo + 1, K - 1)
 *   q  = (g == 0) ? x_lo : x_lo + g * (x_hi - x_lo)
 * Non-finite samples propagate by the IEEE rules through that one expression and nowhere else (g == 0 gives x_lo whatever x_hi is).
 * The numpy statement of all of this is mcmc_amd/quantiles.py. */
#define MI_ORDER_STATS_MAX_RANKS 32
int mi_mcmc_draws_order_stats(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                              const uint64_t* ranks /* host, n_ranks values, each < K */, uint32_t n_ranks,
                              double* out /* host, [n_ranks][d] */, void* stream);
int mi_mcmc_draws_quantiles(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                            const double* probs /* host, n_probs values in [0, 1] */, uint32_t n_probs /* <= 16 */,
                            double* out /* host, [n_probs][d] */, void* stream);

/* Exact ranks, normal scores and the rank-normalised diagnostics of a slab [n_keep][d][C] (in `mem`; a host slab is staged), on the device: Vehtari,
 * Gelman, Simpson, Carpenter and Buerkner (2021), "Rank-normalization, folding, and localization: an improved R-hat".  Blocking.  Workspace: the
 * stream's cached one (mi_mcmc_release_workspace).  No CPU path: no device is MI_ERR_NO_DEVICE (mi_mcmc_norm_ppf is host arithmetic and needs none).
 * MI_ERR_BAD_ARG, before any HIP call: a NULL slab or out; all five outputs NULL; d = 0 or d > 65 536; n_keep or n_chains beyond 32 bits; S = 0 or
 * S >= 2^32; an unknown `what` or flag bit; n_keep < 2 with MI_RANK_SPLIT; n_keep < 4 for mi_mcmc_draw_stats_ranked.
 * fp64, every operation rounded once, nothing contracted.
 * RETAINED ROWS AND LAYOUT.  Without MI_RANK_SPLIT every row is retained and out is [n_keep][d][C].  With it h = floor(n_keep / 2), the retained
 *   rows are t < h and t >= n_keep - h (the middle row of an odd n_keep is not read) and out is [h][d][2C]:
 *     out[t][i][c]     from x[t][i][c]
 *     out[t][i][C + c] from x[n_keep - h + t][i][c]
 *   the slab of 2C half-chains, which mi_mcmc_draw_stats takes as it is.  S is the number of retained samples of a dimension (n_keep C, or 2 h C).
 * VALUE RANKED.  v = x, or with MI_RANK_FOLD v = |x - med_i|: one subtraction, then the sign cleared; med_i is the type-7 quantile at p = 0.5 of
 *   dimension i's S retained samples, by mi_mcmc_draws_quantiles' rule above (K = S).
 * ORDER.  The 64-bit key of mi_mcmc_draws_order_stats, unchanged: -0.0 sorts below +0.0, every NaN has one key, above +inf.
 * RANK.  lo = the number of retained keys of the dimension below key(v), hi = the number not above it; R2 = lo + hi + 1 is twice the average
 *   1-based rank.  MI_RANK_AVERAGE writes 0.5 * (double)R2 (exact: a multiple of 0.5).  A NaN v counts in S and in the ranks of the others, and
 *   itself comes out as the canonical quiet NaN 0x7FF8000000000000, for both values of `what`.
 * NORMAL SCORE.  MI_RANK_NORMAL writes z = norm_ppf(p), p = (0.5 * (double)R2 - 0.375) / ((double)S + 0.25).  p lies strictly inside (0, 1) for
 *   every S >= 1, so z is finite for every non-NaN sample, +-inf included; a constant dimension gives p = 0.5 exactly and z = +0.0.
 * norm_ppf.  Wichura's algorithm AS 241, routine PPND16, one function for the host and the device (include/mi_mcmc_engine/det_math.hpp): three
 *   rational polynomials in nested Horner form, plain multiplies and adds, one division; |p - 0.5| <= 0.425 the central one in r = 0.180625 - q^2,
 *   otherwise r = sqrt(-det_log(min(p, 1 - p))) and the branches r <= 5 and r > 5; coefficients, limits and nesting as in CPython's
 *   statistics.NormalDist.inv_cdf.  p <= 0 gives -inf, p >= 1 gives +inf, NaN gives NaN.
 * The ranks come from a full sort of every dimension's keys (mcmc_amd/csrc/draws_rank.hip: a radix sort whose counts are integers, and a search of
 * every sample in the sorted image): the result depends on no grid, timing or atomic order.  The numpy statement is mcmc_amd/rank_stats.py. */
#define MI_RANK_AVERAGE 0      /* out = the average 1-based rank, as a double (exact: a multiple of 0.5) */
#define MI_RANK_NORMAL  1      /* out = z, the normal score of that rank */
#define MI_RANK_SPLIT   1u     /* flags: split every chain into halves */
#define MI_RANK_FOLD    2u     /* flags: rank |x - med_i| instead of x */
int mi_mcmc_draws_rank_transform(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                                 int32_t what, uint32_t flags, double* out /* in `mem` */, void* stream);
/* The diagnostics, composed of the transform above and mi_mcmc_draw_stats, whose R-hat formula and Geyer ESS are unchanged and here apply to a slab
 * of 2C half-chains of length h (outputs: HOST arrays [d], any of them may be NULL):
 *   rhat_bulk, ess_bulk   R-hat and ESS of the MI_RANK_SPLIT, MI_RANK_NORMAL slab
 *   rhat_tail             R-hat of the MI_RANK_SPLIT | MI_RANK_FOLD, MI_RANK_NORMAL slab
 *   rhat                  the larger of the two, NaN if either is NaN
 *   ess_tail              the smaller of the ESS of the two indicator slabs 1{x <= q05_i} and 1{x <= q95_i} (values 0.0 / 1.0 in the split layout; q
 *                         the type-7 quantile of the retained samples; a NaN x gives a NaN indicator)
 * The ESS values are per HALF-chain, as mi_mcmc_draw_stats' are per chain: the many-chain figure is 2C times it.  A dimension with a NaN among its
 * retained samples gives NaN in all five outputs.  What a dimension gives for which mi_mcmc_draw_stats has no defined answer on the composed slab
 * (a constant dimension) is whatever that function returns there. */
int mi_mcmc_draw_stats_ranked(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                              double* rhat, double* rhat_bulk, double* rhat_tail, double* ess_bulk, double* ess_tail, /* host [d], any may be NULL */
                              void* stream);
/* mi_mcmc_draw_stats_ranked with mi_mcmc_draw_stats_lags as the reducer of the composed slabs: K = min(max_lag, h - 1), h = floor(n_keep / 2), so the
 * bulk-ESS and tail-ESS of half-chains longer than 160 draws use every lag.  Argument checks: those of mi_mcmc_draw_stats_ranked (all six outputs
 * NULL: MI_ERR_BAD_ARG).  ended [d] (host, may be NULL): 1 only if all three ESS sums of the dimension ended -- bulk, the q05 and the q95 indicator. */
int mi_mcmc_draw_stats_ranked_lags(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains,
                                   uint32_t max_lag,
                                   double* rhat, double* rhat_bulk, double* rhat_tail, double* ess_bulk, double* ess_tail,
                                   uint8_t* ended /*[d]*/, void* stream);
int mi_mcmc_norm_ppf(const double* p, uint64_t n, double* z);   /* host arrays, host arithmetic, needs no device */

/* The log-posterior trace of a slab [n_keep][d][C] (in `mem`; a host slab is staged), on the device: out[t][c] = log K(x[t][:][c]), the target's own
 * log-kernel at every kept draw of every chain, d = target->d.  The chains' current state mi_chains.theta ([d][C]) is the case n_keep = 1.
 * target->prec / X / y live in target->mem, as for the samplers; kernel_hint is ignored.  out is [n_keep][C] in `mem` -- exactly a slab [n_keep][1][C],
 * so mi_mcmc_draw_stats, mi_mcmc_draw_stats_ranked, mi_mcmc_draws_quantiles and mi_mcmc_draws_covariance take it as it is, with d = 1.  A device slab:
 * the call returns after enqueueing on `stream` (with a target in host memory: once its arrays have been read).  A host slab: blocking.  Draws are
 * stored in the original space, and the value is the target's log-kernel there: no bounds, no Jacobian.  Workspace: the stream's cached one
 * (mi_mcmc_release_workspace) -- the packed matrix and the staged copies of a host slab, result and target.  No CPU path: no device is
 * MI_ERR_NO_DEVICE; what does not fit the free device memory is MI_ERR_OOM.
 * MI_ERR_BAD_ARG, before any HIP call: a NULL target, slab or out; a struct_size mismatch; d, n_keep or n_chains 0; n_keep or n_chains beyond 32 bits;
 * d > 65 536; DENSE / DIAG without prec; LOGISTIC / NORMAL_MODEL without their data or with n_rows = 0; NORMAL_MODEL with d != 2; an unknown kind.
 * MI_ERR_UNSUPPORTED: MI_TARGET_GAUSS_MIXTURE -- left out of this reducer on purpose (mi_mcmc_aees_run evaluates it).
 * DEFINITION (fp64, every operation rounded once, nothing contracted; exp / log: det_math.hpp).  x is the column, of d values.
 *   dot4(a, b)  four chains over the n terms: q[i % 4] = fma(a_i, b_i, q[i % 4]), i ascending, each from +0; the result is (q0 + q2) + (q1 + q3)
 *   sum4(a)     the same with q[i % 4] = q[i % 4] + a_i
 *   ISO           -0.5 * dot4(x, x)
 *   DIAG          w_i = prec_i * x_i;  -0.5 * dot4(x, w)
 *   DENSE         w_i = the fma chain over j ascending of P_ij * x_j, from +0 (row i of the row-major matrix AS GIVEN: symmetry is not assumed);
 *                 -0.5 * dot4(x, w)
 *   LOGISTIC      eta_r = the fma chain over j ascending of X_rj * x_j, from +0
 *                 softplus(eta) = eta > 0 ? eta + log(1 + exp(-eta)) : log(1 + exp(eta))
 *                 term_r = y_r * eta_r - softplus(eta_r);  ll = sum4(term) over the n_rows rows;  ll - 0.5 * dot4(x, x)
 *   NORMAL_MODEL  (mu, sigma) = x;  m2 = the chain fma(e, e, m2) over r ascending from +0, e = y_r - mu, n = (double)n_rows
 *                 -(n * (0.5 * LOG_2PI + log(sigma))) - m2 / (2 * (sigma * sigma))
 * The dense products run on v_mfma_f64_16x16x4_f64 with the contraction ascending -- the fma chain above -- and w / eta never reach memory
 * (mcmc_amd/csrc/draws_logk.hip).  The result depends on no grid, timing or atomic order, and has this ONE order for every d: it is the order of the
 * matrix-product route (d > 512), while for d <= 512 the samplers' internal energies use their routes' own blocked orders and may differ from this
 * value in the last bits.  Non-finite samples propagate by the IEEE rules through exactly these expressions, in their own column and nowhere else;
 * nothing is flagged or replayed. */
int mi_mcmc_draws_log_kernel(const mi_target* target, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t n_chains,
                             double* out /* [n_keep][C], in `mem` */, void* stream);

/* The pointwise log-likelihood of a slab [n_keep][d][C] (in `mem`; a host slab is staged) under a target that carries observations, and its fold over the
 * draws per observation, on the device: for every data row r the log pointwise predictive density lppd_r and the effective number of parameters
 * p_waic_r (WAIC, Watanabe 2010; Vehtari, Gelman and Gabry 2017), and on request the matrix ll itself.  It is the other fold of the product that
 * mi_mcmc_draws_log_kernel folds over the rows.  target->X / y live in target->mem; kernel_hint is ignored.  lppd_out, p_waic_out ([n_rows]) and
 * loglik_out ([n_rows][n_keep][C]) are in `mem`; any may be NULL.  Row r of loglik_out is a slab [n_keep][1][C] that mi_mcmc_draw_stats,
 * mi_mcmc_draw_stats_ranked, mi_mcmc_draws_quantiles and mi_mcmc_draws_covariance take as it is; PSIS-LOO does not need it copied out: mi_mcmc_draws_psis_loo
 * below forms and consumes it on the device, a group of rows at a time.  summary (HOST, 4
 * doubles, may be NULL) = {elpd_waic, p_waic, lppd, se_elpd}.  A device slab with summary == NULL: the call returns after enqueueing on `stream` (with
 * a target in host memory: once its arrays have been read).  A device slab with summary, or a host slab: blocking.  Workspace: the stream's cached
 * one (mi_mcmc_release_workspace) -- the packed matrix, the chunk partials (32 n_chunks bytes per padded row), and the staged copies of a host slab,
 * target and outputs.  No CPU path: no device is MI_ERR_NO_DEVICE; what does not fit the free device memory is MI_ERR_OOM.
 * MI_ERR_BAD_ARG, before any HIP call: a NULL target or slab; all four outputs NULL; a struct_size mismatch; d 0; n_keep or n_chains beyond 32 bits;
 * K = n_keep * n_chains < 2; d > 65 536; LOGISTIC / NORMAL_MODEL without their data or with n_rows = 0; NORMAL_MODEL with d != 2; an unknown kind.
 * MI_ERR_UNSUPPORTED: ISO / DIAG / DENSE / GAUSS_MIXTURE -- they have no observations.
 * DEFINITION (fp64, every operation rounded once, nothing contracted; exp / log / softplus: det_math.hpp).  K = n_keep * C; sample k = t * C + c is
 * column (t, c), x its d values.
 *   LOGISTIC      eta = the fma chain over j ascending of X_rj * x_j, from +0;  ll[r][k] = y_r * eta - softplus(eta)  -- term_r of
 *                 mi_mcmc_draws_log_kernel, the same bits
 *   NORMAL_MODEL  (mu, sigma) = x;  e = y_r - mu;  ll[r][k] = -(0.5 * LOG_2PI + log(sigma)) - (e * e) / (2 * (sigma * sigma))
 *   loglik_out[r][t][c] = ll[r][k]
 * THE ORDER of the sums over k, for every row r alike (the constants are part of the definition):
 *   chunks        the columns are cut into chunks of 2048: chunk b holds k = 2048 b .. min(K, 2048 b + 2048) - 1, n_b columns
 *   shift         sh_b = ll[r][2048 b], the chunk's first column
 *   slots         the column at offset o = k - 2048 b belongs to slot s = 16 ((o mod 128) div 32) + o mod 16, one of 64.  A slot takes its columns
 *                 ascending, from +0:  v = ll - sh_b;  S1 = S1 + v;  S2 = S2 + v * v;  A = A + exp(ll)
 *   tree          each of S1, S2, A: the 16 slots s = 16 w .. 16 w + 15 of w meet as u[i] = u[i] + u[i + 8] (i < 8), then + u[i + 4] (i < 4), + u[i + 2],
 *                 + u[i + 1]; the four w as (w0 + w1) + (w2 + w3)
 *   chunk moments mean_b = sh_b + S1 / n_b;  M2_b = S2 - (S1 * S1) / n_b  (n_b as a double)
 *   merge         chunk 0 starts (n, mean, M2, A) = (n_0, mean_0, M2_0, A_0); then b ascending: delta = mean_b - mean;  nn = n + n_b;
 *                 mean = mean + delta * (n_b / nn);  M2 = (M2 + M2_b) + (delta * delta) * ((n * n_b) / nn);  n = nn;  A = A + A_b
 *   lppd_r = log(A / (double)K);   p_waic_r = M2 / (double)(K - 1)  -- the sample variance of ll[r][:], from sums about a shift that is one of the
 *   values: no difference of two large numbers is formed
 *   summary       elpd_r = lppd_r - p_waic_r;  elpd_waic, p_waic, lppd: the plain sums over r ascending from +0 of elpd_r, p_waic_r, lppd_r;
 *                 m = elpd_waic / (double)n_rows;  v = the sum over r ascending of (elpd_r - m) * (elpd_r - m);
 *                 se_elpd = sqrt((double)n_rows * (v / (double)(n_rows - 1)))  -- NaN for n_rows = 1
 * The logistic product runs on v_mfma_f64_16x16x4_f64 with the contraction ascending; a workgroup owns 128 rows and one chunk, and ll reaches memory
 * only where loglik_out asks for it (mcmc_amd/csrc/draws_waic.hip).  The result depends on no device, grid, timing or atomic order.  Non-finite
 * draws propagate by the IEEE rules through exactly these expressions; nothing is filtered or flagged.  The numpy statement is mcmc_amd/waic.py. */
int mi_mcmc_draws_waic(const mi_target* target, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t n_chains,
                       double* lppd_out,    /* [n_rows] in `mem`, may be NULL */
                       double* p_waic_out,  /* [n_rows] in `mem`, may be NULL */
                       double* loglik_out,  /* [n_rows][n_keep][C] in `mem`, may be NULL */
                       double* summary,     /* HOST, 4 doubles, may be NULL */
                       void* stream);

/* PSIS-LOO: the Pareto-smoothed importance-sampling leave-one-out estimate elpd_loo_r of every data row r of a target that carries observations, and the
 * shape pareto_k_r of the generalised Pareto distribution fitted to the row's largest importance ratios, its reliability diagnostic (Vehtari, Gelman and
 * Gabry 2017; Vehtari, Simpson, Gelman, Yao and Gabry 2024; the fit: Zhang and Stephens 2009), of a slab [n_keep][d][C] on the device.  The matrix ll of
 * mi_mcmc_draws_waic never leaves the device: the rows are walked in consecutive groups of G (a multiple of 128 whose block ll [G][K] fits a budget of
 * 4 GiB, never less than 128, at most n_rows); a group's block is written by the WAIC kernels, every row of it is fully sorted by the radix sort of
 * mi_mcmc_draws_rank_transform, and mcmc_amd/csrc/draws_psis.hip reads the sorted rows.  Targets, target->mem, staging of a host slab / target and
 * MI_ERR_NO_DEVICE / MI_ERR_OOM / MI_ERR_UNSUPPORTED are those of mi_mcmc_draws_waic.  elpd_loo_out, pareto_k_out, lppd_out ([n_rows]) are in `mem`, any
 * may be NULL; lppd_out holds the bits of mi_mcmc_draws_waic's lppd_out.  summary (HOST, 5 doubles, may be NULL) = {elpd_loo, p_loo, lppd, se_elpd_loo,
 * n_bad}.  ALWAYS blocking (the sort waits for its digit histograms).  Workspace: the stream's cached one -- the block ll, the sort's two key images and
 * counts (its own budget of 2 GiB), the WAIC workspace of a group, and the staged copies of a host slab and target.
 * MI_ERR_BAD_ARG, before any HIP call: as mi_mcmc_draws_waic, with all four outputs NULL, and K = n_keep * n_chains < 25 (the tail would have fewer than
 * five values: nothing is fitted) or K >= 2^32.
 * DEFINITION (fp64, every operation rounded once, nothing contracted; exp / log: det_math.hpp; sqrt and division: IEEE).  For one data row r:
 *   sorted row    ll[r][k] is mi_mcmc_draws_waic's, the same bits; s_0 <= ... <= s_{K-1} its K values ascending by the key of mi_mcmc_draws_order_stats.
 *                 The importance ratios of leaving r out are exp(-ll): the largest come first.  Everything below is a function of the sorted row, hence
 *                 of the multiset of the values.  s_0 or s_{K-1} not finite: elpd_loo_r = pareto_k_r = NaN (the other rows are untouched)
 *   tail length   M = min(K div 5, m3), m3 the smallest integer with m3 * m3 >= 9 K (ceil(3 sqrt(K)), in integers).  5 <= M < K
 *   cutoff        d = s_0 - s_M;  cut = d > -708.3964185322641 ? d : -708.3964185322641 (log of the smallest normal double);  ec = exp(cut)
 *   exceedances   x_j = exp(s_0 - s_{M-j}) - ec, j = 1 .. M: ascending
 *   SUM           SUM(v_0 .. v_{n-1}), the one order of every sum over tail or body values: slot t (t < 256) takes v_t, v_{t+256}, ... ascending from +0;
 *                 the 256 slots meet as u[i] = u[i] + u[i + 128] (i < 128), then + u[i + 64] (i < 64), ..., + u[i + 1]
 *   fit           n = (double)M;  m = 30 + floor(sqrt(M)) (integer);  q = x_{(M + 2) div 4} (= x_{floor(M / 4 + 0.5)});  for j = 1 .. m:
 *                 b_j = (1 - sqrt((double)m / ((double)j - 0.5))) / (3 * q) + 1 / x_M;   k_j = SUM_i(log(1 - b_j * x_i)) / n  (i = 1 .. M, v_{i-1});
 *                 L_j = n * ((log(-(b_j / k_j)) - k_j) - 1);   w_j = 1 / (the sum over l = 1 .. m ascending from +0 of exp(L_l - L_j));
 *                 w_j >= 10 * 2^-52 ? kept : replaced by +0;  sw = the sum over j ascending from +0 of w_j;  bh = the sum over j ascending from +0 of
 *                 b_j * (w_j / sw);  k0 = SUM_i(log(1 - bh * x_i)) / n;  sigma = -(k0 / bh);  khat = (n * k0 + 5) / (n + 10)
 *   degenerate    !(q > 0), or khat not finite, or !(sigma > 0) -- ties that fill a quarter of the tail, a constant row --: nothing is smoothed, t_j is the raw
 *                 s_0 - s_{M-j}, and pareto_k_r = +inf
 *   smoothed tail otherwise, j = 1 .. M:  p = ((double)j - 0.5) / n;  lg = log(1 - p);  g = khat == 0 ? -(sigma * lg) : (sigma * (exp((-khat) * lg) - 1)) / khat;
 *                 lt = log(g + ec);  t_j = lt < 0 ? lt : 0  -- the truncation at the largest raw ratio; t_j replaces the log-ratio of s_{M-j}
 *   folds         Wt = SUM_j(exp(t_j));  Nt = SUM_j(exp(t_j + (s_{M-j} - s_0)))  (v_{j-1});  the body values e = 0 .. K - M - 1, exp(s_0 - s_{M+e}), in pieces
 *                 of 16 384: B = the sum over the pieces ascending from +0 of SUM(the piece);  W = B + Wt;  N = (double)(K - M) + Nt  (a body term of
 *                 the numerator is exp(0) = 1);  elpd_loo_r = (s_0 + log(N)) - log(W);  pareto_k_r = khat
 *   summary       elpd_loo, lppd: the plain sums over r ascending from +0 of elpd_loo_r, lppd_r;  p_loo = lppd - elpd_loo;  se_elpd_loo: se_elpd of
 *                 mi_mcmc_draws_waic on elpd_loo_r;  n_bad = the number of rows with !(pareto_k_r <= 0.7) (NaN and +inf count), as a double
 * log(1 - t) and exp(t) - 1 go through log and exp as written (det_math.hpp has no log1p / expm1); what that costs is measured in DESIGN.md 4.27.
 * The tail of a row is held in LDS up to 8 192 values and re-read from the sorted row beyond; the result depends on neither, nor on the groups, a
 * grid, timing or an atomic order.  The numpy statement is mcmc_amd/psis.py. */
int mi_mcmc_draws_psis_loo(const mi_target* target, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t n_chains,
                           double* elpd_loo_out,  /* [n_rows] in `mem`, may be NULL */
                           double* pareto_k_out,  /* [n_rows] in `mem`, may be NULL */
                           double* lppd_out,      /* [n_rows] in `mem`, may be NULL: the bits of mi_mcmc_draws_waic's lppd_out */
                           double* summary,       /* HOST, 5 doubles, may be NULL */
                           void* stream);

/* WAIC and PSIS-LOO of a pointwise log-likelihood matrix that the CALLER supplies -- the way to both for a user-defined device target
 * (mi_mcmc_target.hpp, mi_mcmc_tile_target.hpp) or a host callback target, which the two entries above do not take: who can sample a model with a
 * functor of their own can fill ll[r][k] with a kernel of their own (examples/user_loglik.hip), and the matrix need not leave the device.
 * loglik (in `mem`; a host matrix is staged whole into the stream's cached workspace) holds n_rows x K doubles, K = n_keep * n_chains, in one of two layouts: */
enum { MI_LOGLIK_ROWS = 0,   /* [n_rows][n_keep][C]: the layout of mi_mcmc_draws_waic's loglik_out                      */
       MI_LOGLIK_SLAB = 1 }; /* [n_keep][n_rows][C]: a draws slab whose "dimensions" are the observations -- what a
                                kernel with one thread per chain writes next to the draws                                 */
/* DEFINITION.  ll[r][k] is the caller's value at sample k = t * C + c.  After that nothing new is defined:
 *   mi_mcmc_loglik_waic      lppd_r, p_waic_r and summary = {elpd_waic, p_waic, lppd, se_elpd} are the section THE ORDER of mi_mcmc_draws_waic, unchanged:
 *                            chunks of 2 048, the chunk's first column as shift, 64 slots, tree, chunk moments, merge, summary.
 *   mi_mcmc_loglik_psis_loo  elpd_loo_r, pareto_k_r and summary = {elpd_loo, p_loo, lppd, se_elpd_loo, n_bad} are the section DEFINITION of
 *                            mi_mcmc_draws_psis_loo, unchanged; lppd_out carries the bits of mi_mcmc_loglik_waic's.
 * Both layouts describe the same matrix, so they give the same bits; fed mi_mcmc_draws_waic's loglik_out, the two entries give the bits of
 * mi_mcmc_draws_waic and mi_mcmc_draws_psis_loo.  The result depends on no device, grid, timing or atomic order; non-finite values propagate by the IEEE
 * rules through those expressions.  The numpy statements are mcmc_amd/waic.py (row_stats, summary) and mcmc_amd/psis.py (psis_ref).
 * The outputs ([n_rows]) are in `mem`, any may be NULL; summary is on the HOST, may be NULL.  mi_mcmc_loglik_waic on a device matrix with summary == NULL
 * returns after enqueueing on `stream`; with summary, or on a host matrix, it blocks.  mi_mcmc_loglik_psis_loo ALWAYS blocks (the sort waits for its
 * digit histograms).  The matrix is read where it lies: the sorter of mi_mcmc_draws_rank_transform takes it as its slab, nothing is copied or grouped
 * beyond the sorter's own groups (its budget of 2 GiB).  Workspace: the stream's cached one (mi_mcmc_release_workspace) -- the chunk partials (32 n_chunks
 * bytes per padded row), the results, the sort's key images and counts, the staged copy of a host matrix.  No CPU path: no device is MI_ERR_NO_DEVICE;
 * what does not fit the free device memory is MI_ERR_OOM, as are K or n_rows beyond 2^38 and a matrix of more than 2^40 values.
 * MI_ERR_BAD_ARG, before any HIP call, in this order: a NULL matrix; all outputs NULL; an unknown layout; n_rows = 0; n_keep or n_chains beyond 32 bits;
 * K < 2 (mi_mcmc_loglik_waic) or K < 25 (mi_mcmc_loglik_psis_loo); K >= 2^32 (mi_mcmc_loglik_psis_loo); MI_LOGLIK_SLAB with n_rows > 65 536, the bound on
 * the dimensions of a slab of mi_mcmc_draws_rank_transform (MI_LOGLIK_ROWS has no such bound). */
int mi_mcmc_loglik_waic(const double* loglik, int32_t layout, int32_t mem, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains,
                        double* lppd_out,    /* [n_rows] in `mem`, may be NULL */
                        double* p_waic_out,  /* [n_rows] in `mem`, may be NULL */
                        double* summary,     /* HOST, 4 doubles, may be NULL */
                        void* stream);
int mi_mcmc_loglik_psis_loo(const double* loglik, int32_t layout, int32_t mem, uint64_t n_rows, uint64_t n_keep, uint64_t n_chains,
                            double* elpd_loo_out,  /* [n_rows] in `mem`, may be NULL */
                            double* pareto_k_out,  /* [n_rows] in `mem`, may be NULL */
                            double* lppd_out,      /* [n_rows] in `mem`, may be NULL: the bits of mi_mcmc_loglik_waic's lppd_out */
                            double* summary,       /* HOST, 5 doubles, may be NULL */
                            void* stream);

/* BRIDGE SAMPLING: the log marginal likelihood log Z = log of the integral of K(theta) over R^d -- what Bayes factors and posterior model probabilities are
 * made of -- from the posterior draws of a slab [n_keep][d][C] and draws of a Gaussian proposal fitted to them (Meng and Wong 1996; Gronau et al. 2017, the
 * R package bridgesampling), on the device.  Three entries: the proposal (fit, draw, evaluate), the estimate (the iteration and its error terms) and their
 * composition for the built-in targets.  A user-defined or callback target calls the first, evaluates its own log-kernel on prop_out and on the
 * iteration part (as examples/user_loglik.hip does for ll), and calls the second.
 * NOTATION.  n_fit (0: n_keep div 2), 1 <= n_fit < n_keep.  The FIT PART is rows t < n_fit: a prefix slab [n_fit][d][C], K0 = n_fit * C samples.  The
 * ITERATION PART is rows t >= n_fit: a suffix slab [n_it][d][C], n_it = n_keep - n_fit, N1 = n_it * C, sample j = (t - n_fit) * C + c.  n_prop = N2
 * (0: N1) proposal draws.  seed: the Philox key.
 * ALL THREE always block, use the stream's cached workspace (mi_mcmc_release_workspace), stage a host slab (`mem`), and have no CPU path: no device is
 * MI_ERR_NO_DEVICE; a need beyond the free device memory is MI_ERR_OOM, as is a host without memory for the fit's three d x d matrices (S, L, Pg:
 * 24 d^2 bytes).  The PRACTICAL range of d is that of a dense precond_mat: the factorisations run on the device up to d = 3 840 (INV) / 7 680 (CHOL_LOWER)
 * and in O(d^3) loops on the calling thread beyond, minutes at d of ten thousand; d <= 65 536 is the bound of the slab reducers, not a promise of speed.
 * mi_mcmc_last_kernel() names the bridge kernels.
 * MI_ERR_BAD_ARG, before any HIP call: a NULL slab, input or target; all outputs NULL; d = 0 or d > 65 536; n_keep < 2; n_fit >= n_keep; K0 < 2 or N1 < 2;
 * N2 < 2; n_keep, n_chains or N2 beyond 32 bits; tol < 0 or NaN; n_eff < 0 or NaN; a struct_size mismatch; an unknown kind (and, for the target's own
 * arrays, what mi_mcmc_draws_log_kernel refuses).
 *
 * mi_mcmc_bridge_proposal.  DEFINITION (fp64, every operation rounded once, nothing contracted; log: det_math.hpp; LOG_2PI = 1.83787706640934548356):
 *   A  (mu, S) = mi_mcmc_draws_covariance's mean and cov of the prefix slab [n_fit][d][C]: the same bits.
 *   B  S holds a non-finite entry: status = 1.  Otherwise L = CHOL_LOWER(S), Pg = INV(S) (mi_mcmc_mat_cholesky_lower's / mi_mcmc_mat_inverse's routines);
 *      any entry of L or Pg non-finite, or any L_aa <= 0: status = 1 (K0 <= d, a NaN in the fit part).  Otherwise status = 0 and
 *      ldh = (the sum over a ascending from +0 of log(L_aa)) + (0.5 * (double)d) * LOG_2PI.
 *      status 1: every value of prop_out, logg_post_out, logg_prop_out, mean_out, cov_out and ldh is NaN; the call returns MI_OK.
 *   C  z^(i) = the d normals of Philox stream 7 (STREAM_BRIDGE, det_math.hpp) with "chain" i = 0 .. N2 - 1 and draw 0: element 8 b + 4 h + j (j < 4, h < 2)
 *      is component h of the Box-Muller pair of slot 4 b + j, as for every normal vector of the engine.
 *      y_a = mu_a + (the fma chain over b = 0 .. a ascending of L_ab * z_b, from +0);  prop_out[a][i] = y_a -- a slab [1][d][N2].
 *   D  for a column x:  e_a = x_a - mu_a;  w_a = the fma chain over b = 0 .. d - 1 ascending of Pg_ab * e_b, from +0 (row a of Pg AS COMPUTED: symmetry is
 *      not assumed);  logg(x) = (-0.5 * dot4(e, w)) - ldh, dot4 as defined for mi_mcmc_draws_log_kernel.
 *      logg_post_out[t - n_fit][c] = logg of column (t, c) of the iteration part;  logg_prop_out[i] = logg of the STORED (rounded) y^(i), not of z.
 * The products of C and D run on v_mfma_f64_16x16x4_f64 over the stage of mcmc_amd/csrc/draws_product.hpp with the contraction ascending; z is generated
 * and x centred on the way into LDS; w and L z never reach memory except through prop_out (mcmc_amd/csrc/draws_bridge.hip).  Without prop_out the
 * proposal is generated and consumed in groups of columns (a multiple of 128; never fewer than 16) whose block [d][g] fits a budget of 2 GiB.  No result depends on the
 * grouping, a grid, timing or an atomic order.  prop_out ([1][d][N2]), logg_post_out ([n_it][C]) and logg_prop_out ([N2]) are in `mem`; mean_out ([d]),
 * cov_out ([d * d]) and info (2 doubles: {status, ldh}) are HOST arrays; any may be NULL, not all. */
int mi_mcmc_bridge_proposal(const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t d, uint64_t n_chains, uint64_t n_fit, uint64_t n_prop, uint64_t seed,
                            double* prop_out,       /* [1][d][N2] in `mem`, may be NULL */
                            double* logg_post_out,  /* [n_it][C] in `mem`, may be NULL */
                            double* logg_prop_out,  /* [N2] in `mem`, may be NULL */
                            double* mean_out,       /* HOST, [d], may be NULL */
                            double* cov_out,        /* HOST, [d * d], may be NULL */
                            double* info,           /* HOST, 2 doubles {status, ldh}, may be NULL */
                            void* stream);

/* mi_mcmc_bridge_estimate: the iterative bridge estimator from the four log-density arrays, all in `mem`: logp_post, logg_post ([n_it][C]: the target's
 * log-kernel and the proposal's log-density at the iteration part) and logp_prop, logg_prop ([N2]: the same at the proposal draws).  n_prop 0: N1;
 * n_eff 0: (double)N1 -- the effective size of the iteration part, where the caller knows it; tol 0: 1e-10; max_iter 0: 1000.
 * DEFINITION (fp64, every operation rounded once, nothing contracted; exp / log: det_math.hpp; division: IEEE):
 *   setup      l1_j = logp_post_j - logg_post_j;  l2_i = logp_prop_i - logg_prop_i;  l* = the type-7 median of l1: mi_mcmc_draws_quantiles with p = 0.5 on
 *              the slab [n_it][1][C], the same bits;  s1 = n_eff / (n_eff + (double)N2);  s2 = (double)N2 / (n_eff + (double)N2);
 *              a_i = exp(l2_i - l*);  b_j = exp(l1_j - l*)
 *   SUMP(v)    the sum over the pieces of 16 384 values, ascending from +0, of SUM(piece) -- SUM the 256-slot sum, and the whole the body fold, of
 *              mi_mcmc_draws_psis_loo
 *   iteration  r = 1, it = 0; then:  num = SUMP_i(a_i / (s1 * a_i + s2 * r)) / (double)N2;  den = SUMP_j(1 / (s1 * b_j + s2 * r)) / (double)N1;
 *              r' = num / den;  it = it + 1;  rel = |r' - r| / |r'|;  r = r';  stop with status 3 when r is not finite or not > 0, else with status 0
 *              when rel <= tol, else with status 2 when it = max_iter
 *   logml      log(r) + l*
 *   errors     at the final r:  f1_i = a_i / (s1 * a_i + s2 * r);  f2_j = 1 / (s1 * b_j + s2 * r).  (mean, M2) of each by THE ORDER of mi_mcmc_draws_waic:
 *              chunks of 2 048, the chunk's first value as shift, 64 slots (S1, S2), tree, chunk moments, merge.
 *              cv1 = (M2_1 / (double)(N2 - 1)) / ((mean_1 * mean_1) * (double)N2);  cv2 likewise with f2 and N1
 *   summary    {logml, status, it, rel, l*, cv1, cv2, (double)N2}
 * f2_out ([n_it][C] in `mem`, may be NULL) = f2: a slab [n_it][1][C] that mi_mcmc_draw_stats takes with d = 1; with its ESS per chain the caller forms
 * Fruehwirth-Schnatter's relative mean-squared error of the estimate of Z, cv1 + ((double)n_it / ESS) * cv2 (= cv1 + (N1 / (C ESS)) * cv2), whose root
 * is the approximate standard error of logml.  Non-finite inputs propagate by the IEEE rules through exactly these expressions: l2 = -inf contributes 0,
 * nothing is filtered.  The pieces and chunks are workgroups; the host adds them in ascending order: no result depends on a grid, timing or an
 * atomic order.  The numpy statement of all three entries is mcmc_amd/bridge.py. */
int mi_mcmc_bridge_estimate(const double* logp_post, const double* logg_post, const double* logp_prop, const double* logg_prop, int32_t mem,
                            uint64_t n_it, uint64_t n_chains, uint64_t n_prop, double n_eff, double tol, uint64_t max_iter,
                            double* f2_out,   /* [n_it][C] in `mem`, may be NULL */
                            double* summary,  /* HOST, 8 doubles, may be NULL */
                            void* stream);

/* mi_mcmc_draws_bridge: the two entries above composed with logp = mi_mcmc_draws_log_kernel's DEFINITION, on the iteration part and on the proposal
 * draws (generated and consumed in groups, never copied out): the bits are those of making the three calls by hand.  d = target->d; target->prec / X / y
 * live in target->mem.  Targets: ISO / DIAG / DENSE / LOGISTIC -- their support is R^d.  MI_ERR_UNSUPPORTED: MI_TARGET_NORMAL_MODEL (sigma > 0: a Gaussian
 * proposal leaves the support) and MI_TARGET_GAUSS_MIXTURE.  status 1 of the proposal: summary = {NaN, 1, NaN, NaN, NaN, NaN, NaN, (double)N2}, f2_out,
 * mean_out and cov_out NaN, MI_OK. */
int mi_mcmc_draws_bridge(const mi_target* target, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t n_chains, uint64_t n_fit, uint64_t n_prop,
                         uint64_t seed, double n_eff, double tol, uint64_t max_iter,
                         double* f2_out,    /* [n_it][C] in `mem`, may be NULL */
                         double* mean_out,  /* HOST, [d], may be NULL */
                         double* cov_out,   /* HOST, [d * d], may be NULL */
                         double* summary,   /* HOST, 8 doubles, may be NULL */
                         void* stream);

/* Posterior predictive checks of a slab [n_keep][d][C] (in `mem`; a host slab is staged) under MI_TARGET_LOGISTIC, on the device: at every row r of
 * target->X and every sample k the success probability p[r][k] and a replicated outcome yrep[r][k] drawn from it, folded BOTH ways -- per row over the
 * draws (the posterior mean and variance of P(y = 1 | x_r) and the frequency of replicated successes) and per draw over the rows (the test statistic
 * "number of successes" and the log-likelihood of the replicate and of the observed y), and the posterior predictive p-values of the two (Gelman, Meng
 * and Stern 1996).  target->X (n_rows x d) / y live in target->mem; X need not be the matrix the chains were sampled on -- held-out rows or a grid of
 * new covariates will do -- and target->y may be NULL (prediction at covariates with no outcomes): then ll_obs_out and summary must be NULL.
 * kernel_hint is ignored.  Every output may be NULL; the per-row outputs and the per-draw outputs come from two kernels and only what is asked for is
 * launched.  Row r of prob_out is a slab [n_keep][1][C] that mi_mcmc_draw_stats, mi_mcmc_draws_quantiles, ... take as it is; so are t_rep_out,
 * ll_rep_out and ll_obs_out.  A device slab with summary == NULL: the call returns after enqueueing on `stream` (with a target in host memory: once its
 * arrays have been read).  A device slab with summary, or a host slab: blocking.  Workspace, MI_ERR_NO_DEVICE and MI_ERR_OOM: as mi_mcmc_draws_waic.
 * MI_ERR_BAD_ARG, before any HIP call: as mi_mcmc_draws_waic (a NULL target or slab; a struct_size mismatch; d 0; n_keep or n_chains beyond 32 bits;
 * K = n_keep * n_chains < 2; d > 65 536; LOGISTIC without X or with n_rows = 0; an unknown kind), and: all nine outputs NULL; y NULL together with
 * ll_obs_out or summary; n_rows >= 2^32 (the row index is a slot of the generator).
 * MI_ERR_UNSUPPORTED: MI_TARGET_NORMAL_MODEL -- left out ON PURPOSE for now: its replicates are normals on an element-wise route, a follow-up; ISO / DIAG /
 * DENSE / GAUSS_MIXTURE -- they carry no observations.
 * DEFINITION (fp64, every operation rounded once, nothing contracted; exp / log / sigmoid / softplus, the Philox block rng_block and u01: det_math.hpp).
 * K = n_keep * C; sample k = t * C + c is column (t, c), x its d values.
 *   eta[r][k]     the fma chain over j ascending of X_rj * x_j, from +0  -- the bits of mi_mcmc_draws_waic
 *   p[r][k]       sigmoid(eta):  eta >= 0 ? 1 / (1 + exp(-eta)) : e / (1 + e) with e = exp(eta)
 *   u[r][k]       u01(w.x, w.y), w = rng_block(seed, chain = k, draw = 0, slot = r, STREAM_PREDICT = 8); w.z and w.w are unused
 *   yrep[r][k]    (u < p) ? 1.0 : 0.0  -- a NaN p gives 0
 *   prob_out[r][t][c] = p[r][k];   yrep_out[r][t][c] = yrep[r][k]
 * PER ROW, over the draws: the section THE ORDER of mi_mcmc_draws_waic, word for word -- chunks of 2048, the chunk's first column as shift, 64 slots,
 * tree, chunk moments, merge -- with p where ll stood:  sh_b = p[r][2048 b];  v = p - sh_b;  S1 = S1 + v;  S2 = S2 + v * v;  A = A + yrep  (where
 * A + exp(ll) stood: a sum of zeros and ones, exact in any order).
 *   p_mean_r = mean;   p_var_r = M2 / (double)(K - 1);   rep_freq_r = A / (double)K
 * PER DRAW, over the rows: sum4 of mi_mcmc_draws_log_kernel -- four chains q[r % 4], r ascending, each from +0, the result (q0 + q2) + (q1 + q3):
 *   t_rep_k  = sum4_r(yrep[r][k])                                   the number of replicated successes, an exact integer
 *   ll_rep_k = sum4_r(yrep[r][k] * eta - softplus(eta))             term_r of mi_mcmc_draws_log_kernel with the replicate as its y
 *   ll_obs_k = sum4_r(y_r * eta - softplus(eta))                    the bits of the ll part of mi_mcmc_draws_log_kernel's LOGISTIC value
 * SUMMARY = {t_obs, ppp_t, ppp_dev, t_rep_mean}:  t_obs = the plain sum of y_r over r ascending from +0;  ppp_t = (double)#{k : t_rep_k >= t_obs} /
 * (double)K;  ppp_dev = (double)#{k : ll_rep_k <= ll_obs_k} / (double)K -- the draws whose replicated deviance is at least the realised one;
 * t_rep_mean = (double)(sum_k t_rep_k) / (double)K.  The two counts and the integer sum are exact, so their order is free; a comparison with a NaN
 * counts as false.
 * Both products run on v_mfma_f64_16x16x4_f64 with the contraction ascending (mcmc_amd/csrc/draws_predict.hip); both kernels form yrep[r][k] from the
 * same (seed, r, k, bits of eta), so t_rep_out[t][c] is the sum over r of yrep_out[r][t][c], and rep_freq_out[r] the sum over (t, c) divided by K, exactly.
 * Non-finite draws propagate by the IEEE rules through exactly these expressions, in their own column and nowhere else; the result depends on no
 * device, grid, timing or atomic order.  The numpy statement is mcmc_amd/predict.py. */
int mi_mcmc_draws_predict(const mi_target* target, const double* draws_kdc, int32_t mem, uint64_t n_keep, uint64_t n_chains, uint64_t seed,
                          double* p_mean_out,    /* [n_rows] in `mem`, may be NULL */
                          double* p_var_out,     /* [n_rows] in `mem`, may be NULL */
                          double* rep_freq_out,  /* [n_rows] in `mem`, may be NULL */
                          double* prob_out,      /* [n_rows][n_keep][C] in `mem`, may be NULL: row r is a slab [n_keep][1][C] */
                          double* yrep_out,      /* [n_rows][n_keep][C] in `mem`, 0.0 / 1.0, may be NULL */
                          double* t_rep_out,     /* [n_keep][C] in `mem`, may be NULL: a slab [n_keep][1][C] */
                          double* ll_rep_out,    /* [n_keep][C] in `mem`, may be NULL */
                          double* ll_obs_out,    /* [n_keep][C] in `mem`, may be NULL; needs target->y */
                          double* summary,       /* HOST, 4 doubles, may be NULL; needs target->y */
                          void* stream);

/* (The diagnostics the GPU tests and the measurement tools use -- mi_probe_* -- are not part of this library: they live in
 * libmi_mcmc_probes.so, declared in mcmc_amd/csrc/mi_mcmc_probes.h.) */

#ifdef __cplusplus
}
#endif
#endif /* MI_MCMC_H */
