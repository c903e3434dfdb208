"""The Python statement of the C boundary: the constants and struct mirrors of include/mi_mcmc.h and one prototype table for
libmi_mcmc.so (include/mi_mcmc.h and the mi_mcmc_test_* hooks of mcmc_amd/csrc/mi_mcmc_probes.h) and libmi_mcmc_probes.so (the mi_probe_* of
that header).  mcmc_amd.lib() / probes_lib() apply the table once, when they load; tests/test_abi_prototypes.py holds it to the headers.

The mapping from a C parameter: int, int32_t, uint32_t, uint64_t, double -> the ctypes type of that name; a pointer to a struct mirrored here ->
POINTER(that class); every other pointer and the four function-pointer typedefs -> c_void_p (takes a Python int, None, byref(x), a ctypes array,
a CFUNCTYPE object; refuses numpy scalars and arrays: addresses are Python ints, what _ptr returns)."""
import ctypes as C

MI_OK, MI_ERR_BAD_ARG, MI_ERR_HIP, MI_ERR_UNSUPPORTED, MI_ERR_OOM, MI_ERR_NO_DEVICE = range(6)
TARGET_GAUSS_ISO, TARGET_GAUSS_DIAG, TARGET_GAUSS_DENSE, TARGET_LOGISTIC, TARGET_NORMAL_MODEL = 1, 2, 3, 4, 5
TARGET_GAUSS_MIXTURE = 6                  # value only: mcmc::aees alone (mixture_target builds one)
MEM_HOST, MEM_DEVICE = 0, 1
KERNEL_AUTO, KERNEL_ELEMENTWISE_1LANE, KERNEL_ELEMENTWISE_4LANE, KERNEL_NUTS_LOCKSTEP = 0, 1, 2, 3   # mi_kernel_hint
KERNEL_HMC_TWO_WAVES_PER_SIMD, KERNEL_HMC_ONE_WAVE_PER_SIMD, KERNEL_HMC_SPLIT2, KERNEL_HMC_SPLIT4, KERNEL_HMC_SPLIT4_TWO_WAVES = 4, 5, 6, 7, 8
KERNEL_NUTS_TICK_LOCAL, KERNEL_NUTS_REG, KERNEL_NUTS_SPLIT, KERNEL_LITERAL, KERNEL_NUTS_DYN, KERNEL_NUTS_MEMO, KERNEL_NUTS_MEMO_INTICK = 9, 10, 11, 12, 13, 14, 15
STATS_ALL_LAGS = 0xFFFFFFFF
RANK_AVERAGE, RANK_NORMAL = 0, 1
RANK_SPLIT, RANK_FOLD = 1, 2
LOGLIK_ROWS, LOGLIK_SLAB = 0, 1
GEMM_PLAIN, GEMM_DENSE_M, GEMM_BOUNDED = 0, 1, 2       # the variants of hmc / mala / rwmh on the matrix-product route (test_gemm_need_bytes)


class mi_target(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("d", C.c_uint64),
                ("prec", C.c_void_p), ("X", C.c_void_p), ("y", C.c_void_p),
                ("n_rows", C.c_uint64), ("mem", C.c_int32), ("kernel_hint", C.c_int32)]


class mi_settings(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("vals_bound", C.c_int32),
                ("rng_seed_value", C.c_uint64), ("lower_bounds", C.c_void_p),
                ("upper_bounds", C.c_void_p), ("n_burnin_draws", C.c_uint64),
                ("n_keep_draws", C.c_uint64), ("n_leap_steps", C.c_uint64),
                ("step_size", C.c_double), ("precond_mat", C.c_void_p),
                ("n_adapt_draws", C.c_uint64), ("target_accept_rate", C.c_double),
                ("max_tree_depth", C.c_uint64), ("gamma_val", C.c_double),
                ("t0_val", C.c_double), ("kappa_val", C.c_double), ("n_fp_steps", C.c_uint64)]


class mi_chains(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mem", C.c_int32), ("n_chains", C.c_uint64),
                ("chain0", C.c_uint64), ("theta", C.c_void_p), ("draws", C.c_void_p),
                ("n_accept", C.c_void_p), ("step_size", C.c_void_p), ("n_leapfrogs", C.c_void_p),
                ("nuts_depth", C.c_void_p), ("draw0", C.c_uint64), ("nuts_adapt_state", C.c_void_p), ("mass_diag", C.c_void_p),
                ("n_leapfrogs_executed", C.c_void_p)]


class mi_de_settings(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("jumps", C.c_int32), ("n_pop", C.c_uint64), ("par_b", C.c_double),
                ("par_gamma_jump", C.c_double), ("par_gamma", C.c_double), ("initial_lb", C.c_void_p), ("initial_ub", C.c_void_p)]


class mi_populations(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mem", C.c_int32), ("n_populations", C.c_uint64), ("population0", C.c_uint64),
                ("initial_vals", C.c_void_p), ("population", C.c_void_p), ("draws", C.c_void_p), ("n_accept", C.c_void_p),
                ("draw0", C.c_uint64)]


class mi_aees_settings(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_rings", C.c_uint32), ("n_initial_draws", C.c_uint64), ("par_scale", C.c_double),
                ("cov_mat", C.c_void_p), ("ee_prob_par", C.c_double), ("temper_vec", C.c_void_p), ("temper_len", C.c_uint64)]


class mi_aees_runs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mem", C.c_int32), ("n_runs", C.c_uint64), ("run0", C.c_uint64),
                ("initial_vals", C.c_void_p), ("draws", C.c_void_p), ("final_states", C.c_void_p), ("n_accept", C.c_void_p),
                ("n_ee_accept", C.c_void_p)]


_i, _i32, _u32, _u64, _f64, _p, _str = C.c_int, C.c_int32, C.c_uint32, C.c_uint64, C.c_double, C.c_void_p, C.c_char_p
_T, _S, _Ch = C.POINTER(mi_target), C.POINTER(mi_settings), C.POINTER(mi_chains)
_DS, _Po, _AS, _AR = C.POINTER(mi_de_settings), C.POINTER(mi_populations), C.POINTER(mi_aees_settings), C.POINTER(mi_aees_runs)

# name -> (restype, [argtypes]), in the headers' order
PROTOTYPES = {
    "mi_settings_default": (None, [_S]),
    "mi_mcmc_last_error": (_str, []),
    "mi_mcmc_last_kernel": (_str, []),
    "mi_mcmc_version": (_i, []),
    "mi_mcmc_device_count": (_i, []),
    "mi_mcmc_run_user_target": (_i, [_i, _u64, _p, _p, _u64, _S, _Ch, _p]),
    "mi_mcmc_run_user_target_v": (_i, [_i, _u64, _p, _p, _u64, _i, _S, _Ch, _p]),
    "mi_mcmc_run_tile_target": (_i, [_i, _u64, _i, _i, _u64, _p, _p, _u64, _i, _S, _Ch, _p]),
    "mi_mcmc_release_workspace": (_i, [_p, _i, _p]),
    "mi_mcmc_hmc_run": (_i, [_T, _S, _Ch, _p]),
    "mi_mcmc_mala_run": (_i, [_T, _S, _Ch, _p]),
    "mi_mcmc_nuts_run": (_i, [_T, _S, _Ch, _p]),
    "mi_mcmc_rwmh_run": (_i, [_T, _S, _Ch, _p]),
    "mi_mcmc_rmhmc_run": (_i, [_T, _S, _Ch, _p]),
    "mi_mcmc_hmc_run_mass_adapted": (_i, [_T, _S, _Ch, _u32, _p, _p]),
    "mi_mcmc_hmc_run_mass_adapted_dense": (_i, [_T, _S, _Ch, _u32, _p, _p]),
    "mi_mcmc_mala_run_mass_adapted_dense": (_i, [_T, _S, _Ch, _u32, _p, _p]),
    "mi_mcmc_hmc_run_mass_adapted_per_chain": (_i, [_T, _S, _Ch, _u32, _f64, _p, _p]),
    "mi_mcmc_hmc_run_callback": (_i, [_p, _u64, _p, _p, _S, _p, _p]),
    "mi_mcmc_mala_run_callback": (_i, [_p, _u64, _p, _p, _S, _p, _p]),
    "mi_mcmc_nuts_run_callback": (_i, [_p, _u64, _p, _p, _S, _p, _p, _p]),
    "mi_mcmc_rwmh_run_callback": (_i, [_p, _u64, _p, _p, _S, _p, _p]),
    "mi_mcmc_rmhmc_run_callback": (_i, [_p, _u64, _p, _p, _p, _p, _S, _p, _p]),
    "mi_de_settings_default": (None, [_DS]),
    "mi_mcmc_de_run": (_i, [_T, _S, _DS, _Po, _p]),
    "mi_mcmc_de_run_callback": (_i, [_p, _u64, _p, _p, _S, _DS, _p, _p]),
    "mi_aees_settings_default": (None, [_AS]),
    "mi_mcmc_aees_run": (_i, [_T, _S, _AS, _AR, _p]),
    "mi_mcmc_aees_run_callback": (_i, [_p, _u64, _p, _p, _S, _AS, _p, _p, _p, _p]),
    "mi_mcmc_mat_inverse": (_i, [_p, _u64, _p]),
    "mi_mcmc_mat_cholesky_lower": (_i, [_p, _u64, _p]),
    "mi_mcmc_shard_bounds": (None, [_u64, _u32, _u32, _p, _p]),
    "mi_mcmc_allgather_draws": (_i, [_p, _u32, _u32, _p, _u64, _u64, _u64, _p, _p, _p]),
    "mi_mcmc_allgather_draws_ragged": (_i, [_p, _u32, _u32, _p, _u64, _u64, _u64, _p, _p, _p]),
    "mi_mcmc_merge_shards": (_i, [_p, _u32, _u64, _u64, _u64, _p, _p]),
    "mi_mcmc_allgather_draws_rank_major": (_i, [_p, _u32, _u32, _p, _u64, _u64, _u64, _p, _p]),
    "mi_mcmc_rank_major_index": (_u64, [_u64, _u32, _u64, _u64, _u64, _u64, _u64]),
    "mi_mcmc_allgather_draws_begin": (_i, [_p, _u32, _u32, _p, _u64, _u64, _u64, _u64, _u64, _p, _p, _p]),
    "mi_mcmc_allgather_draws_wait": (_i, [_p, _p, _i]),
    "mi_mcmc_draws_to_chain_major": (_i, [_p, _u64, _u64, _u64, _p]),
    "mi_mcmc_draws_to_chain_major_device": (_i, [_p, _u64, _u64, _u64, _p, _p]),
    "mi_mcmc_draw_stats": (_i, [_p, _i32, _u64, _u64, _u64, _p, _p, _p, _p, _p]),
    "mi_mcmc_draw_stats_lags": (_i, [_p, _i32, _u64, _u64, _u64, _u32, _p, _p, _p, _p, _p, _p]),
    "mi_mcmc_draws_covariance": (_i, [_p, _i32, _u64, _u64, _u64, _p, _p, _p]),
    "mi_mcmc_draw_stats_nested": (_i, [_p, _i32, _u64, _u64, _u64, _u64, _p, _p, _p, _p, _p, _p, _p]),
    "mi_mcmc_draw_stats_nested_ranked": (_i, [_p, _i32, _u64, _u64, _u64, _u64, _p, _p, _p, _p]),
    "mi_mcmc_draws_order_stats": (_i, [_p, _i32, _u64, _u64, _u64, _p, _u32, _p, _p]),
    "mi_mcmc_draws_quantiles": (_i, [_p, _i32, _u64, _u64, _u64, _p, _u32, _p, _p]),
    "mi_mcmc_draws_rank_transform": (_i, [_p, _i32, _u64, _u64, _u64, _i32, _u32, _p, _p]),
    "mi_mcmc_draw_stats_ranked": (_i, [_p, _i32, _u64, _u64, _u64, _p, _p, _p, _p, _p, _p]),
    "mi_mcmc_draw_stats_ranked_lags": (_i, [_p, _i32, _u64, _u64, _u64, _u32, _p, _p, _p, _p, _p, _p, _p]),
    "mi_mcmc_norm_ppf": (_i, [_p, _u64, _p]),
    "mi_mcmc_draws_log_kernel": (_i, [_T, _p, _i32, _u64, _u64, _p, _p]),
    "mi_mcmc_draws_waic": (_i, [_T, _p, _i32, _u64, _u64, _p, _p, _p, _p, _p]),
    "mi_mcmc_draws_psis_loo": (_i, [_T, _p, _i32, _u64, _u64, _p, _p, _p, _p, _p]),
    "mi_mcmc_loglik_waic": (_i, [_p, _i32, _i32, _u64, _u64, _u64, _p, _p, _p, _p]),
    "mi_mcmc_loglik_psis_loo": (_i, [_p, _i32, _i32, _u64, _u64, _u64, _p, _p, _p, _p, _p]),
    "mi_mcmc_bridge_proposal": (_i, [_p, _i32, _u64, _u64, _u64, _u64, _u64, _u64, _p, _p, _p, _p, _p, _p, _p]),
    "mi_mcmc_bridge_estimate": (_i, [_p, _p, _p, _p, _i32, _u64, _u64, _u64, _f64, _f64, _u64, _p, _p, _p]),
    "mi_mcmc_draws_bridge": (_i, [_T, _p, _i32, _u64, _u64, _u64, _u64, _u64, _f64, _f64, _u64, _p, _p, _p, _p, _p]),
    "mi_mcmc_draws_predict": (_i, [_T, _p, _i32, _u64, _u64, _u64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    # mcmc_amd/csrc/mi_mcmc_probes.h: the probes (their own library) ...
    "mi_probe_mfma_f64": (_i, [_p, _p, _p, _p]),
    "mi_probe_math": (_i, [_i, _p, _u64, _p, _p]),
    "mi_probe_math2": (_i, [_i, _p, _p, _u64, _p]),
    "mi_probe_normals": (_i, [_u64, _u64, _u32, _u32, _u64, _p]),
    "mi_probe_normals_variant": (_i, [_i, _u64, _u64, _u32, _u32, _u64, _p]),
    "mi_probe_math_kc2": (_i, [_i, _p, _u64, _p, _p]),
    "mi_probe_math2_kc2": (_i, [_i, _p, _p, _u64, _p]),
    "mi_probe_normals_kc2": (_i, [_i, _u64, _u64, _u32, _u32, _u64, _p]),
    "mi_probe_uniform": (_i, [_u64, _u64, _u32, _u32, _p]),
    "mi_probe_fp64_peak": (_i, [_i, _i, _p]),
    "mi_probe_mfma_cycles": (_i, [_i, _i, _i, _p, _p]),
    # ... and the test hooks (defined in the shipped library)
    "mi_mcmc_test_set_grid_cap": (None, [_u32]),
    "mi_mcmc_test_set_linalg_stage_bytes": (None, [_u32]),
    "mi_mcmc_test_linalg_computed": (_u64, []),
    "mi_mcmc_test_linalg_computed_on_device": (_u64, []),
    "mi_mcmc_test_set_gemm_nuts_ws_bytes": (None, [_u64]),
    "mi_mcmc_test_gemm_nuts_ranges": (_u64, []),
    "mi_mcmc_test_gemm_nuts_last_ticks": (None, [_p, _p, _p]),
    "mi_mcmc_test_gemm_nuts_tick_ceiling": (_u64, [_u32, _u64, _i]),
    "mi_mcmc_test_gemm_nuts_chain_bytes": (_u64, [_u32, _u32, _u32]),
    "mi_mcmc_test_gemm_nuts_fixed_bytes": (_u64, [_u32, _u32]),
    "mi_mcmc_test_gemm_nuts_bounded_chain_bytes": (_u64, [_u32, _u32, _u32]),
    "mi_mcmc_test_gemm_nuts_range_chains": (_u64, [_u64, _u64, _u64, _u64]),
    "mi_mcmc_test_set_gemm_graph": (None, [_i]),
    "mi_mcmc_test_set_gemm_ws_bytes": (None, [_u64]),
    "mi_mcmc_test_gemm_need_bytes": (_u64, [_u32, _u32, _u64, _i, _i]),
    "mi_mcmc_test_set_rank_ws_bytes": (None, [_u64]),
    "mi_mcmc_test_rank_dim_bytes": (_u64, [_u64, _u64, _u32, _i]),
    "mi_mcmc_test_rank_dims_per_group": (_u64, [_u64, _u64, _u64, _u32, _i]),
    "mi_mcmc_test_rank_counts": (None, [_p, _p]),
    "mi_mcmc_test_logk_plan": (None, [_i32, _u64, _u64, _u64, _u64, _i, _i, _p]),
    "mi_mcmc_test_draw_stats_last": (None, [_p]),
    "mi_mcmc_test_draw_stats_lags_last": (None, [_p]),
    "mi_mcmc_test_stats_host": (None, [_p, _u64, _u64, _u64, _p, _u32, _u64, _p, _p, _p]),
    "mi_mcmc_test_waic_plan": (None, [_i32, _u64, _u64, _u64, _u64, _i, _i, _i, _p]),
    "mi_mcmc_test_set_psis_ll_bytes": (None, [_u64]),
    "mi_mcmc_test_set_psis_lds_tail": (None, [_u32]),
    "mi_mcmc_test_psis_plan": (None, [_i32, _u64, _u64, _u64, _u64, _i, _i, _p]),
    "mi_mcmc_test_loglik_plan": (None, [_i32, _u64, _u64, _u64, _i, _i, _p]),
    "mi_mcmc_test_set_bridge_prop_bytes": (None, [_u64]),
}

TEST_HOOKS = [n for n in PROTOTYPES if n.startswith("mi_mcmc_test_")]         # declared in mi_mcmc_probes.h, defined in the shipped library
PROBE_EXPORTS = [n for n in PROTOTYPES if n.startswith("mi_probe_")]          # libmi_mcmc_probes.so: test / measurement infrastructure
EXPORTS = [n for n in PROTOTYPES if n not in TEST_HOOKS and n not in PROBE_EXPORTS]   # include/mi_mcmc.h


def declare(handle, names, path):
    """Set restype and argtypes of every name on a loaded library; a name the library lacks is an error."""
    for name in names:
        try:
            fn = getattr(handle, name)
        except AttributeError:
            raise AttributeError(f"{path} does not export {name}: rebuild it (`make -C mcmc_amd/csrc`)") from None
        fn.restype, fn.argtypes = PROTOTYPES[name]
    return handle
