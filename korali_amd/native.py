"""ctypes binding of the korali_amd C-ABI (include/korali_amd.h).

The product path: every call here goes to the HIP kernels in
korali_amd/libkorali_amd.so.  There is no CPU fallback — if the library is
missing or no HIP device is present, construction raises.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libkorali_amd.so")
if os.environ.get("KORALI_AMD_LIB_VARIANT"):  # A/B builds (libkorali_amd_<variant>.so, same sources, other -D flags)
    LIB_PATH = os.path.join(_PKG, f"libkorali_amd_{os.environ['KORALI_AMD_LIB_VARIANT']}.so")
_LIB = None

MU_TYPES = {"logarithmic": 0, "linear": 1, "equal": 2, "proportional": 3}
OBJECTIVES = {"negative rosenbrock": 0, "negative ackley": 1, "negative sphere": 2,
              "rosenbrock": 0, "ackley": 1, "sphere": 2}
COV_MODES = {"exact": 0, "mfma": 1}


class KoraliDeviceError(RuntimeError):
    pass


class _CmaesCfg(C.Structure):
    _fields_ = [
        ("variable_count", C.c_size_t), ("population_size", C.c_size_t), ("mu_value", C.c_size_t),
        ("mu_type", C.c_int), ("initial_sigma_cumulation_factor", C.c_double),
        ("initial_damp_factor", C.c_double), ("initial_cumulative_covariance", C.c_double),
        ("is_sigma_bounded", C.c_int), ("diagonal_covariance", C.c_int), ("mirrored_sampling", C.c_int),
        ("max_infeasible_resamplings", C.c_double),
        ("lower_bound", C.POINTER(C.c_double)), ("upper_bound", C.POINTER(C.c_double)),
        ("initial_value", C.POINTER(C.c_double)), ("initial_std", C.POINTER(C.c_double)),
        ("min_std_update", C.POINTER(C.c_double)),
        ("normal_seed", C.c_uint64), ("uniform_seed", C.c_uint64), ("cov_mode", C.c_int), ("device", C.c_int),
        ("store_bdz", C.c_int), ("eigen_device_chase", C.c_int), ("shard_rank", C.c_int), ("shard_count", C.c_int),
        ("use_gradients", C.c_int), ("gradient_step_size", C.c_double),
        ("granularity", C.POINTER(C.c_double)),
        ("constraint_count", C.c_size_t), ("viability_population_size", C.c_size_t),
        ("viability_mu_value", C.c_size_t), ("max_covariance_matrix_corrections", C.c_double),
        ("target_success_rate", C.c_double), ("covariance_matrix_adaption_strength", C.c_double),
        ("global_success_learning_rate", C.c_double),
    ]


# int (*)(const double *X, size_t rows, size_t N, const size_t *ids, double *out, void *ctx)
CONSTRAINT_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t),
                            C.POINTER(C.c_double), C.c_void_p)


class _TmcmcCfg(C.Structure):
    _fields_ = [
        ("variable_count", C.c_size_t), ("population_size", C.c_size_t), ("max_chain_length", C.c_double),
        ("default_burn_in", C.c_double), ("target_cov", C.c_double), ("covariance_scaling", C.c_double),
        ("min_annealing_exponent_update", C.c_double), ("max_annealing_exponent_update", C.c_double),
        ("prior_min", C.POINTER(C.c_double)), ("prior_max", C.POINTER(C.c_double)),
        ("prior_distribution", C.POINTER(C.c_int)), ("distribution_count", C.c_size_t),
        ("prior_seeds", C.POINTER(C.c_uint64)), ("multinomial_seed", C.c_uint64),
        ("multivariate_seed", C.c_uint64), ("uniform_seed", C.c_uint64), ("likelihood", C.c_int),
        ("device", C.c_int), ("per_generation_burn_in", C.POINTER(C.c_double)),
        ("per_generation_burn_in_count", C.c_size_t), ("shard_rank", C.c_int), ("shard_count", C.c_int),
        ("version", C.c_int), ("step_size", C.c_double), ("domain_extension_factor", C.c_double),
        ("prior_kind", C.POINTER(C.c_int)),
    ]


class _TmcmcHierarchical(C.Structure):
    _fields_ = [
        ("mode", C.c_int), ("prior_count", C.c_size_t), ("kind", C.POINTER(C.c_int)),
        ("param_index", C.POINTER(C.c_int)), ("param_const", C.POINTER(C.c_double)),
        ("group_count", C.c_size_t), ("group_size", C.POINTER(C.c_size_t)), ("row_width", C.c_size_t),
        ("rows", C.POINTER(C.c_double)), ("log_prior", C.POINTER(C.c_double)),
    ]


class _TmcmcHierTheta(C.Structure):
    _fields_ = [
        ("prior_count", C.c_size_t), ("kind", C.POINTER(C.c_int)), ("param_index", C.POINTER(C.c_int)),
        ("param_const", C.POINTER(C.c_double)), ("psi_rows", C.c_size_t), ("psi_width", C.c_size_t),
        ("psi_db", C.POINTER(C.c_double)), ("sub_rows", C.c_size_t), ("sub_db", C.POINTER(C.c_double)),
        ("sub_log_prior", C.POINTER(C.c_double)),
    ]


HIER_MODES = {"psi": 0, "thetanew": 1}
PRIOR_KINDS = {"uniform": 0, "normal": 1, "exponential": 2, "laplace": 3, "cauchy": 4, "lognormal": 5}


class _DeaCfg(C.Structure):
    _fields_ = [
        ("variable_count", C.c_size_t), ("population_size", C.c_size_t),
        ("lower_bound", C.POINTER(C.c_double)), ("upper_bound", C.POINTER(C.c_double)),
        ("crossover_rate", C.c_double), ("mutation_rate", C.c_double), ("mutation_rule", C.c_int),
        ("parent_rule", C.c_int), ("accept_rule", C.c_int), ("fix_infeasible", C.c_int),
        ("normal_seed", C.c_uint64), ("uniform_seed", C.c_uint64), ("window_words", C.c_size_t),
        ("max_windows", C.c_size_t), ("device", C.c_int),
    ]


DEA_MUTATION_RULES = {"fixed": 0, "self adaptive": 1}
DEA_PARENT_RULES = {"random": 0, "best": 1}
DEA_ACCEPT_RULES = {"best": 0, "greedy": 1, "iterative": 2, "improved": 3}

class _MocmaesCfg(C.Structure):
    _fields_ = [
        ("variable_count", C.c_size_t), ("population_size", C.c_size_t), ("mu_value", C.c_size_t),
        ("num_objectives", C.c_size_t),
        ("lower_bound", C.POINTER(C.c_double)), ("upper_bound", C.POINTER(C.c_double)),
        ("initial_value", C.POINTER(C.c_double)), ("initial_sdev", C.POINTER(C.c_double)),
        ("evolution_path_adaption_strength", C.c_double), ("covariance_learning_rate", C.c_double),
        ("target_success_rate", C.c_double), ("success_learning_rate", C.c_double), ("parent_order", C.c_int),
        ("multinormal_seed", C.c_uint64), ("uniform_seed", C.c_uint64), ("window_blocks", C.c_size_t),
        ("max_windows", C.c_size_t), ("archive_rows", C.c_size_t), ("device", C.c_int),
    ]


class _NestedCfg(C.Structure):
    _fields_ = [
        ("variable_count", C.c_size_t), ("number_live_points", C.c_size_t), ("batch_size", C.c_size_t),
        ("add_live_points", C.c_int), ("resampling_method", C.c_int), ("proposal_update_frequency", C.c_size_t),
        ("ellipsoidal_scaling", C.c_double), ("min_log_evidence_delta", C.c_double),
        ("max_effective_sample_size", C.c_double), ("max_log_likelihood", C.c_double),
        ("prior_min", C.POINTER(C.c_double)), ("prior_max", C.POINTER(C.c_double)), ("prior_kind", C.POINTER(C.c_int)),
        ("lower_bound", C.POINTER(C.c_double)), ("upper_bound", C.POINTER(C.c_double)),
        ("uniform_seed", C.c_uint64), ("normal_seed", C.c_uint64), ("shuffle_seed", C.c_uint64),
        ("likelihood", C.c_int), ("window_tries", C.c_size_t), ("max_windows", C.c_size_t), ("device", C.c_int),
    ]


class _McmcCfg(C.Structure):
    _fields_ = [
        ("variable_count", C.c_size_t), ("burn_in", C.c_longlong), ("leap", C.c_longlong),
        ("rejection_levels", C.c_longlong), ("use_adaptive_sampling", C.c_int),
        ("non_adaption_period", C.c_longlong), ("chain_covariance_scaling", C.c_double),
        ("max_samples", C.c_size_t), ("initial_mean", C.POINTER(C.c_double)), ("initial_sdev", C.POINTER(C.c_double)),
        ("probability_kernel", C.c_int), ("prior_min", C.POINTER(C.c_double)), ("prior_max", C.POINTER(C.c_double)),
        ("prior_kind", C.POINTER(C.c_int)), ("normal_seed", C.c_uint64), ("uniform_seed", C.c_uint64),
        ("window_candidates", C.c_size_t), ("device", C.c_int),
    ]


MCMC_KERNELS = {"gaussian": 1}
MCMC_STOP = {1: "Max Samples", 2: "Max Model Evaluations"}

NESTED_METHODS = {"box": 0, "ellipse": 1, "multi ellipse": 2}
NESTED_TERMINATION = {1: "Min Log Evidence Delta", 2: "Max Effective Sample Size", 4: "Max Log Likelihood"}

MOCMAES_PARENT_ORDERS = {"descending": 0, "recorded": 1}
MOCMAES_OBJECTIVES = {"negative_rosenbrock_and_sphere": 0, "negative_rosenbrock_and_two_spheres": 1}

EXPORTED = [
    "kg_last_error", "kg_abi_version", "kg_device_count",
    "kg_cmaes_create", "kg_cmaes_destroy", "kg_cmaes_initialize", "kg_cmaes_sample", "kg_cmaes_eval_builtin",
    "kg_cmaes_sample_eval",
    "kg_cmaes_get_candidates", "kg_cmaes_set_fitness", "kg_cmaes_set_log_posterior", "kg_cmaes_update", "kg_cmaes_generation",
    "kg_cmaes_begin_sample", "kg_cmaes_wait_termination_fields", "kg_cmaes_set_gradients", "kg_cmaes_update_partial", "kg_cmaes_update_finalize",
    "kg_cmaes_shard_row_count", "kg_cmaes_update_rows",
    "kg_cmaes_synchronize", "kg_cmaes_field_size", "kg_cmaes_get_field", "kg_cmaes_set_field",
    "kg_cmaes_get_fields", "kg_cmaes_get_sorting_index", "kg_cmaes_get_rng", "kg_cmaes_set_rng", "kg_cmaes_device_ptr",
    "kg_cmaes_stream", "kg_cmaes_profile", "kg_cmaes_profile_read", "kg_cmaes_profile_mark",
    "kg_cmaes_set_constraints", "kg_cmaes_prepare_constrained", "kg_cmaes_population_size",
    "kg_dea_create", "kg_dea_destroy", "kg_dea_initialize", "kg_dea_prepare", "kg_dea_eval_builtin",
    "kg_dea_get_candidates", "kg_dea_set_fitness", "kg_dea_update", "kg_dea_generation", "kg_dea_synchronize",
    "kg_dea_field_size", "kg_dea_get_field", "kg_dea_set_field", "kg_dea_get_rng", "kg_dea_set_rng",
    "kg_dea_windows", "kg_dea_profile", "kg_dea_profile_read",
    "kg_mocmaes_create", "kg_mocmaes_destroy", "kg_mocmaes_initialize", "kg_mocmaes_prepare",
    "kg_mocmaes_eval_builtin", "kg_mocmaes_get_candidates", "kg_mocmaes_set_values", "kg_mocmaes_update",
    "kg_mocmaes_generation", "kg_mocmaes_synchronize", "kg_mocmaes_field_size", "kg_mocmaes_get_field",
    "kg_mocmaes_set_field", "kg_mocmaes_get_rng", "kg_mocmaes_set_rng", "kg_mocmaes_diagnostics",
    "kg_mocmaes_profile", "kg_mocmaes_profile_read",
    "kg_nested_create", "kg_nested_destroy", "kg_nested_first_generation", "kg_nested_generation",
    "kg_nested_prepare", "kg_nested_get_candidates", "kg_nested_set_evaluations", "kg_nested_eval_builtin",
    "kg_nested_process", "kg_nested_finalize", "kg_nested_field_size", "kg_nested_get_field", "kg_nested_set_field",
    "kg_nested_get_rng", "kg_nested_set_rng", "kg_nested_diagnostics", "kg_nested_profile",
    "kg_nested_profile_read", "kg_nested_synchronize", "kg_nested_permutation",
    "kg_mcmc_create", "kg_mcmc_destroy", "kg_mcmc_run", "kg_mcmc_propose", "kg_mcmc_get_candidate", "kg_mcmc_decide",
    "kg_mcmc_end_generation", "kg_mcmc_database", "kg_mcmc_field_size", "kg_mcmc_get_field", "kg_mcmc_set_field",
    "kg_mcmc_get_rng", "kg_mcmc_set_rng", "kg_mcmc_diagnostics", "kg_mcmc_profile", "kg_mcmc_profile_read",
    "kg_mcmc_synchronize",
    "kg_supervisor_create", "kg_supervisor_destroy", "kg_supervisor_hyperparameter_count",
    "kg_supervisor_set_training_data", "kg_supervisor_train", "kg_supervisor_forward",
    "kg_supervisor_backward_direct", "kg_supervisor_field_size", "kg_supervisor_get_field",
    "kg_supervisor_set_field", "kg_supervisor_get_scalar", "kg_supervisor_set_scalar",
    "kg_supervisor_synchronize", "kg_supervisor_profile", "kg_supervisor_profile_read",
    "kg_tmcmc_create", "kg_tmcmc_destroy", "kg_tmcmc_generation", "kg_tmcmc_synchronize", "kg_tmcmc_field_size",
    "kg_tmcmc_get_field", "kg_tmcmc_set_field", "kg_tmcmc_get_rng", "kg_tmcmc_set_rng", "kg_tmcmc_prepare",
    "kg_tmcmc_evaluate", "kg_tmcmc_process", "kg_tmcmc_advance", "kg_tmcmc_get_pending",
    "kg_tmcmc_process_partial", "kg_tmcmc_process_finalize", "kg_tmcmc_device_ptr", "kg_tmcmc_stream", "kg_tmcmc_evaluate_prior", "kg_tmcmc_get_candidates", "kg_tmcmc_set_evaluations",
    "kg_tmcmc_set_gradients", "kg_tmcmc_set_hierarchical", "kg_tmcmc_hierarchical_loglik",
    "kg_tmcmc_set_hierarchical_theta", "kg_tmcmc_theta_denominators", "kg_tmcmc_theta_loglik",
    "kg_tmcmc_profile", "kg_tmcmc_profile_read", "kg_debug_mt_jump", "kg_debug_multinomial", "kg_debug_cartpole",
    "kg_debug_cartpole_at",
    "kg_debug_host_tridiag", "kg_debug_host_tridiag_seq", "kg_debug_host_chase",
    "kg_debug_cholesky", "kg_debug_prior_logdens",
    "kg_debug_mt_open", "kg_debug_mt_close", "kg_debug_mt_import", "kg_debug_mt_count_blocks",
    "kg_debug_mt_polar_normals", "kg_debug_mt_consume_normals", "kg_debug_mt_consume_normals_dev",
    "kg_debug_mt_uniforms", "kg_debug_mt_peek_uniforms", "kg_debug_mt_consume_words_dev",
    "kg_debug_mt_prefetch", "kg_debug_mt_polar_normals_ahead", "kg_debug_mt_join", "kg_debug_mt_export_gsl",
    "kg_debug_mt_state",
    # VRACER (korali_amd/vracer.py binds their argument types)
    "kg_vracer_create", "kg_vracer_create_discrete", "kg_vracer_destroy", "kg_vracer_hyperparameter_count", "kg_vracer_field_size",
    "kg_vracer_get_field", "kg_vracer_set_field", "kg_vracer_get_scalar", "kg_vracer_set_scalar",
    "kg_vracer_run_policy", "kg_vracer_set_action_noise", "kg_vracer_environment_step", "kg_vracer_train_policy",
    "kg_vracer_train_policy_minibatch", "kg_vracer_training_step", "kg_vracer_test_episodes", "kg_vracer_rescale_states", "kg_vracer_synchronize", "kg_vracer_stream",
    "kg_vracer_profile", "kg_vracer_profile_read", "kg_vracer_save_state", "kg_vracer_load_state",
    "kg_vracer_train_pending", "kg_vracer_host_launch", "kg_vracer_host_act", "kg_vracer_host_feed",
]


def lib():
    """Load libkorali_amd.so (raises if it is absent: no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise KoraliDeviceError(f"{LIB_PATH} not built; run `python -m korali_amd._build` (hipcc, gfx950)")
        L = C.CDLL(LIB_PATH)
        vp, sz, dp, cp, ip = C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.c_char_p, C.c_int
        L.kg_last_error.restype = cp
        L.kg_abi_version.restype = ip
        L.kg_device_count.argtypes = [C.POINTER(C.c_int)]
        # the entries every solver handle has (class _Handle)
        for p in ("kg_cmaes", "kg_dea", "kg_mocmaes", "kg_nested", "kg_mcmc", "kg_tmcmc"):
            getattr(L, p + "_field_size").argtypes = [vp, cp, C.POINTER(sz)]
            getattr(L, p + "_get_field").argtypes = [vp, cp, dp, sz]
            getattr(L, p + "_set_field").argtypes = [vp, cp, dp, sz]
            getattr(L, p + "_get_rng").argtypes = [vp, ip, vp]
            getattr(L, p + "_set_rng").argtypes = [vp, ip, vp]
            getattr(L, p + "_profile").argtypes = [vp, ip]
            getattr(L, p + "_profile_read").argtypes = [vp, cp, dp, C.POINTER(sz)]
        L.kg_cmaes_create.argtypes = [C.POINTER(_CmaesCfg), C.POINTER(vp)]
        for f in ("kg_cmaes_destroy", "kg_cmaes_initialize", "kg_cmaes_sample", "kg_cmaes_synchronize",
                  "kg_cmaes_begin_sample"):
            getattr(L, f).argtypes = [vp]
        L.kg_cmaes_eval_builtin.argtypes = [vp, ip]
        L.kg_cmaes_sample_eval.argtypes = [vp, ip]
        L.kg_cmaes_get_candidates.argtypes = [vp, dp, sz]
        L.kg_cmaes_set_fitness.argtypes = [vp, dp]
        L.kg_cmaes_set_log_posterior.argtypes = [vp, dp]
        L.kg_cmaes_set_gradients.argtypes = [vp, dp]
        L.kg_cmaes_update.argtypes = [vp, sz]
        L.kg_cmaes_update_partial.argtypes = [vp, sz]
        L.kg_cmaes_update_finalize.argtypes = [vp, sz]
        L.kg_cmaes_shard_row_count.argtypes = [vp, C.POINTER(sz)]
        L.kg_cmaes_update_rows.argtypes = [vp, sz]
        L.kg_debug_mt_jump.argtypes = [vp, C.c_uint64, vp]
        L.kg_debug_multinomial.argtypes = [C.c_uint64, C.c_size_t, C.c_uint, vp, C.c_size_t, vp, vp]
        L.kg_debug_cartpole.argtypes = [ip, vp, vp, sz, sz, vp, vp]
        L.kg_debug_cartpole_at.argtypes = [ip, vp, vp, vp, sz, sz, vp, vp, vp]
        L.kg_debug_host_tridiag.argtypes = [sz, vp, vp, vp, vp, vp]
        L.kg_debug_host_tridiag_seq.argtypes = [sz, sz, vp, vp, vp, vp, vp]
        L.kg_debug_host_chase.argtypes = [sz, vp, vp, C.c_int, sz, vp, vp, vp, sz, vp, vp]
        L.kg_debug_cholesky.argtypes = [C.c_int, sz, vp, vp, vp]
        L.kg_debug_prior_logdens.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, vp, sz, vp, vp]
        L.kg_debug_mt_open.argtypes = [ip, sz, vp, C.POINTER(vp)]
        L.kg_debug_mt_close.argtypes = [vp]
        L.kg_debug_mt_import.argtypes = [vp, vp]
        L.kg_debug_mt_count_blocks.argtypes = [vp, sz, C.POINTER(sz)]
        L.kg_debug_mt_polar_normals.argtypes = [vp, sz, sz, sz, sz, vp, sz, vp, C.POINTER(sz)]
        L.kg_debug_mt_consume_normals.argtypes = [vp, sz, sz, ip]
        L.kg_debug_mt_consume_normals_dev.argtypes = [vp, C.c_ulonglong, sz]
        L.kg_debug_mt_uniforms.argtypes = [vp, sz, vp]
        L.kg_debug_mt_peek_uniforms.argtypes = [vp, sz, vp]
        L.kg_debug_mt_consume_words_dev.argtypes = [vp, C.c_ulonglong]
        L.kg_debug_mt_prefetch.argtypes = [vp, sz]
        L.kg_debug_mt_polar_normals_ahead.argtypes = [vp, sz, sz, vp, sz, C.POINTER(ip)]
        L.kg_debug_mt_join.argtypes = [vp, vp, sz]
        L.kg_debug_mt_export_gsl.argtypes = [vp, vp]
        L.kg_debug_mt_state.argtypes = [vp, vp, C.POINTER(C.c_ulonglong)]
        L.kg_cmaes_generation.argtypes = [vp, sz, ip]
        L.kg_cmaes_get_sorting_index.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.kg_cmaes_get_fields.argtypes = [vp, C.POINTER(cp), sz, dp]
        L.kg_cmaes_wait_termination_fields.argtypes = [vp, dp]
        L.kg_cmaes_set_constraints.argtypes = [vp, CONSTRAINT_FN, vp]
        L.kg_cmaes_prepare_constrained.argtypes = [vp, sz]
        L.kg_cmaes_population_size.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
        L.kg_cmaes_device_ptr.argtypes = [vp, cp, C.POINTER(vp)]
        L.kg_cmaes_stream.argtypes = [vp, C.POINTER(vp)]
        L.kg_cmaes_profile_mark.argtypes = [vp, cp, ip]
        L.kg_dea_create.argtypes = [C.POINTER(_DeaCfg), C.POINTER(vp)]
        for f in ("kg_dea_destroy", "kg_dea_initialize", "kg_dea_synchronize"):
            getattr(L, f).argtypes = [vp]
        for f in ("kg_dea_prepare", "kg_dea_update"):
            getattr(L, f).argtypes = [vp, sz]
        L.kg_dea_eval_builtin.argtypes = [vp, ip]
        L.kg_dea_generation.argtypes = [vp, sz, ip]
        L.kg_dea_get_candidates.argtypes = [vp, dp, sz]
        L.kg_dea_set_fitness.argtypes = [vp, dp]
        L.kg_dea_windows.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
        L.kg_mocmaes_create.argtypes = [C.POINTER(_MocmaesCfg), C.POINTER(vp)]
        for f in ("kg_mocmaes_destroy", "kg_mocmaes_initialize", "kg_mocmaes_synchronize"):
            getattr(L, f).argtypes = [vp]
        for f in ("kg_mocmaes_prepare", "kg_mocmaes_update"):
            getattr(L, f).argtypes = [vp, sz]
        L.kg_mocmaes_eval_builtin.argtypes = [vp, ip]
        L.kg_mocmaes_generation.argtypes = [vp, sz, ip]
        L.kg_mocmaes_get_candidates.argtypes = [vp, dp, sz]
        L.kg_mocmaes_set_values.argtypes = [vp, dp]
        L.kg_mocmaes_diagnostics.argtypes = [vp] + [C.POINTER(sz)] * 4
        L.kg_nested_create.argtypes = [C.POINTER(_NestedCfg), C.POINTER(vp)]
        for f in ("kg_nested_destroy", "kg_nested_first_generation", "kg_nested_eval_builtin", "kg_nested_finalize",
                  "kg_nested_synchronize"):
            getattr(L, f).argtypes = [vp]
        L.kg_nested_generation.argtypes = [vp, sz, C.POINTER(ip)]
        L.kg_nested_prepare.argtypes = [vp, sz]
        L.kg_nested_get_candidates.argtypes = [vp, dp, sz]
        L.kg_nested_set_evaluations.argtypes = [vp, dp]
        L.kg_nested_process.argtypes = [vp, sz, C.POINTER(ip), C.POINTER(ip)]
        L.kg_nested_diagnostics.argtypes = [vp] + [C.POINTER(sz)] * 3
        L.kg_nested_permutation.argtypes = [C.c_uint64, sz, C.POINTER(sz)]
        L.kg_mcmc_create.argtypes = [C.POINTER(_McmcCfg), C.POINTER(vp)]
        for f in ("kg_mcmc_destroy", "kg_mcmc_synchronize"):
            getattr(L, f).argtypes = [vp]
        L.kg_mcmc_run.argtypes = [vp, sz, sz, sz, C.POINTER(sz), C.POINTER(ip)]
        L.kg_mcmc_propose.argtypes = [vp, sz]
        L.kg_mcmc_get_candidate.argtypes = [vp, dp]
        L.kg_mcmc_decide.argtypes = [vp, sz, C.c_double, C.POINTER(ip)]
        L.kg_mcmc_end_generation.argtypes = [vp, sz]
        L.kg_mcmc_database.argtypes = [vp, dp, dp, C.POINTER(sz)]
        L.kg_mcmc_diagnostics.argtypes = [vp] + [C.POINTER(sz)] * 3
        L.kg_tmcmc_create.argtypes = [C.POINTER(_TmcmcCfg), C.POINTER(vp)]
        for f in ("kg_tmcmc_destroy", "kg_tmcmc_synchronize", "kg_tmcmc_evaluate", "kg_tmcmc_evaluate_prior"):
            getattr(L, f).argtypes = [vp]
        L.kg_tmcmc_device_ptr.argtypes = [vp, cp, C.POINTER(vp)]
        L.kg_tmcmc_stream.argtypes = [vp, C.POINTER(vp)]
        for f in ("kg_tmcmc_generation", "kg_tmcmc_prepare", "kg_tmcmc_process", "kg_tmcmc_process_partial",
                  "kg_tmcmc_process_finalize"):
            getattr(L, f).argtypes = [vp, sz]
        L.kg_tmcmc_get_candidates.argtypes = [vp, dp, sz]
        L.kg_tmcmc_set_evaluations.argtypes = [vp, dp, dp]
        L.kg_tmcmc_set_gradients.argtypes = [vp, dp, dp]
        L.kg_tmcmc_set_hierarchical.argtypes = [vp, C.POINTER(_TmcmcHierarchical)]
        L.kg_tmcmc_hierarchical_loglik.argtypes = [vp, dp, sz, dp]
        L.kg_tmcmc_set_hierarchical_theta.argtypes = [vp, C.POINTER(_TmcmcHierTheta)]
        L.kg_tmcmc_theta_denominators.argtypes = [vp, dp, sz]
        L.kg_tmcmc_theta_loglik.argtypes = [vp, dp, sz, dp, dp]
        L.kg_tmcmc_advance.argtypes = [vp, sz, C.POINTER(sz)]
        L.kg_tmcmc_get_pending.argtypes = [vp, C.POINTER(C.c_ubyte)]
        _LIB = L
    return _LIB


def check(rc):
    if rc != 0:
        raise KoraliDeviceError(lib().kg_last_error().decode())


def device_count():
    n = C.c_int(0)
    check(lib().kg_device_count(C.byref(n)))
    return n.value


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _vec(x, n, default):
    if x is None:
        return np.full(n, default, dtype=np.float64)
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)))
    return a


class _Handle:
    """What every solver handle of the C-ABI has under its prefix (kg_dea, ...):
    destroy, the named fields, the 5000-byte generator states, the stage timer."""

    _prefix = None

    def _fn(self, name):
        return getattr(self._L, self._prefix + name)

    def close(self):
        if getattr(self, "h", None):
            self._fn("_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def field_size(self, name):
        n = C.c_size_t()
        check(self._fn("_field_size")(self.h, name.encode(), C.byref(n)))
        return n.value

    def __getitem__(self, name):
        n = self.field_size(name)
        out = np.empty(n)
        check(self._fn("_get_field")(self.h, name.encode(), _dptr(out), n))
        return out

    def __setitem__(self, name, value):
        a = np.ascontiguousarray(np.asarray(value, dtype=np.float64).reshape(-1))
        check(self._fn("_set_field")(self.h, name.encode(), _dptr(a), a.size))

    def _get_rng(self, which):
        buf = C.create_string_buffer(5000)
        check(self._fn("_get_rng")(self.h, int(which), buf))
        return buf.raw

    def _set_rng(self, which, state):
        assert len(state) == 5000
        buf = C.create_string_buffer(bytes(state), 5000)
        check(self._fn("_set_rng")(self.h, int(which), buf))

    def profile(self, enable=True):
        check(self._fn("_profile")(self.h, int(enable)))

    def profile_read(self, stage):
        ms, n = C.c_double(), C.c_size_t()
        check(self._fn("_profile_read")(self.h, stage.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


class CmaesDevice(_Handle):
    """One CMA-ES solver instance resident on one MI355X (kg_cmaes_t)."""

    _prefix = "kg_cmaes"

    def __init__(self, N, lam, mu=0, mu_type="Logarithmic", lower_bound=None, upper_bound=None, initial_value=None,
                 initial_std=None, min_std_update=None, normal_seed=0, uniform_seed=0, cov_mode="exact",
                 is_sigma_bounded=False, diagonal=False, max_infeasible_resamplings=float("inf"),
                 initial_sigma_cumulation_factor=-1.0, initial_damp_factor=-1.0,
                 initial_cumulative_covariance=-1.0, device=0, store_bdz=False, eigen_chase="host", shard_rank=0,
                 shard_count=1, mirrored=False, gradient_step_size=None, granularity=None, constraints=None,
                 viability_population_size=2, viability_mu_value=0, max_covariance_matrix_corrections=1e6,
                 target_success_rate=0.1818, covariance_matrix_adaption_strength=0.1,
                 global_success_learning_rate=0.2):
        """constraints: CCMA-ES constraint functions c(x) -> float (x: the
        sample as a list), evaluated in list order per sample; a sample
        violates c when c(x) > 0 (beyond the viability boundary)."""
        L = lib()
        self.N, self._lam_cfg = int(N), int(lam)
        self.mu = int(mu) if mu else self._lam_cfg // 2
        self._arrays = [
            _vec(lower_bound, self.N, -np.inf), _vec(upper_bound, self.N, np.inf),
            _vec(initial_value, self.N, np.nan), _vec(initial_std, self.N, np.nan),
            _vec(min_std_update, self.N, 0.0), _vec(granularity, self.N, 0.0),
        ]
        cfg = _CmaesCfg()
        cfg.variable_count, cfg.population_size, cfg.mu_value = self.N, self._lam_cfg, int(mu)
        cfg.mu_type = MU_TYPES[mu_type.lower()] if isinstance(mu_type, str) else int(mu_type)
        cfg.initial_sigma_cumulation_factor = initial_sigma_cumulation_factor
        cfg.initial_damp_factor = initial_damp_factor
        cfg.initial_cumulative_covariance = initial_cumulative_covariance
        cfg.is_sigma_bounded, cfg.diagonal_covariance = int(is_sigma_bounded), int(diagonal)
        cfg.mirrored_sampling = int(bool(mirrored))
        cfg.use_gradients, cfg.gradient_step_size = int(gradient_step_size is not None), float(gradient_step_size or 0.0)
        cfg.max_infeasible_resamplings = float(max_infeasible_resamplings)
        (cfg.lower_bound, cfg.upper_bound, cfg.initial_value, cfg.initial_std,
         cfg.min_std_update, cfg.granularity) = [_dptr(a) for a in self._arrays]
        cfg.normal_seed, cfg.uniform_seed = int(normal_seed), int(uniform_seed)
        cfg.cov_mode = COV_MODES[cov_mode.lower()] if isinstance(cov_mode, str) else int(cov_mode)
        cfg.device, cfg.store_bdz = int(device), int(store_bdz)
        cfg.eigen_device_chase = 1 if eigen_chase == "device" else 0
        cfg.shard_rank, cfg.shard_count = int(shard_rank), int(shard_count)
        self.shard_rank, self.shard_count = int(shard_rank), max(1, int(shard_count))
        self._constraints = list(constraints or [])
        cfg.constraint_count = len(self._constraints)
        cfg.viability_population_size, cfg.viability_mu_value = int(viability_population_size), int(viability_mu_value)
        cfg.max_covariance_matrix_corrections = float(max_covariance_matrix_corrections)
        cfg.target_success_rate = float(target_success_rate)
        cfg.covariance_matrix_adaption_strength = float(covariance_matrix_adaption_strength)
        cfg.global_success_learning_rate = float(global_success_learning_rate)
        h = C.c_void_p()
        check(L.kg_cmaes_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._L = L
        if self._constraints:
            funcs = self._constraints

            def cb(X, rows, n, ids, out, ctx):
                try:
                    nc = len(funcs)
                    for r in range(rows):
                        x = [float(X[r * n + d]) for d in range(n)]
                        for c in range(nc):
                            out[r * nc + c] = float(funcs[c](x))
                    return 0
                except Exception:  # reported as a failed evaluation by the library
                    return 1

            self._cfn = CONSTRAINT_FN(cb)  # kept alive with the handle
            check(L.kg_cmaes_set_constraints(self.h, self._cfn, None))

    @property
    def lam(self):
        """the current population size (CCMA-ES: the viability one in its viability regime)"""
        n = C.c_size_t()
        check(self._L.kg_cmaes_population_size(self.h, C.byref(n), None))
        return n.value

    def prepare_constrained(self, generation):
        """CCMA-ES: regime check, draw, constraint evaluation and handling
        (kg_cmaes_prepare_constrained); then evaluate the current population."""
        check(self._L.kg_cmaes_prepare_constrained(self.h, int(generation)))

    # stages
    def initialize(self):
        check(self._L.kg_cmaes_initialize(self.h))

    def sample(self):
        check(self._L.kg_cmaes_sample(self.h))

    def evaluate(self, objective):
        check(self._L.kg_cmaes_eval_builtin(self.h, OBJECTIVES[objective.lower()] if isinstance(objective, str)
                                            else int(objective)))

    def sample_eval(self, objective):
        """sample() + evaluate(objective) in one call (kg_cmaes_sample_eval)."""
        check(self._L.kg_cmaes_sample_eval(self.h, OBJECTIVES[objective.lower()] if isinstance(objective, str)
                                           else int(objective)))

    def update(self, generation):
        check(self._L.kg_cmaes_update(self.h, int(generation)))

    def update_partial(self, generation):
        check(self._L.kg_cmaes_update_partial(self.h, int(generation)))

    def update_finalize(self, generation):
        check(self._L.kg_cmaes_update_finalize(self.h, int(generation)))

    def shard_row_count(self):
        """Doubles per rank block of the "Shard Rows" all-gather (exact-order
        sharded update; waits for the packing)."""
        n = C.c_size_t(0)
        check(self._L.kg_cmaes_shard_row_count(self.h, C.byref(n)))
        return int(n.value)

    def update_rows(self, generation):
        check(self._L.kg_cmaes_update_rows(self.h, int(generation)))

    def begin_sample(self):
        """Enqueue the next generation's generator prefetch and the first
        eigendecomposition phases (workspace only) — what the korali engine
        does right after each update (kg_cmaes_begin_sample)."""
        check(self._L.kg_cmaes_begin_sample(self.h))

    def generation(self, generation, objective):
        obj = OBJECTIVES[objective.lower()] if isinstance(objective, str) else int(objective)
        check(self._L.kg_cmaes_generation(self.h, int(generation), obj))

    def synchronize(self):
        check(self._L.kg_cmaes_synchronize(self.h))

    # host-callback objectives
    def candidates(self):
        X = np.empty((self.lam, self.N))
        check(self._L.kg_cmaes_get_candidates(self.h, _dptr(X), self.N))
        return X

    def _fitness_arg(self, F):
        F = np.ascontiguousarray(F, dtype=np.float64)
        if F.shape != (self.lam,):
            raise ValueError("fitness vector has shape %s, expected (%d,)" % (F.shape, self.lam))
        return F

    def set_fitness(self, F):
        F = self._fitness_arg(F)
        check(self._L.kg_cmaes_set_fitness(self.h, _dptr(F)))

    def set_gradients(self, G):
        """Use Gradient Information: every sample's gradient (lambda x N)."""
        G = np.ascontiguousarray(G, dtype=np.float64)
        if G.size != self.lam * self.N:
            raise ValueError(f"set_gradients: expected {self.lam} x {self.N} gradients, got {G.shape}")
        check(self._L.kg_cmaes_set_gradients(self.h, _dptr(G)))

    def set_log_posterior(self, F):
        """Bayesian problems: F(x) = logPosterior, -inf allowed."""
        F = self._fitness_arg(F)
        check(self._L.kg_cmaes_set_log_posterior(self.h, _dptr(F)))

    def get_prefix(self, name, n):
        """The first n doubles of an exchange buffer ("Shard Rows")."""
        out = np.empty(int(n))
        check(self._L.kg_cmaes_get_field(self.h, name.encode(), _dptr(out), int(n)))
        return out

    def sorting_index(self):
        out = np.empty(self.lam, dtype=np.uint64)
        check(self._L.kg_cmaes_get_sorting_index(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def get_rng(self, which):
        return self._get_rng(which)

    def set_rng(self, which, state):
        self._set_rng(which, state)

    def device_ptr(self, name):
        p = C.c_void_p()
        check(self._L.kg_cmaes_device_ptr(self.h, name.encode(), C.byref(p)))
        return p.value

    def stream(self):
        p = C.c_void_p()
        check(self._L.kg_cmaes_stream(self.h, C.byref(p)))
        return p.value

    def profile_mark(self, stage, phase):
        """kg_cmaes_profile_mark: phase 0 begins, 1 ends a caller-bracketed
        stage on the handle's stream; returns the C-ABI status (1: an end
        without a begin)."""
        return int(self._L.kg_cmaes_profile_mark(self.h, stage.encode(), int(phase)))


class DeaDevice(_Handle):
    """One Optimizer/DEA (differential evolution) instance on one MI355X
    (kg_dea_t), bit-exact to the reference's DEA.cpp.base.  Generator indices
    for rng_state / set_rng_state: 0 Normal (kept, never drawn from), 1 Uniform."""

    _prefix = "kg_dea"

    def __init__(self, N, P, lower_bound, upper_bound, crossover_rate=0.9, mutation_rate=0.5, mutation_rule="Fixed",
                 parent_rule="Random", accept_rule="Greedy", fix_infeasible=True, normal_seed=0, uniform_seed=0,
                 window_words=0, max_windows=0, device=0):
        L = lib()
        self.N, self.P = int(N), int(P)
        self._arrays = [_vec(lower_bound, self.N, np.nan), _vec(upper_bound, self.N, np.nan)]
        cfg = _DeaCfg()
        cfg.variable_count, cfg.population_size = self.N, self.P
        cfg.lower_bound, cfg.upper_bound = [_dptr(a) for a in self._arrays]
        cfg.crossover_rate, cfg.mutation_rate = float(crossover_rate), float(mutation_rate)
        cfg.mutation_rule = DEA_MUTATION_RULES[mutation_rule.lower()] if isinstance(mutation_rule, str) else int(mutation_rule)
        cfg.parent_rule = DEA_PARENT_RULES[parent_rule.lower()] if isinstance(parent_rule, str) else int(parent_rule)
        cfg.accept_rule = DEA_ACCEPT_RULES[accept_rule.lower()] if isinstance(accept_rule, str) else int(accept_rule)
        cfg.fix_infeasible = int(bool(fix_infeasible))
        cfg.normal_seed, cfg.uniform_seed = int(normal_seed) & (2**64 - 1), int(uniform_seed) & (2**64 - 1)
        cfg.window_words, cfg.max_windows, cfg.device = int(window_words), int(max_windows), int(device)
        h = C.c_void_p()
        check(L.kg_dea_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._L = L

    # stages
    def initialize(self):
        check(self._L.kg_dea_initialize(self.h))

    def prepare(self, generation):
        check(self._L.kg_dea_prepare(self.h, int(generation)))

    def evaluate(self, objective):
        check(self._L.kg_dea_eval_builtin(self.h, OBJECTIVES[objective.lower()] if isinstance(objective, str)
                                          else int(objective)))

    def update(self, generation):
        check(self._L.kg_dea_update(self.h, int(generation)))

    def generation(self, generation, objective):
        obj = OBJECTIVES[objective.lower()] if isinstance(objective, str) else int(objective)
        check(self._L.kg_dea_generation(self.h, int(generation), obj))

    def synchronize(self):
        check(self._L.kg_dea_synchronize(self.h))

    # host-callback objectives
    def candidates(self):
        X = np.empty((self.P, self.N))
        check(self._L.kg_dea_get_candidates(self.h, _dptr(X), self.N))
        return X

    def set_fitness(self, F):
        F = np.ascontiguousarray(F, dtype=np.float64)
        if F.shape != (self.P,):
            raise ValueError("fitness vector has shape %s, expected (%d,)" % (F.shape, self.P))
        check(self._L.kg_dea_set_fitness(self.h, _dptr(F)))

    def rng_state(self, which=1):
        return self._get_rng(which)

    def set_rng_state(self, state, which=1):
        self._set_rng(which, state)

    def windows(self):
        """(windows the last prepare() used, current window size in words)"""
        a, b = C.c_size_t(), C.c_size_t()
        check(self._L.kg_dea_windows(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


class MocmaesDevice(_Handle):
    """One Optimizer/MOCMAES (multi-objective CMA-ES) instance on one MI355X
    (kg_mocmaes_t), bit-exact to the reference's MOCMAES.cpp.base.  Generator
    indices for rng_state / set_rng_state: 0 Multinormal, 1 Uniform.
    parent_order "recorded" is the slot order of the reference's committed 2021
    result files, not a Korali setting."""

    _prefix = "kg_mocmaes"

    def __init__(self, N, P, lower_bound, upper_bound, mu=0, num_objectives=2, initial_value=None, initial_sdev=None,
                 evolution_path_adaption_strength=-1.0, covariance_learning_rate=-1.0, target_success_rate=0.175,
                 success_learning_rate=0.08, parent_order="Descending", multinormal_seed=0, uniform_seed=0,
                 window_blocks=0, max_windows=0, archive_rows=0, device=0):
        L = lib()
        self.N, self.K = int(N), int(num_objectives)
        self._arrays = [_vec(lower_bound, self.N, np.nan), _vec(upper_bound, self.N, np.nan),
                        _vec(initial_value, self.N, np.nan), _vec(initial_sdev, self.N, np.nan)]
        cfg = _MocmaesCfg()
        cfg.variable_count, cfg.population_size, cfg.mu_value = self.N, int(P), int(mu)
        cfg.num_objectives = self.K
        cfg.lower_bound, cfg.upper_bound, cfg.initial_value, cfg.initial_sdev = [_dptr(a) for a in self._arrays]
        cfg.evolution_path_adaption_strength = float(evolution_path_adaption_strength)
        cfg.covariance_learning_rate = float(covariance_learning_rate)
        cfg.target_success_rate, cfg.success_learning_rate = float(target_success_rate), float(success_learning_rate)
        cfg.parent_order = (MOCMAES_PARENT_ORDERS[parent_order.lower()] if isinstance(parent_order, str)
                            else int(parent_order))
        cfg.multinormal_seed = int(multinormal_seed) & (2**64 - 1)
        cfg.uniform_seed = int(uniform_seed) & (2**64 - 1)
        cfg.window_blocks, cfg.max_windows, cfg.archive_rows = int(window_blocks), int(max_windows), int(archive_rows)
        cfg.device = int(device)
        h = C.c_void_p()
        check(L.kg_mocmaes_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._L = L
        # the defaults of setInitialConfiguration (MOCMAES.cpp.base:24-25)
        self.P = int(P) or int(np.ceil(4. + np.floor(3. * np.log(float(self.N)))))
        self.mu = int(mu) or int(self.P / 2.)

    @staticmethod
    def _objective(objective):
        return MOCMAES_OBJECTIVES[objective.lower()] if isinstance(objective, str) else int(objective)

    # stages
    def initialize(self):
        check(self._L.kg_mocmaes_initialize(self.h))

    def prepare(self, generation):
        check(self._L.kg_mocmaes_prepare(self.h, int(generation)))

    def evaluate(self, objective):
        check(self._L.kg_mocmaes_eval_builtin(self.h, self._objective(objective)))

    def update(self, generation):
        check(self._L.kg_mocmaes_update(self.h, int(generation)))

    def generation(self, generation, objective):
        check(self._L.kg_mocmaes_generation(self.h, int(generation), self._objective(objective)))

    def synchronize(self):
        check(self._L.kg_mocmaes_synchronize(self.h))

    # host-callback objectives
    def candidates(self):
        X = np.empty((self.P, self.N))
        check(self._L.kg_mocmaes_get_candidates(self.h, _dptr(X), self.N))
        return X

    def set_values(self, V):
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.shape != (self.P, self.K):
            raise ValueError("value matrix has shape %s, expected (%d, %d)" % (V.shape, self.P, self.K))
        check(self._L.kg_mocmaes_set_values(self.h, _dptr(V)))

    def rng_state(self, which=0):
        return self._get_rng(which)

    def set_rng_state(self, state, which=0):
        self._set_rng(which, state)

    def diagnostics(self):
        """(windows the last prepare() used, window size in blocks, archive capacity in rows,
        peeling rounds of the last multi-workgroup sort)"""
        v = [C.c_size_t() for _ in range(4)]
        check(self._L.kg_mocmaes_diagnostics(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


def nested_permutation(seed, n):
    """iota(n) after std::shuffle with std::default_random_engine(seed), the
    order generatePosterior walks the dead samples in (Nested.cpp.base:584-586)."""
    out = (C.c_size_t * max(int(n), 1))()
    check(lib().kg_nested_permutation(int(seed) & (2**64 - 1), int(n), out))
    return np.array(out[:int(n)], dtype=np.int64)


class NestedDevice(_Handle):
    """One Sampler/Nested instance (resampling methods Box and Ellipse) on one
    MI355X (kg_nested_t).  prior_min / prior_max are the two parameters of
    every variable's prior, prior_kinds their kinds (PRIOR_KINDS names or
    numbers; None: Uniform); lower_bound / upper_bound the variables' bounds,
    needed for the non-Uniform ones.  likelihood: "gaussian", or None when
    the caller sets the log-likelihoods.  Generator indices for rng_state /
    set_rng_state: 0 Normal, 1 Uniform."""

    _prefix = "kg_nested"

    def __init__(self, N, L, prior_min, prior_max, batch_size=1, method="Ellipse", add_live_points=True,
                 proposal_update_frequency=1500, ellipsoidal_scaling=1.0, min_log_evidence_delta=0.01,
                 max_effective_sample_size=10e6, max_log_likelihood=10e6, prior_kinds=None, lower_bound=None,
                 upper_bound=None, uniform_seed=0, normal_seed=0, shuffle_seed=0, likelihood="gaussian",
                 window_tries=0, max_windows=0, device=0):
        lb = lib()
        self.N, self.L, self.B = int(N), int(L), int(batch_size)
        kinds = [0] * self.N if prior_kinds is None else [PRIOR_KINDS[k.lower()] if isinstance(k, str) else int(k)
                                                          for k in prior_kinds]
        self._kinds = (C.c_int * max(self.N, 1))(*kinds)
        self._arrays = [_vec(prior_min, self.N, np.nan), _vec(prior_max, self.N, np.nan),
                        _vec(lower_bound, self.N, -np.inf), _vec(upper_bound, self.N, np.inf)]
        cfg = _NestedCfg()
        cfg.variable_count, cfg.number_live_points, cfg.batch_size = self.N, self.L, self.B
        cfg.add_live_points = int(bool(add_live_points))
        cfg.resampling_method = NESTED_METHODS[method.lower()] if isinstance(method, str) else int(method)
        cfg.proposal_update_frequency = int(proposal_update_frequency)
        cfg.ellipsoidal_scaling = float(ellipsoidal_scaling)
        cfg.min_log_evidence_delta = float(min_log_evidence_delta)
        cfg.max_effective_sample_size = float(max_effective_sample_size)
        cfg.max_log_likelihood = float(max_log_likelihood)
        cfg.prior_min, cfg.prior_max, cfg.lower_bound, cfg.upper_bound = [_dptr(a) for a in self._arrays]
        cfg.prior_kind = self._kinds
        cfg.uniform_seed = int(uniform_seed) & (2**64 - 1)
        cfg.normal_seed = int(normal_seed) & (2**64 - 1)
        cfg.shuffle_seed = int(shuffle_seed) & (2**64 - 1)
        cfg.likelihood = -1 if likelihood is None else {"gaussian": 0}[likelihood.lower()]
        cfg.window_tries, cfg.max_windows, cfg.device = int(window_tries), int(max_windows), int(device)
        h = C.c_void_p()
        check(lb.kg_nested_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._L = lb
        self._rows = self.L

    # whole generations, builtin likelihood
    def first_generation(self):
        check(self._L.kg_nested_first_generation(self.h))

    def generation(self, generation):
        """runs one generation; returns the names of the termination criteria that hold after it"""
        t = C.c_int(0)
        check(self._L.kg_nested_generation(self.h, int(generation), C.byref(t)))
        return [n for b, n in NESTED_TERMINATION.items() if t.value & b]

    # stages, for likelihoods evaluated by the caller
    def prepare(self, generation):
        check(self._L.kg_nested_prepare(self.h, int(generation)))
        self._rows = self.L if int(generation) == 1 else self.B

    def candidates(self):
        X = np.empty((self._rows, self.N))
        check(self._L.kg_nested_get_candidates(self.h, _dptr(X), self.N))
        return X

    def set_evaluations(self, loglik):
        v = np.ascontiguousarray(loglik, dtype=np.float64).reshape(-1)
        if v.size != self._rows:
            raise ValueError("%d log-likelihoods, expected %d" % (v.size, self._rows))
        check(self._L.kg_nested_set_evaluations(self.h, _dptr(v)))

    def process(self, generation):
        """-> (accepted, names of the termination criteria that hold)"""
        a, t = C.c_int(0), C.c_int(0)
        check(self._L.kg_nested_process(self.h, int(generation), C.byref(a), C.byref(t)))
        return bool(a.value), [n for b, n in NESTED_TERMINATION.items() if t.value & b]

    def finalize(self):
        check(self._L.kg_nested_finalize(self.h))

    def synchronize(self):
        check(self._L.kg_nested_synchronize(self.h))

    def rng_state(self, which=0):
        return self._get_rng(which)

    def set_rng_state(self, state, which=0):
        self._set_rng(which, state)

    def diagnostics(self):
        """(windows the last candidate draw used, tries it consumed, current window size in tries)"""
        v = [C.c_size_t() for _ in range(3)]
        check(self._L.kg_nested_diagnostics(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


class McmcDevice(_Handle):
    """One Sampler/MCMC chain (Metropolis-Hastings with delayed rejection and
    adaptive sampling) on one MI355X (kg_mcmc_t).  probability: "gaussian", or
    None when the caller evaluates logP(x) (the stepping methods).  With
    prior_kinds (PRIOR_KINDS names or numbers; prior_min / prior_max their two
    parameters) logP = logPrior + the kernel's or the caller's value.
    Generator indices for rng_state / set_rng_state: 0 Normal, 1 Uniform."""

    _prefix = "kg_mcmc"

    def __init__(self, N, initial_mean, initial_sdev, burn_in=0, leap=1, rejection_levels=1,
                 use_adaptive_sampling=False, non_adaption_period=0, chain_covariance_scaling=1.0, max_samples=5000,
                 probability="gaussian", prior_kinds=None, prior_min=None, prior_max=None, normal_seed=0,
                 uniform_seed=0, window_candidates=0, device=0):
        lb = lib()
        self.N, self.R = int(N), int(rejection_levels)
        self._arrays = [_vec(initial_mean, self.N, np.nan), _vec(initial_sdev, self.N, np.nan)]
        cfg = _McmcCfg()
        cfg.variable_count, cfg.burn_in, cfg.leap, cfg.rejection_levels = self.N, int(burn_in), int(leap), self.R
        cfg.use_adaptive_sampling = int(bool(use_adaptive_sampling))
        cfg.non_adaption_period = int(non_adaption_period)
        cfg.chain_covariance_scaling = float(chain_covariance_scaling)
        cfg.max_samples = int(max_samples)
        cfg.initial_mean, cfg.initial_sdev = [_dptr(a) for a in self._arrays]
        cfg.probability_kernel = 0 if probability is None else (
            MCMC_KERNELS[probability.lower()] if isinstance(probability, str) else int(probability))
        if prior_kinds is not None:
            kinds = [PRIOR_KINDS[k.lower()] if isinstance(k, str) else int(k) for k in prior_kinds]
            self._kinds = (C.c_int * max(self.N, 1))(*kinds)
            self._arrays += [_vec(prior_min, self.N, np.nan), _vec(prior_max, self.N, np.nan)]
            cfg.prior_kind = self._kinds
            cfg.prior_min, cfg.prior_max = [_dptr(a) for a in self._arrays[2:]]
        cfg.normal_seed = int(normal_seed) & (2**64 - 1)
        cfg.uniform_seed = int(uniform_seed) & (2**64 - 1)
        cfg.window_candidates, cfg.device = int(window_candidates), int(device)
        h = C.c_void_p()
        check(lb.kg_mcmc_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._L = lb

    # whole generations, builtin kernel
    def run(self, first_generation, count, max_model_evaluations=0):
        """-> (generations completed, names of the stopping criteria that hold)"""
        done, t = C.c_size_t(0), C.c_int(0)
        check(self._L.kg_mcmc_run(self.h, int(first_generation), int(count), int(max_model_evaluations),
                                  C.byref(done), C.byref(t)))
        return done.value, [n for b, n in MCMC_STOP.items() if t.value & b]

    # one level at a time, for probabilities evaluated by the caller
    def propose(self, level):
        check(self._L.kg_mcmc_propose(self.h, int(level)))

    def candidate(self):
        x = np.empty(self.N)
        check(self._L.kg_mcmc_get_candidate(self.h, _dptr(x)))
        return x

    def decide(self, level, logp=0.0):
        a = C.c_int(0)
        check(self._L.kg_mcmc_decide(self.h, int(level), float(logp), C.byref(a)))
        return bool(a.value)

    def end_generation(self, generation):
        check(self._L.kg_mcmc_end_generation(self.h, int(generation)))

    def generation(self, generation, logp):
        """one generation with logp(x) evaluated by the caller; -> accepted"""
        accepted = False
        for level in range(self.R):
            self.propose(level)
            accepted = self.decide(level, logp(self.candidate()))
            if accepted:
                break
        self.end_generation(generation)
        return accepted

    def database(self):
        """-> (Sample Database rows x N, Sample Evaluation Database)"""
        rows = C.c_size_t(0)
        check(self._L.kg_mcmc_database(self.h, None, None, C.byref(rows)))
        X, lp = np.empty((rows.value, self.N)), np.empty(rows.value)
        check(self._L.kg_mcmc_database(self.h, _dptr(X), _dptr(lp), C.byref(rows)))
        return X, lp

    def synchronize(self):
        check(self._L.kg_mcmc_synchronize(self.h))

    def rng_state(self, which=0):
        return self._get_rng(which)

    def set_rng_state(self, state, which=0):
        self._set_rng(which, state)

    def diagnostics(self):
        """(launches the last run used, relaunches after an exhausted window, window size in candidates)"""
        v = [C.c_size_t() for _ in range(3)]
        check(self._L.kg_mcmc_diagnostics(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


class TmcmcDevice(_Handle):
    """One TMCMC sampler instance (Version "TMCMC") on one MI355X (kg_tmcmc_t).

    prior_min / prior_max: the Univariate/Uniform prior of every variable
    (prior_kind[d] = 1: the Univariate/Normal prior's Mean / Standard Deviation);
    prior_distribution[d]: index of the distribution object variable d draws
    from (variables sharing a distribution share its generator); prior_seeds[k]:
    seed of distribution k.  Generator indices for get_rng / set_rng:
    0 Multinomial, 1 Multivariate, 2 Uniform, 3 + k prior distribution k."""

    _prefix = "kg_tmcmc"

    def __init__(self, N, P, prior_min, prior_max, prior_seeds=None, prior_distribution=None,
                 multinomial_seed=0, multivariate_seed=0, uniform_seed=0, target_cov=1.0, covariance_scaling=0.04,
                 min_annealing_exponent_update=1e-5, max_annealing_exponent_update=1.0, max_chain_length=1,
                 default_burn_in=0, per_generation_burn_in=(), likelihood=0, device=0, shard_rank=0, shard_count=0,
                 version=0, step_size=0.1, domain_extension_factor=0.2, prior_kind=None):
        L = lib()
        self.N, self.P = int(N), int(P)
        pdist = (np.arange(self.N, dtype=np.int32) if prior_distribution is None
                 else np.ascontiguousarray(prior_distribution, dtype=np.int32))
        ndist = int(pdist.max()) + 1
        seeds = np.zeros(ndist, dtype=np.uint64) if prior_seeds is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(prior_seeds, dtype=np.uint64), (ndist,)))
        pgb = np.ascontiguousarray(per_generation_burn_in, dtype=np.float64).reshape(-1)
        pkind = None if prior_kind is None else np.ascontiguousarray(prior_kind, dtype=np.int32)
        self._arrays = [_vec(prior_min, self.N, 0.0), _vec(prior_max, self.N, 1.0), pdist, seeds, pgb, pkind]
        cfg = _TmcmcCfg()
        cfg.variable_count, cfg.population_size = self.N, self.P
        cfg.max_chain_length, cfg.default_burn_in = float(max_chain_length), float(default_burn_in)
        cfg.target_cov, cfg.covariance_scaling = float(target_cov), float(covariance_scaling)
        cfg.min_annealing_exponent_update = float(min_annealing_exponent_update)
        cfg.max_annealing_exponent_update = float(max_annealing_exponent_update)
        cfg.prior_min, cfg.prior_max = _dptr(self._arrays[0]), _dptr(self._arrays[1])
        cfg.prior_distribution = pdist.ctypes.data_as(C.POINTER(C.c_int))
        cfg.distribution_count = ndist
        cfg.prior_seeds = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
        cfg.multinomial_seed, cfg.multivariate_seed, cfg.uniform_seed = (int(multinomial_seed),
                                                                        int(multivariate_seed), int(uniform_seed))
        cfg.likelihood, cfg.device = int(likelihood), int(device)
        cfg.per_generation_burn_in = _dptr(pgb) if pgb.size else None
        cfg.per_generation_burn_in_count = pgb.size
        cfg.shard_rank, cfg.shard_count = int(shard_rank), int(shard_count)
        cfg.version = 1 if version in (1, "mTMCMC") else 0
        cfg.step_size, cfg.domain_extension_factor = float(step_size), float(domain_extension_factor)
        cfg.prior_kind = None if pkind is None else pkind.ctypes.data_as(C.POINTER(C.c_int))
        h = C.c_void_p()
        check(L.kg_tmcmc_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._L = L

    def prepare(self, generation):
        check(self._L.kg_tmcmc_prepare(self.h, int(generation)))

    def evaluate(self):
        check(self._L.kg_tmcmc_evaluate(self.h))

    def process(self, generation):
        check(self._L.kg_tmcmc_process(self.h, int(generation)))

    def process_partial(self, generation):
        check(self._L.kg_tmcmc_process_partial(self.h, int(generation)))

    def process_finalize(self, generation):
        check(self._L.kg_tmcmc_process_finalize(self.h, int(generation)))

    def device_ptr(self, name):
        p = C.c_void_p()
        check(self._L.kg_tmcmc_device_ptr(self.h, name.encode(), C.byref(p)))
        return p.value

    def stream(self):
        p = C.c_void_p()
        check(self._L.kg_tmcmc_stream(self.h, C.byref(p)))
        return p.value

    def advance(self, generation):
        """One step of every unfinished chain; returns how many chains now
        have a candidate pending evaluation."""
        n = C.c_size_t()
        check(self._L.kg_tmcmc_advance(self.h, int(generation), C.byref(n)))
        return n.value

    def pending(self):
        m = np.zeros(self.P, dtype=np.uint8)
        check(self._L.kg_tmcmc_get_pending(self.h, m.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return m.astype(bool)

    def generation(self, generation):
        check(self._L.kg_tmcmc_generation(self.h, int(generation)))

    def synchronize(self):
        check(self._L.kg_tmcmc_synchronize(self.h))

    def evaluate_prior(self):
        check(self._L.kg_tmcmc_evaluate_prior(self.h))

    def candidates(self):
        X = np.empty((self.P, self.N))
        check(self._L.kg_tmcmc_get_candidates(self.h, _dptr(X), self.N))
        return X

    def set_evaluations(self, log_prior, log_likelihood):
        lp = np.ascontiguousarray(log_prior, dtype=np.float64)
        ll = np.ascontiguousarray(log_likelihood, dtype=np.float64)
        check(self._L.kg_tmcmc_set_evaluations(self.h, _dptr(lp), _dptr(ll)))

    def set_gradients(self, grad, fisher):
        """mTMCMC: every candidate's log-likelihood gradient (P x N) and Fisher
        information (P x N x N); kg_tmcmc_set_gradients."""
        g = np.ascontiguousarray(grad, dtype=np.float64).reshape(-1)
        f = np.ascontiguousarray(fisher, dtype=np.float64).reshape(-1)
        if g.size != self.P * self.N or f.size != self.P * self.N * self.N:
            raise ValueError("set_gradients: expected P x N gradients and P x N x N Fisher informations")
        check(self._L.kg_tmcmc_set_gradients(self.h, _dptr(g), _dptr(f)))

    def set_hierarchical(self, mode, kinds, param_index, param_const, groups, log_priors=None):
        """The Hierarchical/Psi ("psi") or /ThetaNew ("thetanew") likelihood as
        this handle's builtin one (kg_tmcmc_set_hierarchical), before the first
        prepare.  kinds: D prior kinds (names or enum kg_prior_kind);
        param_index / param_const: D x 2, the variable (Psi) or database column
        (ThetaNew) that supplies each parameter, or -1 and the constant; groups:
        the sample databases (K_g x width each; ThetaNew: one); log_priors:
        Psi, each group's K_g log-priors."""
        d = _TmcmcHierarchical()
        d.mode = HIER_MODES[mode.lower()] if isinstance(mode, str) else int(mode)
        kd = np.ascontiguousarray([PRIOR_KINDS[k.lower()] if isinstance(k, str) else int(k) for k in kinds],
                                  dtype=np.int32)
        D = kd.size
        ix = np.ascontiguousarray(param_index, dtype=np.int32).reshape(-1)
        cs = np.ascontiguousarray(param_const, dtype=np.float64).reshape(-1)
        if ix.size != 2 * D or cs.size != 2 * D:
            raise ValueError("set_hierarchical: param_index / param_const must be D x 2")
        gs = [np.ascontiguousarray(g, dtype=np.float64) for g in groups]
        if any(g.ndim != 2 for g in gs) or len({g.shape[1] for g in gs}) != 1:
            raise ValueError("set_hierarchical: groups must be 2-D arrays of one width")
        sizes = np.ascontiguousarray([g.shape[0] for g in gs], dtype=np.uintp)
        rows = np.ascontiguousarray(np.concatenate(gs, axis=0))
        d.prior_count, d.kind = D, kd.ctypes.data_as(C.POINTER(C.c_int))
        d.param_index, d.param_const = ix.ctypes.data_as(C.POINTER(C.c_int)), _dptr(cs)
        d.group_count, d.group_size = len(gs), sizes.ctypes.data_as(C.POINTER(C.c_size_t))
        d.row_width, d.rows = gs[0].shape[1], _dptr(rows)
        lp = None
        if log_priors is not None:
            lp = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in log_priors]))
            if lp.size != rows.shape[0]:
                raise ValueError("set_hierarchical: one log-prior per database row")
            d.log_prior = _dptr(lp)
        check(self._L.kg_tmcmc_set_hierarchical(self.h, C.byref(d)))

    def hierarchical_loglik(self, X):
        """The hierarchical log-likelihood of arbitrary points (rows x N), the
        prior not consulted (kg_tmcmc_hierarchical_loglik)."""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, self.N)
        out = np.empty(X.shape[0])
        check(self._L.kg_tmcmc_hierarchical_loglik(self.h, _dptr(X), X.shape[0], _dptr(out)))
        return out

    def set_hierarchical_theta(self, kinds, param_index, param_const, psi_db, sub_db, sub_log_priors):
        """The Hierarchical/Theta likelihood (kg_tmcmc_set_hierarchical_theta),
        before the first prepare: the handle's own log-likelihood (the builtin
        kernel, or what set_evaluations is given) becomes the sub-problem's
        and the device completes it.  kinds / param_index / param_const: the
        Psi experiment's D conditional priors, as set_hierarchical("thetanew")
        takes them; psi_db: its sample database (M x width); sub_db: the
        sub-experiment's (K x D); sub_log_priors: its K log-priors."""
        d = _TmcmcHierTheta()
        kd = np.ascontiguousarray([PRIOR_KINDS[k.lower()] if isinstance(k, str) else int(k) for k in kinds],
                                  dtype=np.int32)
        D = kd.size
        ix = np.ascontiguousarray(param_index, dtype=np.int32).reshape(-1)
        cs = np.ascontiguousarray(param_const, dtype=np.float64).reshape(-1)
        if ix.size != 2 * D or cs.size != 2 * D:
            raise ValueError("set_hierarchical_theta: param_index / param_const must be D x 2")
        psi = np.ascontiguousarray(psi_db, dtype=np.float64)
        sub = np.ascontiguousarray(sub_db, dtype=np.float64)
        lp = np.ascontiguousarray(sub_log_priors, dtype=np.float64).reshape(-1)
        if psi.ndim != 2 or sub.ndim != 2 or sub.shape[1] != D:
            raise ValueError("set_hierarchical_theta: psi_db must be M x width and sub_db K x D")
        if lp.size != sub.shape[0]:
            raise ValueError("set_hierarchical_theta: one log-prior per sub-experiment sample")
        d.prior_count, d.kind = D, kd.ctypes.data_as(C.POINTER(C.c_int))
        d.param_index, d.param_const = ix.ctypes.data_as(C.POINTER(C.c_int)), _dptr(cs)
        d.psi_rows, d.psi_width, d.psi_db = psi.shape[0], psi.shape[1], _dptr(psi)
        d.sub_rows, d.sub_db, d.sub_log_prior = sub.shape[0], _dptr(sub), _dptr(lp)
        check(self._L.kg_tmcmc_set_hierarchical_theta(self.h, C.byref(d)))
        self._theta_rows = psi.shape[0]

    def theta_denominators(self):
        """Theta's precomputed log-denominators, one per Psi sample
        (kg_tmcmc_theta_denominators)."""
        out = np.empty(getattr(self, "_theta_rows", 0))
        check(self._L.kg_tmcmc_theta_denominators(self.h, _dptr(out), out.size))
        return out

    def theta_loglik(self, X, sub_loglik=None):
        """The Hierarchical/Theta log-likelihood of arbitrary points (rows x N)
        whose sub-problem log-likelihoods are sub_loglik (None: 0.0), the prior
        not consulted (kg_tmcmc_theta_loglik)."""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, self.N)
        out = np.empty(X.shape[0])
        sub = None
        if sub_loglik is not None:
            sub = np.ascontiguousarray(sub_loglik, dtype=np.float64).reshape(-1)
            if sub.size != X.shape[0]:
                raise ValueError("theta_loglik: one sub-problem log-likelihood per point")
        check(self._L.kg_tmcmc_theta_loglik(self.h, _dptr(X), X.shape[0], _dptr(sub) if sub is not None else None,
                                            _dptr(out)))
        return out

    def get_rng(self, which):
        return self._get_rng(which)

    def set_rng(self, which, state):
        self._set_rng(which, state)
