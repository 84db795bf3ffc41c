"""The public surface of the six solver classes of korali_amd.native, written
down from the commit before they were given a common base class: every public
method (and the three dunder methods callers use) with its signature.  No
device is constructed (CPU, no GPU needed)."""
import inspect

import pytest

from korali_amd import native

DUNDER = ("__init__", "__getitem__", "__setitem__")

SURFACE = {'CmaesDevice': {'__getitem__': '(self, name)',
                 '__init__': "(self, N, lam, mu=0, mu_type='Logarithmic', lower_bound=None, upper_bound=None, "
                             'initial_value=None, initial_std=None, min_std_update=None, normal_seed=0, '
                             "uniform_seed=0, cov_mode='exact', is_sigma_bounded=False, diagonal=False, "
                             'max_infeasible_resamplings=inf, initial_sigma_cumulation_factor=-1.0, '
                             'initial_damp_factor=-1.0, initial_cumulative_covariance=-1.0, device=0, '
                             "store_bdz=False, eigen_chase='host', shard_rank=0, shard_count=1, mirrored=False, "
                             'gradient_step_size=None, granularity=None, constraints=None, '
                             'viability_population_size=2, viability_mu_value=0, '
                             'max_covariance_matrix_corrections=1000000.0, target_success_rate=0.1818, '
                             'covariance_matrix_adaption_strength=0.1, global_success_learning_rate=0.2)',
                 '__setitem__': '(self, name, value)',
                 'begin_sample': '(self)',
                 'candidates': '(self)',
                 'close': '(self)',
                 'device_ptr': '(self, name)',
                 'evaluate': '(self, objective)',
                 'field_size': '(self, name)',
                 'generation': '(self, generation, objective)',
                 'get_prefix': '(self, name, n)',
                 'get_rng': '(self, which)',
                 'initialize': '(self)',
                 'lam': 'property',
                 'prepare_constrained': '(self, generation)',
                 'profile': '(self, enable=True)',
                 'profile_mark': '(self, stage, phase)',
                 'profile_read': '(self, stage)',
                 'sample': '(self)',
                 'sample_eval': '(self, objective)',
                 'set_fitness': '(self, F)',
                 'set_gradients': '(self, G)',
                 'set_log_posterior': '(self, F)',
                 'set_rng': '(self, which, state)',
                 'shard_row_count': '(self)',
                 'sorting_index': '(self)',
                 'stream': '(self)',
                 'synchronize': '(self)',
                 'update': '(self, generation)',
                 'update_finalize': '(self, generation)',
                 'update_partial': '(self, generation)',
                 'update_rows': '(self, generation)'},
 'DeaDevice': {'__getitem__': '(self, name)',
               '__init__': '(self, N, P, lower_bound, upper_bound, crossover_rate=0.9, mutation_rate=0.5, '
                           "mutation_rule='Fixed', parent_rule='Random', accept_rule='Greedy', fix_infeasible=True, "
                           'normal_seed=0, uniform_seed=0, window_words=0, max_windows=0, device=0)',
               '__setitem__': '(self, name, value)',
               'candidates': '(self)',
               'close': '(self)',
               'evaluate': '(self, objective)',
               'field_size': '(self, name)',
               'generation': '(self, generation, objective)',
               'initialize': '(self)',
               'prepare': '(self, generation)',
               'profile': '(self, enable=True)',
               'profile_read': '(self, stage)',
               'rng_state': '(self, which=1)',
               'set_fitness': '(self, F)',
               'set_rng_state': '(self, state, which=1)',
               'synchronize': '(self)',
               'update': '(self, generation)',
               'windows': '(self)'},
 'McmcDevice': {'__getitem__': '(self, name)',
                '__init__': '(self, N, initial_mean, initial_sdev, burn_in=0, leap=1, rejection_levels=1, '
                            'use_adaptive_sampling=False, non_adaption_period=0, chain_covariance_scaling=1.0, '
                            "max_samples=5000, probability='gaussian', prior_kinds=None, prior_min=None, "
                            'prior_max=None, normal_seed=0, uniform_seed=0, window_candidates=0, device=0)',
                '__setitem__': '(self, name, value)',
                'candidate': '(self)',
                'close': '(self)',
                'database': '(self)',
                'decide': '(self, level, logp=0.0)',
                'diagnostics': '(self)',
                'end_generation': '(self, generation)',
                'field_size': '(self, name)',
                'generation': '(self, generation, logp)',
                'profile': '(self, enable=True)',
                'profile_read': '(self, stage)',
                'propose': '(self, level)',
                'rng_state': '(self, which=0)',
                'run': '(self, first_generation, count, max_model_evaluations=0)',
                'set_rng_state': '(self, state, which=0)',
                'synchronize': '(self)'},
 'MocmaesDevice': {'__getitem__': '(self, name)',
                   '__init__': '(self, N, P, lower_bound, upper_bound, mu=0, num_objectives=2, initial_value=None, '
                               'initial_sdev=None, evolution_path_adaption_strength=-1.0, '
                               'covariance_learning_rate=-1.0, target_success_rate=0.175, '
                               "success_learning_rate=0.08, parent_order='Descending', multinormal_seed=0, "
                               'uniform_seed=0, window_blocks=0, max_windows=0, archive_rows=0, device=0)',
                   '__setitem__': '(self, name, value)',
                   'candidates': '(self)',
                   'close': '(self)',
                   'diagnostics': '(self)',
                   'evaluate': '(self, objective)',
                   'field_size': '(self, name)',
                   'generation': '(self, generation, objective)',
                   'initialize': '(self)',
                   'prepare': '(self, generation)',
                   'profile': '(self, enable=True)',
                   'profile_read': '(self, stage)',
                   'rng_state': '(self, which=0)',
                   'set_rng_state': '(self, state, which=0)',
                   'set_values': '(self, V)',
                   'synchronize': '(self)',
                   'update': '(self, generation)'},
 'NestedDevice': {'__getitem__': '(self, name)',
                  '__init__': "(self, N, L, prior_min, prior_max, batch_size=1, method='Ellipse', "
                              'add_live_points=True, proposal_update_frequency=1500, ellipsoidal_scaling=1.0, '
                              'min_log_evidence_delta=0.01, max_effective_sample_size=10000000.0, '
                              'max_log_likelihood=10000000.0, prior_kinds=None, lower_bound=None, upper_bound=None, '
                              "uniform_seed=0, normal_seed=0, shuffle_seed=0, likelihood='gaussian', window_tries=0, "
                              'max_windows=0, device=0)',
                  '__setitem__': '(self, name, value)',
                  'candidates': '(self)',
                  'close': '(self)',
                  'diagnostics': '(self)',
                  'field_size': '(self, name)',
                  'finalize': '(self)',
                  'first_generation': '(self)',
                  'generation': '(self, generation)',
                  'prepare': '(self, generation)',
                  'process': '(self, generation)',
                  'profile': '(self, enable=True)',
                  'profile_read': '(self, stage)',
                  'rng_state': '(self, which=0)',
                  'set_evaluations': '(self, loglik)',
                  'set_rng_state': '(self, state, which=0)',
                  'synchronize': '(self)'},
 'TmcmcDevice': {'__getitem__': '(self, name)',
                 '__init__': '(self, N, P, prior_min, prior_max, prior_seeds=None, prior_distribution=None, '
                             'multinomial_seed=0, multivariate_seed=0, uniform_seed=0, target_cov=1.0, '
                             'covariance_scaling=0.04, min_annealing_exponent_update=1e-05, '
                             'max_annealing_exponent_update=1.0, max_chain_length=1, default_burn_in=0, '
                             'per_generation_burn_in=(), likelihood=0, device=0, shard_rank=0, shard_count=0, '
                             'version=0, step_size=0.1, domain_extension_factor=0.2, prior_kind=None)',
                 '__setitem__': '(self, name, value)',
                 'advance': '(self, generation)',
                 'candidates': '(self)',
                 'close': '(self)',
                 'device_ptr': '(self, name)',
                 'evaluate': '(self)',
                 'evaluate_prior': '(self)',
                 'field_size': '(self, name)',
                 'generation': '(self, generation)',
                 'get_rng': '(self, which)',
                 'hierarchical_loglik': '(self, X)',
                 'pending': '(self)',
                 'prepare': '(self, generation)',
                 'process': '(self, generation)',
                 'process_finalize': '(self, generation)',
                 'process_partial': '(self, generation)',
                 'profile': '(self, enable=True)',
                 'profile_read': '(self, stage)',
                 'set_evaluations': '(self, log_prior, log_likelihood)',
                 'set_gradients': '(self, grad, fisher)',
                 'set_hierarchical': '(self, mode, kinds, param_index, param_const, groups, log_priors=None)',
                 'set_hierarchical_theta': '(self, kinds, param_index, param_const, psi_db, sub_db, sub_log_priors)',
                 'set_rng': '(self, which, state)',
                 'stream': '(self)',
                 'synchronize': '(self)',
                 'theta_denominators': '(self)',
                 'theta_loglik': '(self, X, sub_loglik=None)'}}


def surface(cls):
    out = {}
    for name in dir(cls):
        if name.startswith("_") and name not in DUNDER:
            continue
        a = inspect.getattr_static(cls, name)
        if isinstance(a, property):
            out[name] = "property"
        elif isinstance(a, staticmethod):
            out[name] = "static" + str(inspect.signature(a.__func__))
        else:
            out[name] = str(inspect.signature(a))
    return out


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_class_has_exactly_the_recorded_methods(name):
    got, want = surface(getattr(native, name)), SURFACE[name]
    assert sorted(got) == sorted(want)
    for method in want:
        assert got[method] == want[method], method


def test_rng_accessors_keep_their_two_spellings_and_defaults():
    for name, default in (("DeaDevice", "1"), ("MocmaesDevice", "0"), ("NestedDevice", "0"), ("McmcDevice", "0")):
        assert SURFACE[name]["rng_state"] == "(self, which=%s)" % default
        assert SURFACE[name]["set_rng_state"] == "(self, state, which=%s)" % default
        assert "get_rng" not in SURFACE[name] and "set_rng" not in SURFACE[name]
    for name in ("CmaesDevice", "TmcmcDevice"):
        assert SURFACE[name]["get_rng"] == "(self, which)" and SURFACE[name]["set_rng"] == "(self, which, state)"
        assert "rng_state" not in SURFACE[name]
