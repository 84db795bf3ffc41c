"""Sampler/MCMC and the Sampling problem through korali.Engine: configuration
errors raised before any device call, the defaults, and the rejections (CPU,
no GPU needed)."""
import pytest

import korali


def base_mcmc(n=2, kernel=True, **solver):
    e = korali.Experiment()
    e["Problem"]["Type"] = "Sampling"
    if kernel:
        e["Problem"]["Probability Kernel"] = "Gaussian"
    else:
        e["Problem"]["Probability Function"] = lambda s: None
    for i in range(n):
        e["Variables"][i]["Name"] = "X" + str(i)
        e["Variables"][i]["Initial Mean"] = 0.0
        e["Variables"][i]["Initial Standard Deviation"] = 1.0
    e["Solver"]["Type"] = "Sampler/MCMC"
    for k, v in solver.items():
        e["Solver"][k] = v
    e["File Output"]["Enabled"] = False
    e["Console Output"]["Verbosity"] = "Silent"
    return e


def bayesian_mcmc(n=2, **solver):
    e = base_mcmc(n, **solver)
    e["Problem"] = {"Type": "Bayesian/Custom", "Likelihood Model": lambda s: None}
    e["Distributions"][0]["Name"] = "Uniform 0"
    e["Distributions"][0]["Type"] = "Univariate/Uniform"
    e["Distributions"][0]["Minimum"] = -5.0
    e["Distributions"][0]["Maximum"] = 5.0
    for i in range(n):
        e["Variables"][i]["Prior Distribution"] = "Uniform 0"
    return e


def fails(e, msg, engine=None):
    with pytest.raises(korali.KoraliError, match=msg):
        (engine or korali.Engine()).run(e)


# MCMC.cpp.base:23-27, verbatim
@pytest.mark.parametrize("key,value,msg", [
    ("Chain Covariance Scaling", 0.0, r"Chain Covariance Scaling must be larger 0.0 \(is 0.000000\)."),
    ("Chain Covariance Scaling", -2.0, r"Chain Covariance Scaling must be larger 0.0 \(is -2.000000\)."),
    ("Leap", 0, r"Leap must be larger 0 \(is 0\)."),
    ("Burn In", -1, r"Burn In must be larger equal 0 \(is 18446744073709551615\)."),
    ("Rejection Levels", 0, r"Rejection Levels must be larger 0 \(is 0\)."),
    ("Non Adaption Period", -1, r"Non Adaption Period must be larger equal 0 \(is 18446744073709551615\)."),
])
def test_the_reference_checks(key, value, msg):
    fails(base_mcmc(**{key: value}), msg)


# what this build does not provide
def test_more_than_64_variables():
    fails(base_mcmc(65), "more than 64 variables")


def test_more_than_8_rejection_levels():
    fails(base_mcmc(**{"Rejection Levels": 9}), "more than 8 'Rejection Levels'")


def test_database_capacity():
    e = base_mcmc(64)
    e["Solver"]["Termination Criteria"]["Max Samples"] = 2**21 + 1
    fails(e, "exceeds the database's capacity")


def test_variables_need_mean_and_standard_deviation():
    e = base_mcmc()
    e["Variables"][1] = {"Name": "X1", "Initial Standard Deviation": 1.0}
    fails(e, r"No value provided for mandatory setting: \['Initial Mean'\] required by MCMC")
    e = base_mcmc()
    e["Variables"][0] = {"Name": "X0", "Initial Mean": 1.0}
    fails(e, r"No value provided for mandatory setting: \['Initial Standard Deviation'\] required by MCMC")


def test_sampling_needs_a_function_or_a_kernel():
    e = base_mcmc()
    e["Problem"] = {"Type": "Sampling"}
    fails(e, "Problem 'Sampling' requires a 'Probability Function'")
    e["Problem"]["Probability Kernel"] = "Lorentzian"
    fails(e, "Unknown 'Probability Kernel' 'Lorentzian'")


def test_sampling_needs_a_variable():
    e = base_mcmc(0)
    fails(e, "Sampling Evaluation problems require at least one variable.")


def test_bayesian_problem_reads_its_priors_and_likelihood():
    e = bayesian_mcmc()
    e["Variables"][1]["Prior Distribution"] = "Nowhere"
    fails(e, "Did not find a distribution named 'Nowhere'")
    e = bayesian_mcmc()
    e["Problem"] = {"Type": "Bayesian/Custom"}
    fails(e, "Problem 'Bayesian/Custom' requires a 'Likelihood Model'")
    e = bayesian_mcmc()
    e["Problem"] = {"Type": "Bayesian/Reference"}
    fails(e, "Problem 'Bayesian/Reference' requires a 'Computational Model' function")


def test_hierarchical_problems_need_tmcmc():
    e = base_mcmc()
    e["Problem"]["Type"] = "Hierarchical/Psi"
    fails(e, "are supported with the 'Sampler/TMCMC' solver")


def test_needs_a_sampling_or_bayesian_problem():
    e = base_mcmc()
    e["Problem"] = {"Type": "Optimization", "Objective Kernel": "Negative Rosenbrock"}
    fails(e, "The device MCMC path supports problems of type 'Sampling', 'Bayesian/Custom' and 'Bayesian/Reference'")


def test_distributed_conduit_is_not_provided(monkeypatch):
    for v in ("RANK", "WORLD_SIZE"):
        monkeypatch.delenv(v, raising=False)
    k = korali.Engine()
    k["Conduit"]["Type"] = "Distributed"
    k["Conduit"]["Transport"] = "Host"  # one rank: no sockets
    fails(base_mcmc(), "Sampler/MCMC does not shard across ranks", k)


@pytest.mark.parametrize("where,key,msg", [
    ("Solver", "Burn In Steps", "Unrecognized settings for Korali module: MCMC"),
    ("Termination", "Target Annealing Exponent", "Unrecognized settings for Korali module: MCMC"),
    ("Problem", "Probability", "Unrecognized settings for Korali module: Sampling"),
    ("Variable", "Initial Sigma", "Unrecognized settings for Korali module: MCMC"),
])
def test_unknown_keys_are_rejected(where, key, msg):
    e = base_mcmc()
    if where == "Termination":
        e["Solver"]["Termination Criteria"][key] = 1.0
    elif where == "Variable":
        e["Variables"][1][key] = 1.0
    else:
        e[where][key] = 1.0
    fails(e, msg)


def test_defaults_are_those_of_mcmc_config():
    """MCMC.config:162-189; the run then stops at a limit of this build, before any device call"""
    e = base_mcmc(65)
    fails(e, "more than 64 variables")
    sv = e["Solver"]
    assert sv["Burn In"] == 0 and sv["Leap"] == 1 and sv["Rejection Levels"] == 1
    assert sv["Use Adaptive Sampling"] is False and sv["Non Adaption Period"] == 0
    assert sv["Chain Covariance Scaling"] == 1.0
    tc = sv["Termination Criteria"]
    assert tc["Max Samples"] == 5000 and tc["Max Generations"] == 1e10 and tc["Max Model Evaluations"] == 1e9
    assert sv["Normal Generator"]["Type"] == "Univariate/Normal" and sv["Normal Generator"]["Standard Deviation"] == 1.0
    assert sv["Uniform Generator"]["Type"] == "Univariate/Uniform" and sv["Uniform Generator"]["Maximum"] == 1.0


def test_seeds_follow_the_distributions_normal_first():
    e = bayesian_mcmc(65)
    e["Random Seed"] = 1000
    fails(e, "more than 64 variables")
    assert e["Distributions"][0]["Random Seed"] == 1000
    assert e["Solver"]["Normal Generator"]["Random Seed"] == 1001
    assert e["Solver"]["Uniform Generator"]["Random Seed"] == 1002


def test_type_string_ignores_case_and_whitespace():
    e = base_mcmc(Leap=0)
    e["Solver"]["Type"] = " sampler / mcmc "
    fails(e, r"Leap must be larger 0 \(is 0\).")
    e["Solver"]["Type"] = "Sampler/Metropolis"
    fails(e, "Unrecognized solver type 'Sampler/Metropolis'.*Sampler/Nested, Sampler/MCMC, Agent/Continuous/VRACER")
