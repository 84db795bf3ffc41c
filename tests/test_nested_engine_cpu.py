"""Sampler/Nested through korali.Engine: configuration errors raised before
any device call, the defaults, and the rejections (CPU, no GPU needed)."""
import pytest

import korali


def base_nested(n=3, **solver):
    e = korali.Experiment()
    e["Problem"]["Type"] = "Bayesian/Custom"
    e["Problem"]["Likelihood Model"] = lambda s: None
    e["Distributions"][0]["Name"] = "Uniform 0"
    e["Distributions"][0]["Type"] = "Univariate/Uniform"
    e["Distributions"][0]["Minimum"] = -5.0
    e["Distributions"][0]["Maximum"] = 5.0
    for i in range(n):
        e["Variables"][i]["Name"] = "X" + str(i)
        e["Variables"][i]["Prior Distribution"] = "Uniform 0"
    e["Solver"]["Type"] = "Sampler/Nested"
    for k, v in solver.items():
        e["Solver"][k] = v
    e["File Output"]["Enabled"] = False
    e["Console Output"]["Verbosity"] = "Silent"
    return e


def with_normal_prior(e, lower=None, upper=None):
    e["Distributions"][1]["Name"] = "Normal 1"
    e["Distributions"][1]["Type"] = "Univariate/Normal"
    e["Distributions"][1]["Mean"] = 0.0
    e["Distributions"][1]["Standard Deviation"] = 1.0
    e["Variables"][1]["Prior Distribution"] = "Normal 1"
    if lower is not None:
        e["Variables"][1]["Lower Bound"] = lower
    if upper is not None:
        e["Variables"][1]["Upper Bound"] = upper
    return e


def fails(e, msg, engine=None):
    with pytest.raises(korali.KoraliError, match=msg):
        (engine or korali.Engine()).run(e)


# Nested.cpp.base:64-93, verbatim
def test_min_log_evidence_delta_must_not_be_negative():
    e = base_nested()
    e["Solver"]["Termination Criteria"]["Min Log Evidence Delta"] = -1.0
    fails(e, r"Min Log Evidence Delta must be larger equal 0.0 \(is -1.000000\).")


def test_resampling_method_names():
    fails(base_nested(**{"Resampling Method": "Sphere"}),
          r"Only accepted Resampling Method are 'Box', 'Ellipse' and 'Multi Ellipse' \(is Sphere\).")


def test_proposal_update_frequency_must_be_positive():
    fails(base_nested(**{"Proposal Update Frequency": 0}), "Proposal Update Frequency must be larger 0")


def test_non_uniform_prior_needs_both_bounds():
    fails(with_normal_prior(base_nested(), upper=3.0),
          r"Prior of variable X1 is not 'Univariate/Uniform' \(is Univariate/Normal\) AND lower bound not set "
          r"\(invalid configuration\).")
    fails(with_normal_prior(base_nested(), lower=-3.0),
          r"Prior of variable X1 is not 'Univariate/Uniform' \(is Univariate/Normal\) AND upper bound not set "
          r"\(invalid configuration\).")


@pytest.mark.parametrize("method", ["Ellipse", "Multi Ellipse"])
def test_ellipse_needs_three_variables(method):
    fails(base_nested(2, **{"Resampling Method": method}),
          r"Resampling Method 'Ellipse' and 'Multi Ellipse' only suitable for problems of dim larger 2 \(use Resampling "
          r"Method 'Box'\).")


def test_unknown_prior_distribution():
    e = base_nested()
    e["Variables"][2]["Prior Distribution"] = "Nowhere"
    fails(e, "Did not find a distribution named 'Nowhere'")


# what this build does not provide
def test_multi_ellipse_is_rejected_by_name():
    fails(base_nested(**{"Resampling Method": "Multi Ellipse"}), "'Multi Ellipse' is not provided on the device path")


def test_more_than_64_variables():
    fails(base_nested(65, **{"Resampling Method": "Box"}), "more than 64 variables")


def test_hierarchical_problems_need_tmcmc():
    e = base_nested()
    e["Problem"]["Type"] = "Hierarchical/Psi"
    fails(e, "are supported with the 'Sampler/TMCMC' solver")


def test_needs_a_bayesian_problem():
    e = base_nested()
    e["Problem"]["Type"] = "Optimization"
    fails(e, "The device Nested path supports problems of type 'Bayesian/Custom' and 'Bayesian/Reference'")


def test_distributed_conduit_is_not_provided(monkeypatch):
    for v in ("RANK", "WORLD_SIZE"):
        monkeypatch.delenv(v, raising=False)
    k = korali.Engine()
    k["Conduit"]["Type"] = "Distributed"
    k["Conduit"]["Transport"] = "Host"  # one rank: no sockets
    fails(base_nested(), "Sampler/Nested does not shard across ranks", k)


@pytest.mark.parametrize("where,key,msg", [
    ("Solver", "Number Of Live Points", "Unrecognized settings for Korali module: Nested"),
    ("Termination", "Target Annealing Exponent", "Unrecognized settings for Korali module: Nested"),
    ("Problem", "Likelihood", "Unrecognized settings for Korali module: Custom"),
])
def test_unknown_keys_are_rejected(where, key, msg):
    e = base_nested()
    if where == "Termination":
        e["Solver"]["Termination Criteria"][key] = 1.0
    else:
        e[where][key] = 1.0
    fails(e, msg)


def test_defaults_are_those_of_nested_config():
    """Nested.config:318-335; the run then stops at a limit of this build, before any device call"""
    e = base_nested(65)
    fails(e, "more than 64 variables")
    sv = e["Solver"]
    assert sv["Number Live Points"] == 1500 and sv["Batch Size"] == 1 and sv["Add Live Points"] is True
    assert sv["Resampling Method"] == "Ellipse" and sv["Proposal Update Frequency"] == 1500
    assert sv["Ellipsoidal Scaling"] == 1.0
    tc = sv["Termination Criteria"]
    assert tc["Min Log Evidence Delta"] == 0.01
    assert tc["Max Effective Sample Size"] == 10e6 and tc["Max Log Likelihood"] == 10e6


def test_type_string_ignores_case_and_whitespace():
    e = base_nested(**{"Proposal Update Frequency": 0})
    e["Solver"]["Type"] = " sampler / nested "
    fails(e, "Proposal Update Frequency must be larger 0")
