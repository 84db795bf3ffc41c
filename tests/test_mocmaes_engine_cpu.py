"""Optimizer/MOCMAES through korali.Engine: configuration errors raised before
any device call (CPU, no GPU needed)."""
import pytest

import korali


def base_mocmaes():
    e = korali.Experiment()
    e["Problem"]["Type"] = "Optimization"
    e["Problem"]["Objective Function"] = lambda s: None
    e["Problem"]["Num Objectives"] = 2
    for i in range(2):
        e["Variables"][i]["Name"] = "X" + str(i)
        e["Variables"][i]["Lower Bound"] = -1.0
        e["Variables"][i]["Upper Bound"] = 1.0
    e["Solver"]["Type"] = "Optimizer/MOCMAES"
    e["Solver"]["Population Size"] = 8
    e["File Output"]["Enabled"] = False
    e["Console Output"]["Verbosity"] = "Silent"
    return e


def test_num_objectives_must_exceed_one():
    e = base_mocmaes()
    e["Problem"]["Num Objectives"] = 1
    with pytest.raises(korali.KoraliError, match="Problem requires multiple objectives, 'Num Objectives' is set to 1"):
        korali.Engine().run(e)


def test_num_objectives_is_required():
    e = korali.Experiment()
    e["Problem"]["Type"] = "Optimization"
    e["Problem"]["Objective Function"] = lambda s: None
    e["Variables"][0]["Name"] = "X"
    e["Variables"][0]["Lower Bound"] = -1.0
    e["Variables"][0]["Upper Bound"] = 1.0
    e["Solver"]["Type"] = "Optimizer/MOCMAES"
    e["File Output"]["Enabled"] = False
    with pytest.raises(korali.KoraliError, match="requires multiple objectives"):
        korali.Engine().run(e)


@pytest.mark.parametrize("where,key,value,msg", [
    ("Solver", "Sigma Bounded", True, "Unrecognized settings for Korali module: MOCMAES"),
    ("Termination", "Max Condition Covariance Matrix", 1e8, "Unrecognized settings for Korali module: MOCMAES"),
    ("Problem", "Objectives", 2, "Unrecognized settings for Korali module: Optimization"),
    ("Solver", "Mu Value", 9, r"Number of parents \('Mu Value' 9\) must be smaller or equal with population size \(8\)"),
    ("Problem", "Objective Kernel", "Negative Sphere", "Unknown multi-objective 'Objective Kernel'"),
    ("Problem", "Objective Kernel", "negative_rosenbrock_and_two_spheres", "has 3 objectives, 'Num Objectives' is 2"),
])
def test_configuration_errors_before_device(where, key, value, msg):
    e = base_mocmaes()
    if where == "Termination":
        e["Solver"]["Termination Criteria"][key] = value
    else:
        e[where][key] = value
    with pytest.raises(korali.KoraliError, match=msg):
        korali.Engine().run(e)


def test_needs_an_optimization_problem():
    e = base_mocmaes()
    e["Problem"]["Type"] = "Bayesian/Custom"
    with pytest.raises(korali.KoraliError, match="incompatible with MO-CMAES"):
        korali.Engine().run(e)


def test_distributed_conduit_is_not_provided(monkeypatch):
    for v in ("RANK", "WORLD_SIZE"):
        monkeypatch.delenv(v, raising=False)
    k = korali.Engine()
    k["Conduit"]["Type"] = "Distributed"
    k["Conduit"]["Transport"] = "Host"  # one rank: no sockets
    with pytest.raises(korali.KoraliError, match="Optimizer/MOCMAES does not shard across ranks"):
        k.run(base_mocmaes())


def test_type_string_ignores_case_and_whitespace():
    e = base_mocmaes()
    e["Solver"]["Type"] = " optimizer / mocmaes "
    e["Solver"]["Mu Value"] = 9
    with pytest.raises(korali.KoraliError, match="Number of parents"):
        korali.Engine().run(e)


def test_other_solvers_keep_their_answer_to_num_objectives():
    """CMA-ES accepts the key and ignores it, as before this solver existed:
    the run reaches CMA-ES's own validation."""
    e = base_mocmaes()
    e["Solver"]["Type"] = "Optimizer/CMAES"
    e["Solver"]["Population Size"] = 1
    with pytest.raises(korali.KoraliError, match="'Population Size' must be larger 1"):
        korali.Engine().run(e)
