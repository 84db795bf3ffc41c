"""CPU tests of the Hierarchical/Theta problem definition (korali_amd/engine):
every configuration error of Theta::initialize (problem/hierarchical/theta/
theta.cpp.base:7-57) and of this build's own shape checks, raised before any
device call; a well-formed experiment gets past configuration."""
import json

import pytest

import korali

from test_hier_engine_cpu import K, fails, finished_psi, sub_experiment


def finished_sub(nvar=2, k=K, problem="custom"):
    """A finished phase-1 experiment as its result file would hold it."""
    e = sub_experiment(nvar=nvar, k=k)
    e["Random Seed"] = 77
    if problem == "custom":
        e["Problem"]["Likelihood Model"] = lambda s: s.__setitem__("logLikelihood", -0.5 * s["Parameters"][0] ** 2)
    elif problem == "kernel":
        e["Problem"]["Likelihood Kernel"] = "Gaussian"
    elif problem == "reference":
        e["Problem"]["Type"] = "Bayesian/Reference"
        e["Problem"]["Likelihood Model"] = "Normal"
        e["Problem"]["Reference Data"] = [0.1, 0.2]
        e["Problem"]["Computational Model"] = lambda s: None
    for d in range(nvar):
        e["Variables"][d]["Prior Distribution"] = "Uniform %d" % d
        e["Distributions"][d]["Name"] = "Uniform %d" % d
        e["Distributions"][d]["Type"] = "Univariate/Uniform"
        e["Distributions"][d]["Minimum"] = -5.0
        e["Distributions"][d]["Maximum"] = 5.0
    e["Solver"]["Chain Leaders LogLikelihoods"] = [-2.0] * k
    return e


def theta_experiment(sub=None, psi=None):
    e = korali.Experiment()
    e["Problem"]["Type"] = "Hierarchical/Theta"
    e["Problem"]["Sub Experiment"] = finished_sub() if sub is None else sub
    e["Problem"]["Psi Experiment"] = finished_psi() if psi is None else psi
    e["Solver"]["Type"] = "Sampler/TMCMC"
    e["Solver"]["Population Size"] = 16
    e["File Output"]["Enabled"] = False
    e["Console Output"]["Verbosity"] = "Silent"
    return e


@pytest.mark.parametrize("key", ["Sub Experiment", "Psi Experiment"])
def test_theta_mandatory_experiments_come_first(key):
    d = json.loads(theta_experiment().dump())
    del d["Problem"][key]
    d["Problem"]["Conditional Priors"] = ["Conditional 0"]  # also unrecognised: the mandatory check wins
    e = korali.Experiment()
    for k, v in d.items():
        e[k] = v
    fails(e, r"No value provided for mandatory setting: \['%s'\] required by Theta \(the other hierarchical problems "
          "are 'Hierarchical/Psi' and 'Hierarchical/ThetaNew'\\)" % key)


def test_theta_unrecognised_key():
    e = theta_experiment()
    e["Problem"]["Conditional Priors"] = ["Conditional 0"]
    fails(e, "Unrecognized settings for Korali module: Theta")


def test_unknown_hierarchical_type_names_all_three():
    e = theta_experiment()
    e["Problem"]["Type"] = "Hierarchical/Omega"
    fails(e, "'Hierarchical/Psi', 'Hierarchical/ThetaNew' and 'Hierarchical/Theta'")


def test_theta_needs_tmcmc():
    e = theta_experiment()
    e["Solver"]["Type"] = "Optimizer/CMAES"
    fails(e, "supported with the 'Sampler/TMCMC' solver")


def test_theta_refuses_mtmcmc():
    e = theta_experiment(sub=finished_sub(problem="reference"))
    e["Solver"]["Version"] = "mTMCMC"
    fails(e, "mTMCMC works only for problems of type 'Bayesian/Reference'")


def test_theta_psi_experiment_type():
    fails(theta_experiment(psi=sub_experiment()), "Psi experiment passed is not of type Hierarchical/Psi")


def test_theta_psi_conditional_priors_are_read():
    psi = finished_psi()
    psi["Problem"]["Conditional Priors"] = ["Conditional 0", "Conditional 9"]
    fails(theta_experiment(psi=psi), "Did not find conditional prior distribution Conditional 9")


def test_theta_psi_non_finite_prior():
    psi = finished_psi()
    lp = list(psi["Solver"]["Sample LogPrior Database"])
    lp[K - 1] = float("inf")
    psi["Solver"]["Sample LogPrior Database"] = lp
    fails(theta_experiment(psi=psi), r"Non finite \(inf\) prior has been detected at sample %d in Psi problem" % (K - 1))


def test_theta_psi_database_lengths_agree():
    psi = finished_psi()
    psi["Solver"]["Chain Leaders LogLikelihoods"] = [-3.0] * (K - 1)
    fails(theta_experiment(psi=psi),
          r"psi-problem's 'Chain Leaders LogLikelihoods' \(%d\) and 'Sample Database' \(%d\)" % (K - 1, K))


def test_theta_psi_databases():
    psi = finished_psi()
    d = json.loads(psi.dump())
    del d["Solver"]["Sample LogPrior Database"]
    fails(theta_experiment(psi=d), "Error reading the sample database from the psi-problem")


def test_theta_sub_experiment_must_be_finished():
    sub = finished_sub()
    sub["Is Finished"] = False
    fails(theta_experiment(sub=sub), r"\(Theta\) requires that the sub problem has run completely, but this one has not")


def test_theta_sub_experiment_problem_type():
    sub = finished_sub()
    sub["Problem"]["Type"] = "Optimization"
    fails(theta_experiment(sub=sub), "'Sub Experiment' whose problem is of type 'Bayesian/Custom' or 'Bayesian/Reference'")


def test_theta_sub_non_finite_prior():
    sub = finished_sub()
    lp = list(sub["Solver"]["Sample LogPrior Database"])
    lp[2] = float("inf")
    sub["Solver"]["Sample LogPrior Database"] = lp
    fails(theta_experiment(sub=sub), r"Non finite \(inf\) prior has been detected at sample 2 in sub problem")


def test_theta_sub_variable_count():
    fails(theta_experiment(sub=finished_sub(nvar=3)), "sub-problem has 3 variables, the psi-problem 2 conditional priors")


def test_theta_sub_database_lengths_agree():
    sub = finished_sub()
    sub["Solver"]["Chain Leaders LogLikelihoods"] = [-2.0] * (K + 1)
    fails(theta_experiment(sub=sub),
          r"sub-problem's 'Chain Leaders LogLikelihoods' \(%d\) and 'Sample Database' \(%d\)" % (K + 1, K))


@pytest.mark.parametrize("key", ["Sample Database", "Sample LogPrior Database", "Sample LogLikelihood Database"])
def test_theta_sub_databases(key):
    d = json.loads(finished_sub(problem="kernel").dump())
    del d["Solver"][key]
    fails(theta_experiment(sub=d), "Error reading the sample database from the sub-problem. Was it a sampling experiment?")


def test_theta_sub_problem_needs_its_function():
    d = json.loads(finished_sub(problem="kernel").dump())
    del d["Problem"]["Likelihood Kernel"]
    fails(theta_experiment(sub=d), "Problem 'Bayesian/Custom' requires a 'Likelihood Model'")
    d = json.loads(finished_sub(problem="reference").dump())
    del d["Problem"]["Computational Model"]
    fails(theta_experiment(sub=d), "Problem 'Bayesian/Reference' requires a 'Computational Model' function")
    d = json.loads(finished_sub(problem="reference").dump())
    d["Problem"]["Reference Data"] = []
    fails(theta_experiment(sub=d), r"Bayesian \(Normal\) problems require defining reference data")


def test_theta_refuses_the_distributed_conduit(monkeypatch):
    for v in ("RANK", "WORLD_SIZE"):
        monkeypatch.delenv(v, raising=False)
    e = theta_experiment()
    k = korali.Engine()
    k["Conduit"]["Type"] = "Distributed"
    k["Conduit"]["Transport"] = "Host"  # one rank: no sockets
    with pytest.raises(korali.KoraliError, match="'Hierarchical/Theta' are out of scope for the Distributed conduit"):
        k.run(e)


@pytest.mark.parametrize("problem", ["custom", "kernel", "reference"])
def test_theta_well_formed_gets_past_configuration(problem):
    """Without a GPU the run fails at device creation, with one it finishes;
    either way no configuration error is raised."""
    e = theta_experiment(sub=finished_sub(problem=problem))
    e["Solver"]["Termination Criteria"]["Max Generations"] = 1
    try:
        korali.Engine().run(e)
    except korali.KoraliError as err:
        msg = str(err)
        assert "hip" in msg.lower() or "device" in msg.lower() or "gpu" in msg.lower(), msg
        for word in ("Theta", "Hierarchical", "mandatory", "Unrecognized", "sub-problem", "psi-problem"):
            assert word not in msg, msg
