"""Sampler/MCMC and the Sampling problem through korali.Engine on the device,
against the restatement (tests/mcmc_ref.py) driven with the seeds the engine
assigned: the configuration of the reference's
examples/bayesian.inference/reference/run-mcmc.py, a Python Probability
Function against the device's kernel, result files under windowed execution,
resume from a result file, Concurrent against Sequential."""
import json

import numpy as np
import pytest

import mcmc_ref as mr

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
N = 5


def value(x):
    return x.get() if hasattr(x, "get") and not isinstance(x, dict) else x  # (an experiment's node, or parsed JSON)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)).view(np.uint64)


def state(sv):
    sv = value(sv)
    return {k: np.asarray(v, dtype=np.float64).reshape(-1) for k, v in sv.items()
            if isinstance(v, (list, int, float)) and not isinstance(v, bool)}


def same_states(a, b):
    a, b = state(a), state(b)
    assert a.keys() == b.keys()
    return [k for k in a if not np.array_equal(bits(a[k]), bits(b[k]))]


def mismatches(sv, ref):
    sv = state(sv)
    return [k for k in mr.FIELDS if k not in sv or not np.array_equal(bits(sv[k]), bits(ref[k]))]


def gaussian(s):
    ss = 0.0
    for v in s["Parameters"]:
        ss += v * v
    s["logP(x)"] = -0.5 * ss


def sampling(kernel=True, samples=200, path=None, frequency=50, verbosity="Silent", **solver):
    import korali
    e = korali.Experiment()
    e["Random Seed"] = SEED
    e["Problem"]["Type"] = "Sampling"
    if kernel:
        e["Problem"]["Probability Kernel"] = "Gaussian"
    else:
        e["Problem"]["Probability Function"] = gaussian
    for i in range(N):
        e["Variables"][i]["Name"] = "X" + str(i)
        e["Variables"][i]["Initial Mean"] = 0.1 * i
        e["Variables"][i]["Initial Standard Deviation"] = 0.3 + 0.1 * i
    e["Solver"]["Type"] = "Sampler/MCMC"
    for k, v in dict({"Burn In": 20, "Leap": 2, "Rejection Levels": 3, "Use Adaptive Sampling": True,
                      "Non Adaption Period": 10}, **solver).items():
        e["Solver"][k] = v
    e["Solver"]["Termination Criteria"]["Max Samples"] = samples
    e["Console Output"]["Verbosity"] = verbosity
    if path is None:
        e["File Output"]["Enabled"] = False
    else:
        e["File Output"]["Path"] = str(path)
        e["File Output"]["Frequency"] = frequency
    return e


def sampling_restatement(samples=200):
    """no distributions: the solver's generators take the seeds in MCMC.config's order, Normal then Uniform"""
    r = mr.McmcRef(N, [0.1 * i for i in range(N)], [0.3 + 0.1 * i for i in range(N)], burn_in=20, leap=2,
                   rejection_levels=3, adaptive=True, non_adaption_period=10, max_samples=samples,
                   normal_seed=SEED, uniform_seed=SEED + 1)
    while not r.finished():
        r.step()
    return r


@pytest.fixture(scope="module")
def windowed(tmp_path_factory):
    """the device's kernel, result files every 50 generations, nothing printed: windows of 50 generations"""
    import korali
    path = tmp_path_factory.mktemp("mcmc") / "windowed"
    e = sampling(path=path)
    korali.Engine().run(e)
    return e, path, sampling_restatement()


def test_sampling_kernel_equals_the_restatement(windowed):
    e, _, ref = windowed
    assert value(e["Current Generation"]) == ref.generation == 20 + 2 * 200
    assert mismatches(e["Solver"], ref) == []
    assert value(e["Solver"]["Normal Generator"]["Range"]) == ref.normal.to_hex()
    assert value(e["Solver"]["Uniform Generator"]["Range"]) == ref.uniform.to_hex()
    assert np.array_equal(bits(value(e["Results"]["Sample Database"])), bits(ref["Sample Database"]))
    assert value(e["Is Finished"]) is True


def test_python_probability_function_equals_the_kernel(windowed):
    import korali
    e = sampling(kernel=False)
    korali.Engine().run(e)
    assert same_states(e["Solver"], windowed[0]["Solver"]) == []
    assert value(e["Results"]) == value(windowed[0]["Results"])
    assert value(e["Current Generation"]) == value(windowed[0]["Current Generation"])


def test_non_finite_probability_is_the_reference_error():
    import korali

    def broken(s):
        s["logP(x)"] = float("-inf")

    e = sampling(kernel=False)
    e["Problem"]["Probability Function"] = broken
    with pytest.raises(korali.KoraliError, match="Non finite value of evaluation detected: -inf"):
        korali.Engine().run(e)


def test_result_files_under_windows_equal_those_of_single_steps(windowed, tmp_path):
    """Frequency 1 and Detailed console output make every generation its own launch"""
    import korali
    e, path, _ = windowed
    single = sampling(path=tmp_path / "single", frequency=1)
    korali.Engine().run(single)
    assert same_states(single["Solver"], e["Solver"]) == []
    last = value(e["Current Generation"])
    for g in list(range(0, last + 1, 50)) + [last]:
        name = "gen%08d.json" % g
        with open(path / name) as f, open(tmp_path / "single" / name) as h:
            a, b = json.load(f), json.load(h)
        assert a["Current Generation"] == b["Current Generation"] == g
        assert a["Is Finished"] == b["Is Finished"]
        assert same_states(a["Solver"], b["Solver"]) == [], name
        for gen in ("Normal Generator", "Uniform Generator"):
            assert a["Solver"][gen] == b["Solver"][gen], (name, gen)
        assert a.get("Results") == b.get("Results")


@pytest.mark.parametrize("criterion,limit,generations", [("Max Generations", 137, 137), ("Max Model Evaluations", 150, None)])
def test_termination_inside_a_window(criterion, limit, generations):
    import korali
    e, s = sampling(samples=5000), sampling(samples=5000, verbosity="Normal")
    for x in (e, s):
        x["Solver"]["Termination Criteria"][criterion] = limit
    s["Console Output"]["Frequency"] = 1  # every generation is read: single steps
    korali.Engine().run(e)
    korali.Engine().run(s)
    assert value(e["Current Generation"]) == value(s["Current Generation"])
    assert generations is None or value(e["Current Generation"]) == generations
    assert value(e["Solver"]["Model Evaluation Count"]) >= (limit if generations is None else 0)
    assert same_states(e["Solver"], s["Solver"]) == []


def test_resume_from_a_result_file_reaches_the_same_end(windowed):
    import korali
    e, path, ref = windowed
    r = korali.Experiment()
    assert r.loadState(str(path / "gen00000100.json"))
    r["Preserve Random Number Generator States"] = True
    r["File Output"]["Enabled"] = False
    korali.Engine().run(r)
    assert mismatches(r["Solver"], ref) == []
    assert same_states(r["Solver"], e["Solver"]) == []
    assert value(r["Results"]) == value(e["Results"])
    assert value(r["Current Generation"]) == value(e["Current Generation"])


def test_concurrent_equals_sequential(windowed):
    import korali
    c = sampling(kernel=False)
    k = korali.Engine()
    k["Conduit"]["Type"] = "Concurrent"
    k["Conduit"]["Concurrent Jobs"] = 4
    k.run(c)
    assert same_states(c["Solver"], windowed[0]["Solver"]) == []
    assert value(c["Results"]) == value(windowed[0]["Results"])


# examples/bayesian.inference/reference: _model/model.py's data and linear model, run-mcmc.py's configuration
Y = [3.21, 4.14, 4.94, 6.06, 6.84]
X = [1.0, 2.0, 3.0, 4.0, 5.0]


def linear(s):
    a, b, sig = s["Parameters"]
    s["Reference Evaluations"] = [a * x + b for x in X]
    s["Standard Deviation"] = [sig] * len(X)


def test_the_reference_example_with_burn_in_50_and_200_samples(tmp_path):
    import korali
    from korali_amd import libkorali

    def loglik(x):
        a, b, sig = x
        return libkorali._reference_loglikelihood(
            "Normal", Y, {"Reference Evaluations": [a * t + b for t in X], "Standard Deviation": [sig] * len(X)})

    e = korali.Experiment()
    e["Random Seed"] = SEED
    e["Problem"]["Type"] = "Bayesian/Reference"
    e["Problem"]["Likelihood Model"] = "Normal"
    e["Problem"]["Reference Data"] = Y
    e["Problem"]["Computational Model"] = linear
    e["Solver"]["Type"] = "Sampler/MCMC"
    e["Solver"]["Burn In"] = 50
    e["Solver"]["Termination Criteria"]["Max Samples"] = 200
    e["Distributions"][0]["Name"] = "Uniform 0"
    e["Distributions"][0]["Type"] = "Univariate/Uniform"
    e["Distributions"][0]["Minimum"] = 0.0
    e["Distributions"][0]["Maximum"] = +5.0
    for i, name in enumerate(["a", "b", "[Sigma]"]):
        e["Variables"][i]["Name"] = name
        e["Variables"][i]["Prior Distribution"] = "Uniform 0"
        e["Variables"][i]["Initial Mean"] = 2.0
        e["Variables"][i]["Initial Standard Deviation"] = 0.2
    e["Store Sample Information"] = True
    e["File Output"]["Path"] = str(tmp_path / "_korali_result_mcmc")
    e["Console Output"]["Verbosity"] = "Silent"
    e["File Output"]["Frequency"] = 500
    e["Console Output"]["Frequency"] = 500
    korali.Engine().run(e)
    # the distribution takes the first seed, then the Normal and the Uniform Generator
    ref = mr.McmcRef(3, [2.0] * 3, [0.2] * 3, burn_in=50, max_samples=200, normal_seed=SEED + 1, uniform_seed=SEED + 2,
                     logp=loglik, prior_kinds=["Uniform"] * 3, prior_min=0.0, prior_max=5.0)
    while not ref.finished():
        ref.step()
    assert value(e["Current Generation"]) == ref.generation == 250
    assert mismatches(e["Solver"], ref) == []
    with open(tmp_path / "_korali_result_mcmc" / "gen00000250.json") as f:
        last = json.load(f)
    assert last["Is Finished"] and mismatches(last["Solver"], ref) == []
    assert last["Solver"]["Normal Generator"]["Range"] == ref.normal.to_hex()
    assert last["Solver"]["Uniform Generator"]["Range"] == ref.uniform.to_hex()
    assert np.array_equal(bits(last["Results"]["Sample Database"]), bits(ref["Sample Database"]))
    sv = last["Solver"]
    assert (sv["Burn In"], sv["Leap"], sv["Rejection Levels"], sv["Use Adaptive Sampling"]) == (50, 1, 1, False)
    assert sv["Variable Count"] == 3 and sv["Rejection Alphas"] == [0.0] and len(sv["Chain Candidate"]) == 1
    assert sv["Termination Criteria"]["Max Samples"] == 200
