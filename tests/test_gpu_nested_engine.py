"""Sampler/Nested through korali.Engine on the device: the Gaussian with a
known evidence, the same run with a Python likelihood, Concurrent against
Sequential, resume from a result file, both settings of Add Live Points and
a Bayesian/Reference problem, each against the NumPy restatement
(tests/nested_ref.py) driven with the seeds the engine assigned."""
import json
import math

import numpy as np
import pytest

import nested_ref as nr

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
A, N, L = 5.0, 3, 500
LOG_Z = N * math.log(math.sqrt(2 * math.pi) * math.erf(A / math.sqrt(2)) / (2 * A))
H = N * (math.log(2 * A) - 0.5 * math.log(2 * math.pi * math.e))
BOUND = 4 * math.sqrt(H / L)  # as tests/test_nested_ref_cpu.py
SHORT = 400  # generations of the runs that are only compared with one another and the restatement


def gaussian(s):
    ss = 0.0
    for v in s["Parameters"]:
        ss += v * v
    s["logLikelihood"] = -0.5 * ss


def gaussian_rows(theta):
    return [-0.5 * sum_squares(x) for x in theta]


def sum_squares(x):
    ss = 0.0
    for v in x:
        ss += float(v) * float(v)
    return ss


def experiment(kernel=True, generations=None, path=None, frequency=200, **solver):
    import korali
    e = korali.Experiment()
    e["Random Seed"] = SEED
    e["Problem"]["Type"] = "Bayesian/Custom"
    if kernel:
        e["Problem"]["Likelihood Kernel"] = "gaussian"
    else:
        e["Problem"]["Likelihood Model"] = gaussian
    e["Distributions"][0]["Name"] = "Uniform 0"
    e["Distributions"][0]["Type"] = "Univariate/Uniform"
    e["Distributions"][0]["Minimum"] = -A
    e["Distributions"][0]["Maximum"] = A
    for i in range(N):
        e["Variables"][i]["Name"] = "X" + str(i)
        e["Variables"][i]["Prior Distribution"] = "Uniform 0"
    e["Solver"]["Type"] = "Sampler/Nested"
    e["Solver"]["Number Live Points"] = L
    for k, v in solver.items():
        e["Solver"][k] = v
    if generations:
        e["Solver"]["Termination Criteria"]["Max Generations"] = generations
    e["Console Output"]["Verbosity"] = "Silent"
    if path is None:
        e["File Output"]["Enabled"] = False
    else:
        e["File Output"]["Path"] = str(path)
        e["File Output"]["Frequency"] = frequency
    return e


def restatement(generations=None, likelihood="gaussian", seed0=SEED + 1, **kw):
    """the engine seeds the distribution first, then the solver's generators in
    Nested.config order (Uniform, Normal, Multivariate), then _shuffleSeed (:61)"""
    from korali_amd.native import nested_permutation
    kw.setdefault("prior_min", -A)
    kw.setdefault("prior_max", A)
    pmin, pmax = kw.pop("prior_min"), kw.pop("prior_max")
    r = nr.NestedRef(N, L, pmin, pmax, uniform_seed=seed0, normal_seed=seed0 + 1, shuffle_seed=seed0 + 3,
                     likelihood=likelihood, **kw)
    g = r.run(generations or 10**9)
    r.finalize(nested_permutation)
    return r, g


def value(x):
    return x.get() if hasattr(x, "get") else x


def state(sv):
    sv = value(sv)
    return {k: np.asarray(v, dtype=np.float64).reshape(-1) for k, v in sv.items()
            if isinstance(v, (list, int, float)) and not isinstance(v, bool)}


def mismatches(e, ref):
    sv, res = state(e["Solver"]), value(e["Results"])
    bad = [k for k in ref.field_names() if k in sv and not np.array_equal(sv[k], ref[k])]
    bad += [k for k in ref.field_names() if k not in sv]
    bad += [k for k in nr.POSTERIOR if not np.array_equal(np.asarray(res[k], dtype=np.float64).reshape(-1), ref[k])]
    return bad


@pytest.fixture(scope="module")
def analytic():
    import korali
    e = experiment()
    korali.Engine().run(e)
    return e, restatement()


def test_gaussian_evidence_is_within_skillings_bound(analytic):
    e, (ref, generations) = analytic
    assert abs(value(e["Solver"]["LogEvidence"]) - LOG_Z) <= BOUND
    assert value(e["Current Generation"]) == generations
    P = np.asarray(value(e["Results"]["Posterior Samples Database"]))
    assert np.all(np.abs(P.mean(axis=0)) <= 0.1) and np.all(np.abs(P.std(axis=0, ddof=1) - 1.0) <= 0.1)


def test_gaussian_run_equals_the_restatement(analytic):
    e, (ref, _) = analytic
    assert mismatches(e, ref) == []
    assert value(e["Solver"]["Uniform Generator"]["Range"]) == ref.uniform.to_hex()
    assert value(e["Solver"]["Normal Generator"]["Range"]) == ref.normal.to_hex()


@pytest.fixture(scope="module")
def short(tmp_path_factory):
    import korali
    path = tmp_path_factory.mktemp("nested") / "straight"
    e = experiment(generations=SHORT, path=path)
    korali.Engine().run(e)
    return e, path, restatement(SHORT)[0]


def test_short_run_equals_the_restatement(short):
    e, _, ref = short
    assert mismatches(e, ref) == []


def test_python_likelihood_gives_the_same_run(short):
    import korali
    e = experiment(kernel=False, generations=SHORT)
    korali.Engine().run(e)
    assert mismatches(e, short[2]) == []


def test_concurrent_equals_sequential(short):
    import korali
    e = experiment(kernel=False, generations=SHORT, **{"Batch Size": 8})
    korali.Engine().run(e)
    c = experiment(kernel=False, generations=SHORT, **{"Batch Size": 8})
    k = korali.Engine()
    k["Conduit"]["Type"] = "Concurrent"
    k["Conduit"]["Concurrent Jobs"] = 4
    k.run(c)
    a, b = state(e["Solver"]), state(c["Solver"])
    assert a.keys() == b.keys() and [n for n in a if not np.array_equal(a[n], b[n])] == []
    assert value(e["Results"]) == value(c["Results"])


def test_resume_from_a_result_file_is_bit_exact(short, tmp_path):
    import korali
    e, path, ref = short
    r = korali.Experiment()
    assert r.loadState(str(path / "gen00000200.json"))
    r["Preserve Random Number Generator States"] = True
    r["File Output"]["Enabled"] = False
    korali.Engine().run(r)
    assert mismatches(r, ref) == []
    a, b = state(e["Solver"]), state(r["Solver"])
    assert a.keys() == b.keys() and [n for n in a if not np.array_equal(a[n], b[n])] == []
    assert value(e["Results"]) == value(r["Results"])
    with open(path / "gen00000200.json") as f:
        saved = json.load(f)["Solver"]
    assert saved["Number Dead Samples"] == len(saved["Dead LogWeights"]) and len(saved["Live Samples"]) == L


def test_without_add_live_points():
    import korali
    e = experiment(generations=100, **{"Add Live Points": False, "Resampling Method": "Box"})
    korali.Engine().run(e)
    ref, _ = restatement(100, add_live_points=False, method="Box")
    assert mismatches(e, ref) == []
    assert value(e["Solver"]["Number Dead Samples"]) == 99


# tests/statistical/bayesian/_model/model.py: getReferenceData / getReferencePoints, the linear model
Y = [3.21, 4.14, 4.94, 6.06, 6.84]
X = [1.0, 2.0, 3.0, 4.0, 5.0]


def linear(s):
    a, b, sig = s["Parameters"]
    s["Reference Evaluations"] = [a * x + b for x in X]
    s["Standard Deviation"] = [sig] * len(X)


def test_bayesian_reference_with_the_normal_model():
    import korali
    from korali_amd import libkorali

    def loglik(theta):
        return [libkorali._reference_loglikelihood(
            "Normal", Y, {"Reference Evaluations": [float(a) * x + float(b) for x in X],
                          "Standard Deviation": [float(sig)] * len(X)}) for a, b, sig in theta]

    e = korali.Experiment()
    e["Random Seed"] = SEED
    e["Problem"]["Type"] = "Bayesian/Reference"
    e["Problem"]["Likelihood Model"] = "Normal"
    e["Problem"]["Reference Data"] = Y
    e["Problem"]["Computational Model"] = linear
    e["Distributions"][0]["Name"] = "Uniform 0"
    e["Distributions"][0]["Type"] = "Univariate/Uniform"
    e["Distributions"][0]["Minimum"] = 0.0
    e["Distributions"][0]["Maximum"] = 5.0
    for i, name in enumerate(["a", "b", "[Sigma]"]):
        e["Variables"][i]["Name"] = name
        e["Variables"][i]["Prior Distribution"] = "Uniform 0"
    e["Solver"]["Type"] = "Sampler/Nested"
    e["Solver"]["Resampling Method"] = "Ellipse"
    e["Solver"]["Number Live Points"] = L
    e["Solver"]["Termination Criteria"]["Max Generations"] = 50
    e["Console Output"]["Verbosity"] = "Silent"
    e["File Output"]["Enabled"] = False
    korali.Engine().run(e)
    ref, _ = restatement(50, likelihood=loglik, prior_min=0.0, prior_max=5.0)
    assert mismatches(e, ref) == []
