"""Optimizer/MOCMAES through korali.Engine on the device: the configuration
of the reference's examples/optimization/multiobjective/run-mocmaes.py (dim 4,
seed 0xC0F33) cut to 30 generations, against tests/mocmaes_ref.py.  Every
comparison is exact."""
import json
import os

import numpy as np
import pytest

import mocmaes_ref as mr

pytestmark = pytest.mark.gpu

DIM, SEED, GENERATIONS = 4, 0xC0F33, 30


def model(p):
    # examples/optimization/multiobjective/_model/model.py (x*x for **2, as the kernel)
    p["F(x)"] = mr.negative_rosenbrock_and_sphere(p["Parameters"])


def experiment(path, kernel=False, generations=GENERATIONS):
    import korali
    e = korali.Experiment()
    e["Random Seed"] = SEED
    e["Problem"]["Type"] = "Optimization"
    if kernel:
        e["Problem"]["Objective Kernel"] = "negative_rosenbrock_and_sphere"
    else:
        e["Problem"]["Objective Function"] = model
    e["Problem"]["Num Objectives"] = 2
    for i in range(DIM):
        e["Variables"][i]["Name"] = "X" + str(i)
        e["Variables"][i]["Lower Bound"] = -25.0
        e["Variables"][i]["Upper Bound"] = +25.0
        e["Variables"][i]["Initial Standard Deviation"] = 3.0
    e["Solver"]["Type"] = "Optimizer/MOCMAES"
    e["Solver"]["Population Size"] = 32
    e["Solver"]["Mu Value"] = 16
    e["Solver"]["Termination Criteria"]["Min Value Difference Threshold"] = 1e-8
    e["Solver"]["Termination Criteria"]["Min Variable Difference Threshold"] = 1e-8
    e["Solver"]["Termination Criteria"]["Max Generations"] = generations
    e["Console Output"]["Verbosity"] = "Silent"
    e["File Output"]["Path"] = str(path)
    e["File Output"]["Frequency"] = 10
    return e


def read_gen(path, g):
    with open(os.path.join(path, "gen%08d.json" % g)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    """The uninterrupted run with the Python model (Sequential conduit)."""
    import korali
    path = tmp_path_factory.mktemp("mocmaes") / "python"
    e = experiment(path)
    korali.Engine().run(e)
    return path, e


@pytest.fixture(scope="module")
def restatement():
    ref = mr.Mocmaes([-25.0] * DIM, [25.0] * DIM, 32, mu=16, num_objectives=2, initial_sdev=[3.0] * DIM,
                     normal_seed=SEED, uniform_seed=SEED + 1)
    at = {}
    for g in range(1, GENERATIONS + 1):
        ref.generation()
        if g % 10 == 0:
            at[g] = mr.as_recorded(ref, names={})  # (the result files use the snapshot's names)
    return at


def solver_mismatches(sv, want):
    return mr.mismatches(lambda name: sv[name], (sv["Multinormal Generator"]["Range"], sv["Uniform Generator"]["Range"]),
                         want, None, names={})


def test_python_model_equals_the_restatement(straight, restatement):
    path, e = straight
    assert e["Current Generation"] == GENERATIONS and e["Is Finished"]
    for g in (10, 20, 30):
        sv = read_gen(path, g)["Solver"]
        assert solver_mismatches(sv, restatement[g]) == [], g
        assert sv["Num Objectives"] == 2 and sv["Population Size"] == 32 and sv["Mu Value"] == 16
        assert sv["Evolution Path Adaption Strength"] == 2. / (DIM + 2.)
        assert sv["Covariance Learning Rate"] == 2. / (DIM * DIM + 6.)
        assert sv["Infeasible Sample Count"] == 0


def test_objective_kernel_gives_identical_result_files(straight, tmp_path):
    import korali
    path, _ = straight
    e = experiment(tmp_path / "kernel", kernel=True)
    korali.Engine().run(e)
    for g in (10, 20, 30):
        a, b = read_gen(path, g), read_gen(tmp_path / "kernel", g)
        assert a["Solver"] == b["Solver"], g
        assert a.get("Results") == b.get("Results"), g


def test_pareto_optimal_samples_are_mutually_non_dominated(straight):
    path, e = straight
    res = read_gen(path, GENERATIONS)["Results"]["Pareto Optimal Samples"]
    F, X = np.array(res["F(x)"]), np.array(res["Parameters"])
    sv = read_gen(path, GENERATIONS)["Solver"]
    assert F.shape == (len(X), 2) and X.shape[1] == DIM and len(X) >= 1
    assert res["F(x)"] == sv["Sample Value Collection"] and res["Parameters"] == sv["Sample Collection"]
    for i in range(len(F)):
        assert not np.any(np.all(F > F[i], axis=1)), i  # nobody is better in every objective
        assert list(F[i]) == mr.negative_rosenbrock_and_sphere(list(X[i]))


def test_resume_at_generation_10_equals_the_uninterrupted_run(straight, tmp_path):
    import korali
    path, _ = straight
    r = korali.Experiment()
    assert r.loadState(str(path / "gen00000010.json"))
    r["Preserve Random Number Generator States"] = True
    r["Problem"]["Objective Function"] = model
    r["File Output"]["Path"] = str(tmp_path / "resumed")
    korali.Engine().run(r)
    for g in (20, 30):
        assert read_gen(path, g)["Solver"] == read_gen(tmp_path / "resumed", g)["Solver"], g
    assert read_gen(path, 30)["Results"] == read_gen(tmp_path / "resumed", 30)["Results"]


def test_concurrent_conduit_equals_sequential(straight, tmp_path):
    import korali
    path, _ = straight
    k = korali.Engine()
    k["Conduit"]["Type"] = "Concurrent"
    k["Conduit"]["Concurrent Jobs"] = 4
    k.run(experiment(tmp_path / "concurrent"))
    for g in (10, 20, 30):
        assert read_gen(path, g)["Solver"] == read_gen(tmp_path / "concurrent", g)["Solver"], g


def test_min_variable_difference_threshold_ends_a_run(tmp_path):
    """MOCMAES.config:58-61: max over the objectives of the L2 distance of
    consecutive best samples < threshold, from generation 2 on.  The optimizer
    base criteria stay disabled (setInitialConfiguration :63-65)."""
    import korali
    e = experiment(tmp_path / "threshold", kernel=True, generations=200)
    e["Solver"]["Termination Criteria"]["Min Variable Difference Threshold"] = 1e9
    e["File Output"]["Enabled"] = False
    korali.Engine().run(e)
    assert e["Current Generation"] == 1 and e["Is Finished"]
    assert max(e["Solver"]["Current Best Variable Differences"]) < 1e9


def test_min_value_difference_threshold_ends_a_run_through_the_min_max_criterion(tmp_path):
    """MOCMAES.config:52-55 as written: the criterion named 'Min Max Value
    Difference Threshold' compares |max_k Current Best Value Differences| with
    the optimizer base's 'Min Value Difference Threshold'; the key 'Min Max
    Value Difference Threshold' itself is accepted and never read.  After
    generation 1 the differences are +Inf (the previous best values are -Inf);
    after generation 2 they are finite."""
    import korali
    e = experiment(tmp_path / "value", kernel=True, generations=200)
    e["Solver"]["Termination Criteria"]["Min Value Difference Threshold"] = 1e300
    e["Solver"]["Termination Criteria"]["Min Variable Difference Threshold"] = -1.0
    e["File Output"]["Enabled"] = False
    korali.Engine().run(e)
    assert e["Current Generation"] == 2 and e["Is Finished"]
    assert abs(max(e["Solver"]["Current Best Value Differences"])) < 1e300
    # the key of the criterion's own name changes nothing
    e = experiment(tmp_path / "unread", kernel=True, generations=5)
    e["Solver"]["Termination Criteria"]["Min Value Difference Threshold"] = -1.0
    e["Solver"]["Termination Criteria"]["Min Variable Difference Threshold"] = -1.0
    e["Solver"]["Termination Criteria"]["Min Max Value Difference Threshold"] = 1e300
    e["File Output"]["Enabled"] = False
    korali.Engine().run(e)
    assert e["Current Generation"] == 5


def test_resume_rejects_a_saved_field_of_the_wrong_size(straight, tmp_path):
    import korali
    path, _ = straight
    r = korali.Experiment()
    assert r.loadState(str(path / "gen00000010.json"))
    r["Preserve Random Number Generator States"] = True
    r["Problem"]["Objective Function"] = model
    r["Solver"]["Current Sigma"] = [1.0, 2.0]  # 32 offspring
    r["File Output"]["Enabled"] = False
    with pytest.raises(korali.KoraliError, match="saved field 'Current Sigma' has 2 values"):
        korali.Engine().run(r)


def test_non_finite_objective_value_is_an_error(tmp_path):
    import korali
    e = experiment(tmp_path / "nan")
    e["Problem"]["Objective Function"] = lambda p: p.__setitem__("F(x)", [0.0, float("inf")])
    e["File Output"]["Enabled"] = False
    with pytest.raises(korali.KoraliError, match="Non finite value of function evaluation"):
        korali.Engine().run(e)
