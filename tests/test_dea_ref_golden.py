"""The NumPy restatement of DEA (tests/dea_ref.py) against the reference's
recorded run (tests/golden/dea_golden.json.gz, 24 generation files of
examples/optimization/stochastic/run-dea.py): bit for bit, so the GPU tests
may use the restatement as their oracle at other shapes and rules."""
import numpy as np
import pytest

import dea_ref
from dea_ref import SCALARS, VECTORS


@pytest.fixture(scope="module")
def gens():
    return dea_ref.load_golden()


def assert_state(ref, sv, what):
    for k in VECTORS:
        a, b = np.asarray(ref[k], dtype=np.float64), np.asarray(sv[k], dtype=np.float64)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {k}"
    for k in SCALARS:
        assert float(ref[k]) == float(sv[k]), f"{what}: {k}"


def test_generation_1_from_the_seed(gens):
    g1 = gens[1]
    sv = g1["Solver"]
    ref = dea_ref.from_golden(g1)
    ref.rng = dea_ref.GslStream(seed=sv["Uniform Generator"]["Random Seed"])
    assert dea_ref.GslStream(seed=sv["Uniform Generator"]["Random Seed"]).hex() == \
        gens[0]["Solver"]["Uniform Generator"]["Range"]
    assert dea_ref.GslStream(seed=sv["Normal Generator"]["Random Seed"]).hex() == sv["Normal Generator"]["Range"]
    ref["Model Evaluation Count"] = 0
    ref.generation(1, dea_ref.negative_rosenbrock)
    assert_state(ref, sv, "generation 1")
    assert ref.rng.hex() == sv["Uniform Generator"]["Range"]
    assert ref.rng.words == 32 * 10


@pytest.mark.parametrize("k", range(1, 23))
def test_teacher_forced_transition(gens, k):
    """State k -> k + 1: candidates, exported generator state, population,
    mean, distances, best index, infeasible count."""
    cur, nxt = gens[k], gens[k + 1]["Solver"]
    ref = dea_ref.from_golden(cur)
    ref.prepare(k + 1)
    assert np.array_equal(ref["Candidate Population"], np.array(nxt["Candidate Population"]))
    assert ref["Infeasible Sample Count"] == nxt["Infeasible Sample Count"]
    assert ref.rng.hex() == nxt["Uniform Generator"]["Range"]
    # every recorded value is the example's Python objective on the recorded candidates
    F = [dea_ref.negative_rosenbrock(x) for x in ref.candidates()]
    assert F == nxt["Value Vector"]
    ref.update(nxt["Value Vector"])
    assert_state(ref, nxt, f"generation {k + 1}")


def test_recorded_infeasible_counts_exercise_the_retry_path(gens):
    per_gen = [gens[g]["Solver"]["Infeasible Sample Count"] - gens[g - 1]["Solver"]["Infeasible Sample Count"]
               for g in range(2, 24)]
    assert per_gen[0] == 27 and min(per_gen) >= 1


def test_termination_at_generation_23(gens):
    """Min Value Difference Threshold (1e-12) is met after generation 23 and
    after no earlier one; the recorded results are the best-ever sample."""
    for g in range(2, 24):
        sv = gens[g]["Solver"]
        met = abs(sv["Current Best Value"] - sv["Previous Best Value"]) < \
            sv["Termination Criteria"]["Min Value Difference Threshold"]
        assert met == (g == 23)
        assert bool(gens[g]["Is Finished"]) == (g == 23)
    last = gens[23]
    assert last["Results"]["Best Sample"]["F(x)"] == last["Solver"]["Best Ever Value"]
    assert last["Results"]["Best Sample"]["Parameters"] == last["Solver"]["Best Ever Variables"]
