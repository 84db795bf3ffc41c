"""The MCMC restatement (tests/mcmc_ref.py) against the reference's recorded
run (tests/golden/mcmc_golden.json.gz: 5500 generations, one variable, Burn In
500, 5000 samples), bit for bit, and the parts of MCMC.cpp.base no recorded run
covers: delayed rejection, adaptive sampling, the NaN and alpha == 1.0 branches
of the accept test, the asymmetric covariance recurrence.  (CPU, no GPU needed.)"""
import math

import numpy as np
import pytest

import mcmc_ref as mr

INF = float("inf")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    return mr.load_golden()


def golden_chain(g, **kw):
    c, v = g["Configuration"], g["Variables"]
    return mr.McmcRef(len(v), [x["Initial Mean"] for x in v], [x["Initial Standard Deviation"] for x in v],
                      burn_in=c["Burn In"], leap=c["Leap"], rejection_levels=c["Rejection Levels"],
                      adaptive=bool(c["Use Adaptive Sampling"]), non_adaption_period=c["Non Adaption Period"],
                      scaling=c["Chain Covariance Scaling"], max_samples=g["Max Samples"],
                      normal_seed=g["Normal Seed"], uniform_seed=g["Uniform Seed"], **kw)


def test_the_fixture_is_the_recorded_run(golden):
    g = golden
    assert [r["Current Generation"] for r in g["generations"]] == list(range(0, 5501, 500))
    assert len(g["Sample Database"]) == len(g["Sample Evaluation Database"]) == g["Max Samples"] == 5000
    assert g["Configuration"]["Burn In"] == 500 and g["Configuration"]["Rejection Levels"] == 1
    assert g["Uniform Seed"] == g["Normal Seed"] + 1  # the solver's generators in MCMC.config's order
    assert len(g["Normal Generator Range"]) == len(g["Uniform Generator Range"]) == 10000
    assert g["generations"][1]["Acceptance Count"] == 351 and g["generations"][1]["Acceptance Rate"] == 351 / 499


@pytest.mark.parametrize("exp", ["cr", "libm"])
@pytest.mark.parametrize("logp", ["model", "gaussian"])
def test_restatement_reproduces_the_recorded_run_bit_for_bit(golden, exp, logp):
    g = golden
    r = golden_chain(g, exp=exp, logp="gaussian" if logp == "gaussian" else (lambda x: -0.5 * x[0] * x[0]))
    for rec in g["generations"]:
        r.run(rec["Current Generation"] - r.generation)
        assert len(r.db) == rec["Database Size"]
        if rec["Current Generation"] == 0:
            continue  # (the reference allocates its vectors in generation 1)
        for k, want in rec.items():
            if k in ("Current Generation", "Database Size"):
                continue
            assert np.array_equal(bits(r[k]), bits(want)), (rec["Current Generation"], k)
    assert r.finished()
    assert np.array_equal(bits(r["Sample Database"]), bits(g["Sample Database"]))
    assert np.array_equal(bits(r["Sample Evaluation Database"]), bits(g["Sample Evaluation Database"]))
    assert r.accept == 3838
    assert r.normal.to_hex() == g["Normal Generator Range"]
    assert r.uniform.to_hex() == g["Uniform Generator Range"]


def test_adaptive_delayed_rejection_samples_the_target():
    """tests/statistical/samplers/mean/run-mcmc-gaussian.py's target (mean -2,
    sd 3) and its own tolerance 0.5, kept unscaled although a tenth of its
    50000 samples are drawn (sqrt(10) times the tolerance would be allowed)."""
    logp = lambda x: -0.5 * ((x[0] + 2.0) ** 2 / 9.0) - 0.5 * math.log(2 * math.pi * 9)
    r = mr.McmcRef(1, [0.0], [1.0], burn_in=100, rejection_levels=2, adaptive=True, max_samples=5000,
                   normal_seed=1227, uniform_seed=1228, logp=logp)
    while not r.finished():
        r.step()
    x = r["Sample Database"]
    assert r.generation == 5100 and x.size == 5000
    assert r.proposed > r.generation  # second-level proposals were made
    assert r.chol_failures == 0 and r["Cholesky Decomposition Chain Covariance"][0] > 0
    assert abs(np.mean(x) + 2.0) < 0.5
    assert abs(np.std(x) - 3.0) < 0.5


def test_min_with_nan_is_one():
    assert mr.min1(float("nan")) == 1.0
    assert mr.min1(0.25) == 0.25 and mr.min1(7.0) == 1.0 and mr.min1(INF) == 1.0
    for exp in (mr.exp_cr, mr.exp_libm):
        assert mr.recursive_alpha(exp, -INF, [-INF], 0)[0] == 1.0   # exp(-inf - -inf) = NaN
        assert mr.recursive_alpha(exp, -INF, [-1.0], 0)[0] == 1.0   # the first generation
        assert mr.recursive_alpha(exp, -1.0, [-INF], 0)[0] == 0.0
        # a zero numerator returns before the division (:159) ...
        assert mr.recursive_alpha(exp, -800.0, [-900.0, -800.0], 1)[0] == 0.0
        # ... a denominator that underflowed gives x / 0 = inf, and inf * 0 a NaN ratio: both 1.0
        assert mr.recursive_alpha(exp, -800.0, [-5.0, -1.0], 1)[0] == 1.0
        assert mr.recursive_alpha(exp, 0.0, [900.0, 800.0], 1)[0] == 1.0


def test_minus_infinity_against_minus_infinity_accepts_without_a_uniform():
    r = mr.McmcRef(2, [0.0, 0.0], [1.0, 1.0], logp=lambda x: -INF, normal_seed=5, uniform_seed=6)
    before = r.uniform.get_bytes()
    r.run(20)
    assert r.accept == 20 and r.leader_eval == -INF
    assert r.uniform.get_bytes() == before


def test_alpha_one_draws_no_uniform():
    """an uphill-only walk (every candidate's logP is the generation number)
    leaves the Uniform Generator where it was; a downhill step draws one"""
    count = [0.0]

    def uphill(x):
        count[0] += 1.0
        return count[0]

    r = mr.McmcRef(1, [0.0], [1.0], logp=uphill, normal_seed=11, uniform_seed=12)
    fresh = mr.refcpu.Rng(seed=12)
    r.run(50)
    assert r.accept == 50
    assert r.uniform.get_bytes() == fresh.get_bytes()
    r.logp = lambda x: 0.0  # below the leader's 50: alpha < 1
    r.run(3)
    for _ in range(3):
        fresh.get()
    assert r.uniform.get_bytes() == fresh.get_bytes()


def test_covariance_upper_triangle_differs_from_lower_at_n2():
    r = mr.McmcRef(2, [0.0, 0.0], [1.0, 0.5], normal_seed=21, uniform_seed=22)
    r.run(50)
    C = r["Chain Covariance"].reshape(2, 2)
    P = r["Chain Covariance Placeholder"].reshape(2, 2)
    assert P[0, 1] == P[1, 0]
    assert C[0, 1] != C[1, 0]
    # :213 applies the decay to the element :212 just wrote
    n = len(r.db)
    f, s = (n - 2.0) / (n - 1.0), 1.0 / n
    assert C[0, 1] == f * C[1, 0] + s * P[1, 0]


def test_early_returns_of_update_state():
    r = mr.McmcRef(2, [1.0, 2.0], [1.0, 1.0], burn_in=3, normal_seed=31, uniform_seed=32)
    r.run(3)
    assert len(r.db) == 0 and np.all(r["Chain Mean"] == 0.0)
    assert r.rate == r.accept / 2.0  # the chain length before its increment
    r.run(1)
    assert len(r.db) == 1 and np.array_equal(r["Chain Mean"], r["Chain Leader"]) and np.all(r["Chain Covariance"] == 0.0)
    r.run(1)
    assert len(r.db) == 2 and np.any(r["Chain Covariance"] != 0.0)
    one = mr.McmcRef(1, [0.0], [1.0], normal_seed=31, uniform_seed=32)
    one.run(1)
    assert one.rate == INF and one.accept == 1  # 1 / 0 in the first generation


def test_delayed_rejection_table_equals_the_recursion():
    """the device forms recursiveAlpha from a table over contiguous sub-paths;
    the same table in Python equals the literal recursion at every level"""
    rng = np.random.default_rng(3)
    for trial in range(40):
        n = int(rng.integers(1, 9))
        y = list(rng.normal(-3.0, 2.0, n + 1))
        if trial % 5 == 0:
            y[int(rng.integers(1, n + 1))] = -INF
        for level in range(n):
            want = mr.recursive_alpha(mr.exp_cr, y[0], y[1:], level)[0]
            got = mr.table_alpha(mr.exp_cr, y, level)
            assert bits(want)[0] == bits(got)[0], (trial, level, y)


def test_cholesky_failure_keeps_the_old_factor():
    r = mr.McmcRef(3, [0.0] * 3, [1.0] * 3, adaptive=True, non_adaption_period=5, normal_seed=41,
                   uniform_seed=42)  # (fewer than N + 1 samples give a singular covariance)
    r.run(20)
    old = r["Cholesky Decomposition Chain Covariance"]
    assert r.chol_failures == 0 and np.any(old != 0.0)
    r.cov[:] = np.diag([1.0, -1e6, 1.0])
    r.run(1)
    assert r.chol_failures == 1
    assert np.array_equal(bits(r["Cholesky Decomposition Chain Covariance"]), bits(old))


def test_priors_add_to_the_model_and_minus_infinity_skips_it():
    calls = []

    def model(x):
        calls.append(list(x))
        return -0.5 * x[0] * x[0]

    r = mr.McmcRef(1, [0.0], [2.0], logp=model, prior_kinds=["Uniform"], prior_min=[-1.0], prior_max=[1.0],
                   normal_seed=51, uniform_seed=52)
    r.run(200)
    assert 0 < len(calls) < 200  # candidates outside the prior never reach the model
    assert all(-1.0 <= c[0] <= 1.0 for c in calls)
    x = r["Sample Database"]
    inside = np.abs(x) <= 1.0  # (the first generation accepts -inf against -inf)
    assert inside.any() and inside[np.argmax(inside):].all()
    assert r.evaluate([0.5]) == -mr.log_cr(2.0) + -0.5 * 0.25 and r.evaluate([1.5]) == -INF
