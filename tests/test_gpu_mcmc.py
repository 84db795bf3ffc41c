"""Sampler/MCMC on the device (kg_mcmc_*, korali_amd/csrc/kg_mcmc.hip) against
the reference's recorded run (tests/golden/mcmc_golden.json.gz) and against the
restatement (tests/mcmc_ref.py): every field, the database and both generator
states.  Every comparison is on the bit patterns."""
import numpy as np
import pytest

import mcmc_ref as mr

pytestmark = pytest.mark.gpu

GENERATIONS = 300
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)).view(np.uint64)


def settings(N, priors):
    """initial values that differ per variable; steps sized for a unit Gaussian
    in N dimensions.  With priors: variable 0 Uniform and narrower than two of
    its proposal steps, so candidates fall outside it; the other kinds follow
    (LogNormal, Exponential: supports that hold the starting point)."""
    sd = np.array([(0.4 + 0.1 * (d % 7)) / np.sqrt(N) for d in range(N)])
    mean = np.array([0.05 * ((d % 5) - 2) for d in range(N)])
    if not priors:
        return mean, sd, {}
    kinds, a, b = [], [], []
    table = [("Normal", 0.0, 3.0), ("Laplace", 0.1, 2.0), ("Cauchy", -0.1, 1.5), ("Exponential", -10.0, 5.0),
             ("LogNormal", 0.0, 1.0), ("Uniform", -50.0, 50.0)]
    for d in range(N):
        k, lo, hi = ("Uniform", mean[0] - 1.5 * sd[0], mean[0] + 1.5 * sd[0]) if d == 0 else table[(d - 1) % 6]
        if k == "LogNormal":
            mean[d] = 1.0
        kinds.append(k)
        a.append(lo)
        b.append(hi)
    return mean, sd, dict(prior_kinds=kinds, prior_min=a, prior_max=b)


def pair(N, R=1, adaptive=False, burn_in=0, leap=1, priors=False, host=False, seeds=(3001, 3002), nap=5, **kw):
    from korali_amd.native import McmcDevice
    mean, sd, pk = settings(N, priors)
    dev = McmcDevice(N, mean, sd, burn_in=burn_in, leap=leap, rejection_levels=R, use_adaptive_sampling=adaptive,
                     non_adaption_period=nap, normal_seed=seeds[0], uniform_seed=seeds[1],
                     probability=None if host else "gaussian", **pk, **kw)
    ref = mr.McmcRef(N, mean, sd, burn_in=burn_in, leap=leap, rejection_levels=R, adaptive=adaptive,
                     non_adaption_period=nap, normal_seed=seeds[0], uniform_seed=seeds[1], **pk)
    return dev, ref


def compare(dev, ref, tag):
    for name in mr.FIELDS:
        got, want = dev[name], ref[name]
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (tag, name, got, want)
    assert dev.rng_state(0) == ref.normal.get_bytes(), (tag, "Normal Generator")
    assert dev.rng_state(1) == ref.uniform.get_bytes(), (tag, "Uniform Generator")


def same_state(a, b, tag):
    for name in mr.FIELDS:
        assert np.array_equal(bits(a[name]), bits(b[name])), (tag, name)
    assert a.rng_state(0) == b.rng_state(0) and a.rng_state(1) == b.rng_state(1), tag


def test_recorded_run_bit_for_bit():
    """from the seeds, 5500 generations in windows of 500: the fields at each
    recorded generation, the final databases, the exported generator states"""
    from korali_amd.native import McmcDevice
    g = mr.load_golden()
    c, v = g["Configuration"], g["Variables"]
    dev = McmcDevice(len(v), [x["Initial Mean"] for x in v], [x["Initial Standard Deviation"] for x in v],
                     burn_in=c["Burn In"], leap=c["Leap"], rejection_levels=c["Rejection Levels"],
                     use_adaptive_sampling=bool(c["Use Adaptive Sampling"]),
                     non_adaption_period=c["Non Adaption Period"],
                     chain_covariance_scaling=c["Chain Covariance Scaling"], max_samples=g["Max Samples"],
                     normal_seed=g["Normal Seed"], uniform_seed=g["Uniform Seed"])
    try:
        for rec in g["generations"][1:]:
            gen = rec["Current Generation"]
            done, stop = dev.run(gen - 499, 500)
            assert done == 500 and stop == (["Max Samples"] if gen == 5500 else [])
            assert dev.field_size("Sample Evaluation Database") == rec["Database Size"]
            for k, want in rec.items():
                if k in ("Current Generation", "Database Size"):
                    continue
                assert np.array_equal(bits(dev[k]), bits(want)), (gen, k, dev[k], want)
        X, lp = dev.database()
        assert np.array_equal(bits(X), bits(g["Sample Database"]))
        assert np.array_equal(bits(lp), bits(g["Sample Evaluation Database"]))
        assert dev.rng_state(0).hex().upper() == g["Normal Generator Range"]
        assert dev.rng_state(1).hex().upper() == g["Uniform Generator Range"]
        assert dev.run(5501, 10) == (0, ["Max Samples"])  # the database is full
        dev.synchronize()
    finally:
        dev.close()


@pytest.mark.parametrize("priors", [False, True], ids=["noprior", "priors"])
@pytest.mark.parametrize("burn_in,leap", [(0, 1), (7, 3)])
@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("N", [1, 3, 17, 64])
def test_against_the_restatement(N, R, adaptive, burn_in, leap, priors):
    dev, ref = pair(N, R, adaptive, burn_in, leap, priors)
    try:
        outside = 0
        for first, count in ((1, 150), (151, GENERATIONS - 150)):
            assert dev.run(first, count) == (count, [])
            for _ in range(count):
                ref.step()
                outside += int(ref.cand_eval[0] == -INF)
            compare(dev, ref, first + count - 1)
        dev.synchronize()
        assert not priors or outside > 0  # candidates fell outside the Uniform prior
    finally:
        dev.close()


def test_adaptive_at_64_variables_with_a_factored_covariance():
    """Non Adaption Period 5 switches to the chain's factor while the
    covariance of so few samples is still singular at N = 64: that factor is
    zero, every candidate is the leader, and the chain stands still (as the
    reference's does).  After 120 generations of the initial factor the
    covariance has full rank and the chain's factor takes over."""
    dev, ref = pair(64, R=3, adaptive=True, nap=120)
    try:
        assert dev.run(1, GENERATIONS) == (GENERATIONS, [])
        ref.run(GENERATIONS)
        compare(dev, ref, GENERATIONS)
        assert np.any(ref["Cholesky Decomposition Chain Covariance"] != 0.0)
        assert ref.accept < GENERATIONS
        dev.synchronize()
    finally:
        dev.close()


def test_eight_rejection_levels():
    dev, ref = pair(2, R=8, adaptive=True, priors=True)
    try:
        assert dev.run(1, GENERATIONS) == (GENERATIONS, [])
        ref.run(GENERATIONS)
        compare(dev, ref, GENERATIONS)
        assert ref.proposed > 3 * GENERATIONS  # the deep levels were reached
        dev.synchronize()
    finally:
        dev.close()


def test_window_sizes_and_call_cuts_change_nothing():
    kw = dict(N=17, R=3, adaptive=True, burn_in=7, leap=3)
    one, ref = pair(**kw)
    steps, _ = pair(**kw)
    sevens, _ = pair(**kw)
    tight, _ = pair(window_candidates=1, **kw)  # grown to R: the minimum that holds one generation
    try:
        assert one.run(1, GENERATIONS) == (GENERATIONS, [])
        assert one.diagnostics()[:2] == (1, 0)
        for g in range(1, GENERATIONS + 1):
            assert steps.run(g, 1) == (1, [])
        g = 1
        while g <= GENERATIONS:
            n = min(7, GENERATIONS + 1 - g)
            assert sevens.run(g, n) == (n, [])
            g += n
        assert tight.run(1, GENERATIONS) == (GENERATIONS, [])
        windows, relaunches, window = tight.diagnostics()
        assert window == 3 and relaunches > 0 and windows == relaunches + 1
        ref.run(GENERATIONS)
        compare(one, ref, "one call")
        for other, tag in ((steps, "300 x 1"), (sevens, "windows of 7"), (tight, "minimal windows")):
            same_state(one, other, tag)
            other.synchronize()
    finally:
        for d in (one, steps, sevens, tight):
            d.close()


def numpy_logp(x):
    ss = np.float64(0.0)
    for v in x:
        ss += v * v
    return float(-0.5 * ss)


@pytest.mark.parametrize("priors", [False, True], ids=["noprior", "priors"])
def test_host_evaluated_path_equals_run(priors):
    kw = dict(N=5, R=3, adaptive=True, burn_in=7, leap=3, priors=priors)
    dev, _ = pair(**kw)
    host, _ = pair(host=True, **kw)
    try:
        assert dev.run(1, 120) == (120, [])
        for g in range(1, 121):
            host.generation(g, numpy_logp)
        same_state(dev, host, "host")
        with pytest.raises(Exception, match="no builtin probability kernel"):
            host.run(121, 1)
        host.propose(0)
        with pytest.raises(Exception, match="NaN"):
            host.decide(0, float("nan"))
        host.synchronize()
    finally:
        dev.close()
        host.close()


def test_max_model_evaluations_stops_after_the_right_generation():
    dev, ref = pair(3, R=3)
    try:
        while ref.evals < 100:
            ref.step()
        assert ref.generation < ref.evals  # delayed rejection: the count depends on the data
        done, stop = dev.run(1, GENERATIONS, max_model_evaluations=100)
        assert (done, stop) == (ref.generation, ["Max Model Evaluations"])
        compare(dev, ref, done)
        dev.synchronize()
    finally:
        dev.close()


def test_cholesky_failure_keeps_the_old_factor():
    dev, ref = pair(3, adaptive=True)
    try:
        dev.run(1, 20)
        ref.run(20)
        compare(dev, ref, 20)
        old, failures = dev["Cholesky Decomposition Chain Covariance"], dev["Cholesky Failures"][0]
        assert np.any(old != 0.0)
        bad = np.diag([1.0, -1e6, 1.0])
        dev["Chain Covariance"] = bad
        ref.cov[:] = bad
        dev.run(21, 1)
        ref.run(1)
        assert dev["Cholesky Failures"][0] == failures + 1
        assert np.array_equal(bits(dev["Cholesky Decomposition Chain Covariance"]), bits(old))
        compare(dev, ref, 21)
        dev.synchronize()  # no error bit
    finally:
        dev.close()


def test_resume_from_the_fields():
    kw = dict(N=3, R=3, adaptive=True, burn_in=7, leap=3, priors=True)
    dev, ref = pair(**kw)
    fresh, _ = pair(seeds=(1, 2), **kw)
    try:
        dev.run(1, 150)
        for name in mr.FIELDS:
            fresh[name] = dev[name]
        fresh.set_rng_state(dev.rng_state(0), 0)
        fresh.set_rng_state(dev.rng_state(1), 1)
        dev.run(151, 150)
        fresh.run(151, 150)
        same_state(dev, fresh, "resumed")
        ref.run(300)
        compare(fresh, ref, 300)
        fresh.synchronize()
    finally:
        dev.close()
        fresh.close()
