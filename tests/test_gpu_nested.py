"""Sampler/Nested on the device (kg_nested_*, korali_amd/csrc/kg_nested.hip)
against the NumPy restatement (tests/nested_ref.py): every field and both
generators after the first generation and after each of 30 more, at
Proposal Update Frequency 10 so that the bounds update several times.  Every
comparison is exact."""
import numpy as np
import pytest

import nested_ref as nr

pytestmark = pytest.mark.gpu

GENERATIONS = 30


def pair(method, L, N, B, window_tries=0, **kw):
    from korali_amd.native import NestedDevice
    kw.setdefault("prior_min", -5.0)
    kw.setdefault("prior_max", 5.0)
    kw.setdefault("proposal_update_frequency", 10)
    kw.setdefault("uniform_seed", 1011)
    kw.setdefault("normal_seed", 2022)
    pmin, pmax = kw.pop("prior_min"), kw.pop("prior_max")
    fn = kw.pop("model", None)
    dev = NestedDevice(N, L, pmin, pmax, batch_size=B, method=method, window_tries=window_tries,
                       likelihood=None if fn else "gaussian", **kw)
    ref = nr.NestedRef(N, L, pmin, pmax, batch_size=B, method=method, block_tries=window_tries,
                       likelihood=fn if fn else "gaussian", **kw)
    return dev, ref


def compare(dev, ref, tag, posterior=False):
    for name in ref.field_names(posterior):
        got, want = dev[name], ref[name]
        assert got.shape == want.shape and np.array_equal(got, want), (tag, name, got, want)
    assert dev.rng_state(1) == ref.uniform.get_bytes(), (tag, "Uniform Generator")
    assert dev.rng_state(0) == ref.normal.get_bytes(), (tag, "Normal Generator")


def dev_generation(dev, g, fn):
    """one generation with the caller's likelihood (Nested.cpp.base:167-201)"""
    if fn is None:
        return dev.generation(g)
    while True:
        dev.prepare(g)
        dev.set_evaluations(fn(dev.candidates()))
        accepted, terminated = dev.process(g)
        if accepted:
            return terminated


def run_both(dev, ref, fn=None, generations=GENERATIONS):
    try:
        dev_generation(dev, 1, fn)
        ref.first_generation()
        compare(dev, ref, 1)
        for g in range(2, 2 + generations):
            dev_generation(dev, g, fn)
            ref.generation()
            compare(dev, ref, g)
        dev.synchronize()
    finally:
        dev.close()


# method, L, N, B, Ellipsoidal Scaling.  At N = 64 the ellipsoid that bounds
# uniform points reaches far outside the unit cube (about 3e5 tries per
# candidate at scaling 1); scaling 0.1 keeps the try count in the hundreds and
# takes the other branch of :866 (the volume floor) on the way.
SHAPES = [
    ("Box", 8, 1, 1, 1.0),         # smallest
    ("Box", 100, 2, 7, 1.0),       # non-power-of-two L; B dividing nothing
    ("Ellipse", 4, 4, 1, 1.0),     # the num <= dim branch
    ("Ellipse", 64, 3, 1, 1.0),    # smallest full-covariance case
    ("Ellipse", 257, 64, 3, 0.1),  # the N cap; L just past a wave multiple
    ("Ellipse", 1500, 5, 64, 1.0),  # the example's L with a real batch
]


@pytest.mark.parametrize("method,L,N,B,scaling", SHAPES)
def test_every_field_matches_the_restatement(method, L, N, B, scaling):
    dev, ref = pair(method, L, N, B, ellipsoidal_scaling=scaling)
    run_both(dev, ref)


NON_UNIFORM = {
    "normal-lognormal-uniform": (
        dict(prior_min=[0.0, 0.0, -1.0], prior_max=[1.0, 0.5, 2.0], prior_kinds=["Normal", "LogNormal", "Uniform"],
             lower_bound=[-3.0, 0.1, 0.0], upper_bound=[3.0, 4.0, 0.0]),
        [-3.0, 0.1, -1.0], [6.0, 3.9, 3.0]),
    # the Exponential's bounds start below its location: the first live set has -inf log-priors
    "exponential-laplace-cauchy": (
        dict(prior_min=[0.0, 0.5, 0.0], prior_max=[1.0, 0.7, 0.5], prior_kinds=["Exponential", "Laplace", "Cauchy"],
             lower_bound=[-0.5, -2.0, -3.0], upper_bound=[4.0, 3.0, 3.0]),
        [-0.5, -2.0, -3.0], [4.5, 5.0, 6.0]),
}


@pytest.mark.parametrize("priors", sorted(NON_UNIFORM))
def test_non_uniform_priors(priors):
    """non-Uniform priors inside finite bounds (:77-90, logPriorWeight :366-376)"""
    kw, lower, width = NON_UNIFORM[priors]
    dev, ref = pair("Ellipse", 50, 3, 4, **kw)
    assert ref.lower == lower and ref.width == width
    run_both(dev, ref)


def half_open_model(theta):
    """-0.5 |theta|^2 where theta_0 >= -2.5, -inf elsewhere (a quarter of the prior)"""
    theta = np.asarray(theta)
    out = []
    for x in theta:
        ss = 0.0
        for v in x:
            ss += float(v) * float(v)
        out.append(-0.5 * ss if x[0] >= -2.5 else -np.inf)
    return np.array(out)


def test_host_evaluations_with_minus_infinity():
    """live points and candidates at -inf: the isfinite branches of :330 and :348"""
    dev, ref = pair("Box", 32, 2, 3, model=half_open_model)
    dev.prepare(1)
    dev.set_evaluations(half_open_model(dev.candidates()))
    dev.process(1)
    ref.first_generation()
    compare(dev, ref, 1)
    assert np.isinf(ref["Live LogLikelihoods"]).sum() >= 2
    assert ref.s["LStar"] == nr.LOWEST  # (:248: the worst live point is not finite)
    try:
        for g in range(2, 2 + GENERATIONS):
            dev_generation(dev, g, half_open_model)
            ref.generation()
            compare(dev, ref, g)
        dev.synchronize()
    finally:
        dev.close()
    assert ref.s["Number Dead Samples"] < ref.s["Accepted Samples"]  # :330 skipped rows
    assert np.isfinite(ref.s["LStar"])


def test_a_generation_that_has_to_loop():
    """A teacher-forced live set that ties at a value few candidates reach: the
    generation repeats its draw until one does (:167-201), Last Accepted
    counts every round twice (:199, :362), and the generators end where the
    restatement's do."""
    dev, ref = pair("Box", 16, 2, 4)
    try:
        dev.first_generation()
        ref.first_generation()
        ref.live_ll[:] = -0.25
        ref._sort()
        assert ref.rank == list(range(16))  # the tie rule: lower live index first
        ref.s["LStar"] = float(ref._key(0))
        dev["Live LogLikelihoods"] = ref.live_ll
        dev["Live Samples Rank"] = ref.rank
        dev["LStar"] = ref.s["LStar"]
        compare(dev, ref, "forced")
        dev.generation(2)
        ref.generation()
        compare(dev, ref, 2)
        assert ref.s["Last Accepted"] > 2 and dev["Last Accepted"][0] == ref.s["Last Accepted"]
        dev.synchronize()
    finally:
        dev.close()


@pytest.mark.parametrize("method,L,N,B,window", [("Box", 100, 2, 7, 4), ("Ellipse", 64, 3, 5, 2)])
def test_a_draw_that_spans_several_windows(method, L, N, B, window):
    dev, ref = pair(method, L, N, B, window_tries=window)
    try:
        dev.first_generation()
        ref.first_generation()
        most = 0
        for g in range(2, 8):
            dev.generation(g)
            ref.generation()
            windows, tries, _ = dev.diagnostics()
            assert ref.last_blocks >= 2  # (the restatement starts every draw at `window` tries)
            assert tries == ref.last_tries
            most = max(most, windows)
            compare(dev, ref, g)
        # the device keeps a window it had to double, so its later draws may fit in one
        assert most >= 2
        dev.synchronize()
    finally:
        dev.close()


def test_finalize_matches_the_restatement():
    from korali_amd.native import nested_permutation
    for add in (True, False):
        dev, ref = pair("Ellipse", 64, 3, 2, add_live_points=add, shuffle_seed=77)
        try:
            dev.first_generation()
            ref.first_generation()
            for g in range(2, 2 + GENERATIONS):
                dev.generation(g)
                ref.generation()
            dev.finalize()
            ref.finalize(nested_permutation)
            compare(dev, ref, ("finalize", add), posterior=True)
            assert ref["Posterior Samples LogPrior Database"].size >= 1
        finally:
            dev.close()
