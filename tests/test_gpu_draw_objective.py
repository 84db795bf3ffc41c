"""GPU parity of the fused draw (k_transform_obj: x = m + sigma B (D o z) and
the built-in objective in one launch, behind kg_cmaes_sample_eval) against the
CPU oracle and against the library's own separate kernels.

Every check is bit-exact (np.array_equal).  The shapes are the smallest at
which the 16-row x 128-column tile can go wrong: one column pair, a last row
tile with 1 and with 15 rows, lambda < 16, N not a multiple of 2, 4 or 32, a
ragged last K chunk, N at the limit, the fused update tail behind the fused
draw (lambda > 256), and the configurations that must keep the separate
kernels (N = 129, a finite bound).
"""
import numpy as np
import pytest

import refcpu as R

pytestmark = pytest.mark.gpu

STATE = ("Current Mean", "Previous Mean", "Evolution Path", "Conjugate Evolution Path",
         "Conjugate Evolution Path L2 Norm", "Covariance Matrix", "Covariance Eigenvector Matrix", "Axis Lengths",
         "Sigma", "Best Ever Value", "Best Ever Variables", "Current Best Value")
COUNT = "Model Evaluation Count"


def oracle_and_device(Nv, lam, seed=1337, mirrored=False, lower=None):
    from korali_amd.native import CmaesDevice
    o = R.CMAES(Nv, lam, 0)
    o["Initial Value"] = np.zeros(Nv)
    o["Initial Standard Deviation"] = np.ones(Nv)
    kw = {}
    if mirrored:
        o.option("Mirrored Sampling", 1)
    if lower is not None:
        o["Lower Bound"] = np.full(Nv, lower)
        kw = dict(lower_bound=np.full(Nv, lower))
    R.lib().kr_rng_seed(o.rng(0).ptr, seed)
    R.lib().kr_rng_seed(o.rng(1).ptr, seed + 1)
    dev = CmaesDevice(Nv, lam, initial_value=np.zeros(Nv), initial_std=np.ones(Nv), normal_seed=seed,
                      uniform_seed=seed + 1, cov_mode="exact", mirrored=mirrored, **kw)
    return o, dev


def assert_same_state(o, dev, g):
    dev.synchronize()
    assert np.array_equal(dev["Sample Population"], o["Sample Population"]), g
    assert np.array_equal(dev["Value Vector"], o["Value Vector"]), g
    assert np.array_equal(dev.sorting_index(), o.sorting_index()), g
    for key in STATE:
        assert np.array_equal(dev[key], o[key]), (g, key)


def seeded_run(Nv, lam, gens, objective="rosenbrock", mirrored=False, lower=None):
    o, dev = oracle_and_device(Nv, lam, mirrored=mirrored, lower=lower)
    for g in range(1, gens + 1):
        o.generation(g, objective)
        dev.generation(g, objective)
        assert_same_state(o, dev, g)
    assert dev.get_rng(0) == o.rng(0).get_bytes()
    assert dev.get_rng(1) == o.rng(1).get_bytes()
    assert np.array_equal(dev[COUNT], o[COUNT])
    assert o[COUNT][0] == gens * lam
    dev.close()


@pytest.mark.parametrize("Nv,lam,gens", [(2, 8, 4), (3, 17, 4), (17, 33, 4), (33, 100, 4), (64, 48, 4), (127, 40, 3),
                                         (128, 48, 3), (128, 272, 3)])
def test_seeded_run_matches_oracle_bit_exact(Nv, lam, gens):
    """Every generation's draw and objective are the one fused launch."""
    seeded_run(Nv, lam, gens)


@pytest.mark.parametrize("objective", ["ackley", "sphere"])
@pytest.mark.parametrize("Nv,lam", [(17, 33), (128, 48)])
def test_other_builtin_objectives(Nv, lam, objective):
    seeded_run(Nv, lam, 3, objective=objective)


def test_mirrored_sampling():
    seeded_run(13, 30, 4, mirrored=True)


def test_wider_problem_keeps_the_separate_kernels():
    seeded_run(129, 32, 3)


def test_bounded_handle_keeps_the_redraw_path():
    o, dev = oracle_and_device(5, 20, lower=-2.0)
    for g in range(1, 4):
        o.generation(g, "rosenbrock")
        dev.generation(g, "rosenbrock")
        assert_same_state(o, dev, g)
        assert dev["Infeasible Sample Count"][0] == o["Infeasible Sample Count"][0], g
    assert o["Infeasible Sample Count"][0] > 0  # the bound rejected draws
    assert dev.get_rng(0) == o.rng(0).get_bytes()
    assert np.array_equal(dev[COUNT], o[COUNT])
    dev.close()


# ------------------------------------------------ against the library itself
def twins(Nv, lam, seed=77):
    from korali_amd.native import CmaesDevice
    kw = dict(initial_value=np.zeros(Nv), initial_std=np.ones(Nv), normal_seed=seed, uniform_seed=seed + 1,
              cov_mode="exact")
    return CmaesDevice(Nv, lam, **kw), CmaesDevice(Nv, lam, **kw)


def snapshot(dev):
    dev.synchronize()
    s = {k: np.array(dev[k], copy=True) for k in STATE + ("Sample Population", "Value Vector", COUNT)}
    s["index"] = np.array(dev.sorting_index(), copy=True)
    s["rng0"], s["rng1"] = dev.get_rng(0), dev.get_rng(1)
    return s


def assert_twins_equal(a, b, step):
    sa, sb = snapshot(a), snapshot(b)
    for k in sa:
        if isinstance(sa[k], np.ndarray):
            assert np.array_equal(sa[k], sb[k]), (step, k)
        else:
            assert sa[k] == sb[k], (step, k)


@pytest.mark.parametrize("switch", [None, "0"])
@pytest.mark.parametrize("begin", [False, True])
def test_sample_eval_equals_sample_then_evaluate(monkeypatch, switch, begin):
    """One twin is driven with sample_eval, the other with sample() +
    evaluate(); begin: the engine's order (begin_sample() after each update).
    Setting Sigma between two generations makes the next draw take its
    overflow guard from the state instead of the termination record."""
    if switch is None:
        monkeypatch.delenv("KORALI_AMD_FUSED_DRAW", raising=False)
    else:
        monkeypatch.setenv("KORALI_AMD_FUSED_DRAW", switch)
    obj = "rosenbrock"
    a, b = twins(5, 20)
    a.initialize()
    b.initialize()
    for g in range(1, 7):
        a.sample_eval(obj)
        b.sample()
        b.evaluate(obj)
        assert_twins_equal(a, b, (g, "draw"))
        a.update(g)
        b.update(g)
        if begin:
            a.begin_sample()
            b.begin_sample()
        assert_twins_equal(a, b, (g, "update"))
        if g == 3:
            s = [0.75 * float(a["Sigma"][0])]
            a["Sigma"] = s
            b["Sigma"] = s
    a.close()
    b.close()


def drive(dev, fused, obj, sigma_after, sigma, gens):
    """-> (generation reached, error text or None, snapshot or None)"""
    from korali_amd.native import KoraliDeviceError
    g = 0
    try:
        dev.initialize()
        for g in range(1, gens + 1):
            if fused:
                dev.sample_eval(obj)
            else:
                dev.sample()
                dev.evaluate(obj)
            dev.update(g)
            if g == sigma_after:
                dev["Sigma"] = [sigma]
        return g, None, snapshot(dev)
    except KoraliDeviceError as e:
        return g, str(e), None


def test_tripped_guard_takes_the_redraw_path_and_the_separate_objective():
    """Sigma = 1e299 after two generations: the overflow guard trips, from
    the state in generation 3 (after set_field) and from the termination
    record after it.  sample_eval then runs the redraw rounds followed by the
    separate objective kernel and must end where the twin driven by sample()
    + evaluate() ends, or with the same error text (at these magnitudes the
    update's next guard is not finite, which both report alike)."""
    a, b = twins(4, 16, seed=5)
    ra = drive(a, True, "ackley", 2, 1e299, 5)
    rb = drive(b, False, "ackley", 2, 1e299, 5)
    assert ra[0] == rb[0]
    assert ra[1] == rb[1]
    if ra[2] is not None:
        for k in ra[2]:
            if isinstance(ra[2][k], np.ndarray):  # (bytes: a NaN on both sides is equal, -0.0 and 0.0 are not)
                assert np.array_equal(np.frombuffer(ra[2][k].tobytes(), np.uint8),
                                      np.frombuffer(rb[2][k].tobytes(), np.uint8)), k
            else:
                assert ra[2][k] == rb[2][k], k
    a.close()
    b.close()
