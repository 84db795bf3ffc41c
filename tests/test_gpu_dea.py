"""Optimizer/DEA on the device (kg_dea_*, korali_amd/csrc/kg_dea.hip) against
the reference's recorded run (tests/golden/dea_golden.json.gz) and against the
NumPy restatement (tests/dea_ref.py, itself checked against the recording by
tests/test_dea_ref_golden.py).  Every comparison is exact."""
import numpy as np
import pytest

import dea_ref
from dea_ref import SCALARS, VECTORS

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def gens():
    return dea_ref.load_golden()


def golden_device(gens, **kw):
    from korali_amd.native import DeaDevice
    g1 = gens[1]
    sv, vs = g1["Solver"], g1["Variables"]
    return DeaDevice(len(vs), sv["Population Size"], [v["Lower Bound"] for v in vs], [v["Upper Bound"] for v in vs],
                     crossover_rate=sv["Crossover Rate"], mutation_rate=sv["Mutation Rate"],
                     mutation_rule=sv["Mutation Rule"], parent_rule=sv["Parent Selection Rule"],
                     accept_rule=sv["Accept Rule"], fix_infeasible=bool(sv["Fix Infeasible"]),
                     normal_seed=sv["Normal Generator"]["Random Seed"],
                     uniform_seed=sv["Uniform Generator"]["Random Seed"], **kw)


@pytest.fixture(scope="module")
def forced(gens):
    dev = golden_device(gens)
    yield dev
    dev.close()


def assert_fields(dev, want, what):
    """want: a mapping with the reference's field names (a recorded 'Solver' or a DeaRef)"""
    for k in VECTORS:
        a, b = dev[k], np.asarray(want[k], dtype=np.float64).reshape(-1)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {k}"
    for k in SCALARS:
        assert dev[k][0] == float(want[k]), f"{what}: {k}"


@pytest.mark.parametrize("k", range(1, 23))
def test_teacher_forced_against_the_recording(forced, gens, k):
    dev, cur, nxt = forced, gens[k]["Solver"], gens[k + 1]["Solver"]
    for f in VECTORS + SCALARS:
        dev[f] = cur[f]
    dev.set_rng_state(bytes.fromhex(cur["Uniform Generator"]["Range"]))
    dev.prepare(k + 1)
    assert np.array_equal(dev.candidates(), np.array(nxt["Candidate Population"]))
    assert dev["Infeasible Sample Count"][0] == nxt["Infeasible Sample Count"]
    assert dev.rng_state().hex().upper() == nxt["Uniform Generator"]["Range"]
    dev.set_fitness(nxt["Value Vector"])
    dev.update(k + 1)
    dev.synchronize()
    assert_fields(dev, nxt, f"generation {k + 1}")


@pytest.mark.parametrize("window", [0, 64])
def test_seeded_run_reproduces_all_recorded_generations(gens, window):
    """kg_dea_generation with the Rosenbrock kernel from the recorded seeds;
    with a 64-word window every generation past the first relaunches."""
    dev = golden_device(gens, window_words=window)
    assert dev.rng_state(0).hex().upper() == gens[1]["Solver"]["Normal Generator"]["Range"]
    assert dev.rng_state(1).hex().upper() == gens[0]["Solver"]["Uniform Generator"]["Range"]
    relaunched = 0
    for g in range(1, 24):
        dev.generation(g, "Rosenbrock")
        dev.synchronize()
        relaunched += dev.windows()[0] > 1
        assert_fields(dev, gens[g]["Solver"], f"generation {g}")
        assert dev.rng_state().hex().upper() == gens[g]["Solver"]["Uniform Generator"]["Range"], g
    assert dev.rng_state(0).hex().upper() == gens[1]["Solver"]["Normal Generator"]["Range"]
    assert relaunched == (22 if window else 0)
    dev.close()


def shifted_sphere(x):
    """An objective whose maximum lies at a corner region of the bounds, so
    mutants keep leaving them; plain Python doubles, evaluated on the host
    for the device and the restatement alike."""
    res = 0.0
    for d, v in enumerate(x):
        t = v - 0.9 + 0.01 * (d % 7)
        res += t * t
    return -res


# (P, N, settings, window words, at least this many infeasible attempts in generations 2..5: counted by the
# restatement on the CPU when the cases were chosen; 600 = three quarters of P per generation)
CASES = [
    # rejection loops retry with probability 1/4 to 3/4; a generation draws at least 4 (3 + 1 + 3) = 28 words,
    # so a 16-word window (the smallest) relaunches in every one
    (4, 3, dict(accept_rule="Best", parent_rule="Random", mutation_rule="Fixed", fix_infeasible=True), 16, 1),
    (4, 3, dict(accept_rule="Greedy", parent_rule="Best", mutation_rule="Self Adaptive", fix_infeasible=False,
                crossover_rate=0.3), 16, 1),
    # P not a power of two: the mean's division shows
    (24, 7, dict(accept_rule="Iterative", parent_rule="Best", mutation_rule="Self Adaptive", fix_infeasible=True),
     0, 24),
    (24, 7, dict(accept_rule="Improved", parent_rule="Random", mutation_rule="Fixed", fix_infeasible=False,
                 crossover_rate=0.2), 64, 24),
    # N past two wavefronts, not a multiple of 64; a 64-word window holds no attempt and has to grow
    (50, 130, dict(accept_rule="Improved", parent_rule="Random", mutation_rule="Fixed", fix_infeasible=False,
                   crossover_rate=0.02), 64, 50),
    (50, 130, dict(accept_rule="Iterative", parent_rule="Best", mutation_rule="Fixed", fix_infeasible=True), 0, 200),
    # tight bounds: most samples need several attempts
    (200, 33, dict(accept_rule="Greedy", parent_rule="Random", mutation_rule="Self Adaptive", fix_infeasible=True),
     0, 600),
    (200, 33, dict(accept_rule="Best", parent_rule="Random", mutation_rule="Fixed", fix_infeasible=True), 4096, 600),
]


@pytest.mark.parametrize("P,N,kw,window,min_infeasible", CASES)
def test_five_generations_against_the_restatement(P, N, kw, window, min_infeasible):
    from korali_amd.native import DeaDevice
    lb, ub = -1.0, 1.0
    seed = 1000 + 7 * P + N
    ref = dea_ref.DeaRef(N, P, lb, ub, uniform_seed=seed, **kw)
    dev = DeaDevice(N, P, [lb] * N, [ub] * N, uniform_seed=seed, normal_seed=seed - 1, window_words=window, **kw)
    dev.initialize()
    ref.initialize()
    relaunched = False
    for g in range(1, 6):
        dev.prepare(g)
        ref.prepare(g)
        X = dev.candidates()
        assert np.array_equal(X, ref.candidates()), g
        assert dev.rng_state() == ref.rng.export(), g
        relaunched |= dev.windows()[0] > 1
        F = [shifted_sphere(x) for x in X]
        dev.set_fitness(F)
        dev.update(g)
        ref.update(F)
        dev.synchronize()
        assert_fields(dev, ref, f"generation {g}")
    assert ref["Infeasible Sample Count"] >= min_infeasible
    if 0 < window <= 64:
        assert relaunched
        assert dev.windows()[1] >= max(window, N)
    dev.close()


@pytest.mark.timeout(120)
def test_impossible_configuration_is_an_error_not_a_hang():
    """Bounds of zero width, Fix Infeasible off, a tiny window cap.  With
    zero-width bounds alone every sample equals the bound and every mutant
    parent + F (a - b) = parent is feasible, so the population is placed
    outside the bounds: every candidate then equals 1 > 0 and no attempt can
    ever be feasible.  The reference would redraw forever; the device stops
    after max_windows windows.  A hang here is a bug in the bounded-window
    logic."""
    from korali_amd.native import DeaDevice, KoraliDeviceError
    dev = DeaDevice(3, 4, [0.0] * 3, [0.0] * 3, fix_infeasible=False, uniform_seed=5, window_words=64, max_windows=8)
    dev.initialize()
    assert np.array_equal(dev["Sample Population"], np.zeros(12))
    dev["Sample Population"] = np.ones(12)
    dev.prepare(1)
    with pytest.raises(KoraliDeviceError, match="no feasible candidate after 8 windows of 64"):
        dev.prepare(2)
    # the words of the failed attempts were consumed; the handle is still usable
    assert dev["Infeasible Sample Count"][0] > 0
    dev["Sample Population"] = np.zeros(12)
    dev.prepare(2)
    assert np.array_equal(dev.candidates(), np.zeros((4, 3)))
    dev.close()


def test_builtin_objective_past_128_variables():
    """kg_dea_generation at N = 130: the builtin kernels' N > 128 path, whole
    generations against the restatement with the example's Python objective."""
    from korali_amd.native import DeaDevice
    N, P = 130, 12
    ref = dea_ref.DeaRef(N, P, -2.0, 2.0, uniform_seed=77)
    dev = DeaDevice(N, P, [-2.0] * N, [2.0] * N, uniform_seed=77)
    for g in range(1, 4):
        dev.generation(g, "Rosenbrock")
        ref.generation(g, dea_ref.negative_rosenbrock)
        dev.synchronize()
        assert_fields(dev, ref, f"generation {g}")
        assert dev.rng_state() == ref.rng.export(), g
    dev.close()


def test_entry_points_check_their_arguments():
    from korali_amd.native import DeaDevice, KoraliDeviceError
    dev = DeaDevice(3, 8, [0.0] * 3, [1.0] * 3)
    with pytest.raises(KoraliDeviceError, match="holds no population"):
        dev.prepare(2)
    with pytest.raises(KoraliDeviceError, match="holds no population"):
        dev.update(1)
    dev.initialize()
    dev.prepare(1)
    X = np.empty((8, 3))
    assert dev._L.kg_dea_get_candidates(dev.h, X.ctypes.data_as(dev._L.kg_dea_get_candidates.argtypes[1]), 2) != 0
    assert b"ld is smaller" in dev._L.kg_last_error()
    assert dev._L.kg_dea_set_fitness(dev.h, None) != 0
    with pytest.raises(KoraliDeviceError, match="Non finite"):
        dev.set_fitness([0.0] * 7 + [float("nan")])
    dev.close()


def test_profile_reports_the_four_stages(gens):
    dev = golden_device(gens)
    dev.profile(True)
    for g in range(1, 4):
        dev.generation(g, "Rosenbrock")
    for stage, count in (("words", 3), ("propose", 3), ("evaluate", 3), ("update", 3)):
        ms, n = dev.profile_read(stage)
        assert n == count and ms > 0.0, stage
    dev.close()
