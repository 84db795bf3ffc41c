"""GPU parity of the fused CMA-ES update tail (rank + select, mean + paths,
C's hand-off to the host, the deferred generator consume) against the CPU
oracle.

Every check is bit-exact (np.array_equal).  The fused launches serve the plain
exact update from the second update on (256 < lambda <= 16384, N <= 128 for the
mean + paths launch), so every run here has more than one generation; the
shapes are the smallest at which these kernels can go wrong: N not a multiple
of 4 or 16, odd lambda and odd mu, lambda just above the rank-sort threshold,
a last workgroup with fewer than 16 keys, N at the k_paths3 limit.

The exact covariance update runs on row chains (k_adaptC_row) below N = 256
and on lane chains (k_adaptC_lane) from there up; KORALI_AMD_ADAPTC_LANE_MIN,
read when the handle is created, moves the switch, and the profile counters
adaptC_row / adaptC_lane tell which kernel ran.
"""
import numpy as np
import pytest

import refcpu as R

pytestmark = pytest.mark.gpu

STATE = ("Current Mean", "Previous Mean", "Evolution Path", "Conjugate Evolution Path",
         "Conjugate Evolution Path L2 Norm", "Covariance Matrix", "Covariance Eigenvector Matrix", "Axis Lengths",
         "Sigma", "Best Ever Value", "Best Ever Variables", "Current Best Value")


def oracle_and_device(Nv, lam, seed=1337, mirrored=False, diagonal=False):
    from korali_amd.native import CmaesDevice
    o = R.CMAES(Nv, lam, 0)
    o["Initial Value"] = np.zeros(Nv)
    o["Initial Standard Deviation"] = np.ones(Nv)
    if mirrored:
        o.option("Mirrored Sampling", 1)
    if diagonal:
        o.option("Diagonal Covariance", 1)
    R.lib().kr_rng_seed(o.rng(0).ptr, seed)
    R.lib().kr_rng_seed(o.rng(1).ptr, seed + 1)
    dev = CmaesDevice(Nv, lam, initial_value=np.zeros(Nv), initial_std=np.ones(Nv), normal_seed=seed,
                      uniform_seed=seed + 1, cov_mode="exact", mirrored=mirrored, diagonal=diagonal)
    return o, dev


def assert_same_state(o, dev, g):
    dev.synchronize()
    assert np.array_equal(dev["Sample Population"], o["Sample Population"]), g
    assert np.array_equal(dev["Value Vector"], o["Value Vector"]), g
    assert np.array_equal(dev.sorting_index(), o.sorting_index()), g
    for key in STATE:
        assert np.array_equal(dev[key], o[key]), (g, key)


def seeded_run(Nv, lam, gens, objective="rosenbrock", mirrored=False, diagonal=False, adaptc=None):
    """adaptc ("row" / "lane"): additionally, that kernel served every
    generation's covariance update and the other one none."""
    o, dev = oracle_and_device(Nv, lam, mirrored=mirrored, diagonal=diagonal)
    if adaptc:
        dev.profile()
    for g in range(1, gens + 1):
        o.generation(g, objective)
        dev.generation(g, objective)
        assert_same_state(o, dev, g)
    assert dev.get_rng(0) == o.rng(0).get_bytes()
    assert dev.get_rng(1) == o.rng(1).get_bytes()
    if adaptc:
        ran = {k: dev.profile_read("adaptC_" + k)[1] for k in ("row", "lane")}
        assert ran == {"row": gens if adaptc == "row" else 0, "lane": gens if adaptc == "lane" else 0}, ran
    dev.close()


@pytest.mark.parametrize("Nv,lam,gens", [(3, 257, 4), (17, 300, 4), (33, 1000, 4), (128, 272, 4), (128, 4096, 2)])
def test_seeded_run_matches_oracle_bit_exact(Nv, lam, gens):
    """The eigenvectors of generation g + 1 prove that the C which reached
    the host tridiagonalisation is the C on the device."""
    seeded_run(Nv, lam, gens)


def test_mirrored_sampling_through_the_rank_scatter():
    seeded_run(13, 300, 4, mirrored=True)


def test_old_path_still_matches(monkeypatch):
    """The separate kernels (k_rank_sort, k_update_best, k_gather_selected,
    k_rankmu_prep, k_mean3, k_paths3, publish after sigma) stay reachable:
    both switches are read when the handle is created."""
    monkeypatch.setenv("KORALI_AMD_FUSED_SELECT", "0")
    monkeypatch.setenv("KORALI_AMD_EARLY_PUBLISH", "0")
    seeded_run(17, 300, 4, adaptc="row")


# k_adaptC_lane below its default range (16 x 16 tiles, 64-term chunks summed
# in groups of 8 with single terms after them; mu = lambda / 2)
LANE_SHAPES = [
    (5, 16, 6),     # mu = 8: one partial chunk, exactly one group of 8; the separate sort and selection kernels
    (3, 257, 3),    # mu = 128: two full chunks (no load after the last one); one tile, mostly inactive lanes
    (16, 272, 3),   # N fills one tile; mu = 136: two chunks and one group of 8, no singles
    (17, 300, 4),   # three tiles, the second row block holds one row; mu = 150: 2 chunks, 2 groups of 8, 6 singles
    (33, 1000, 3),  # six tiles; mu = 500: seven chunks and a tail of 52
]


@pytest.mark.parametrize("Nv,lam,gens", LANE_SHAPES)
def test_lane_chains_match_oracle_bit_exact(monkeypatch, Nv, lam, gens):
    monkeypatch.setenv("KORALI_AMD_ADAPTC_LANE_MIN", "0")
    seeded_run(Nv, lam, gens, adaptc="lane")


def test_lane_chains_with_separate_selection_kernels(monkeypatch):
    """The factors come from k_rankmu_prep, not from the fused selection."""
    monkeypatch.setenv("KORALI_AMD_ADAPTC_LANE_MIN", "0")
    monkeypatch.setenv("KORALI_AMD_FUSED_SELECT", "0")
    monkeypatch.setenv("KORALI_AMD_EARLY_PUBLISH", "0")
    seeded_run(17, 300, 4, adaptc="lane")


def test_lane_chains_diagonal_covariance(monkeypatch):
    monkeypatch.setenv("KORALI_AMD_ADAPTC_LANE_MIN", "0")
    seeded_run(17, 300, 3, diagonal=True, adaptc="lane")


def test_select_prep_path_still_matches(monkeypatch):
    """KORALI_AMD_EARLY_PUBLISH=0 alone: k_rank_sort followed by
    k_select_prep at lambda > 256, the consume not deferred."""
    monkeypatch.setenv("KORALI_AMD_EARLY_PUBLISH", "0")
    seeded_run(17, 300, 4)


def forced(F):
    """ties (a run of 40 equal keys, one far pair) and signed zeros"""
    F = np.array(F, copy=True)
    F[40:80] = F[7]
    F[200] = F[3]
    F[5] = -0.0
    F[6] = 0.0
    return F


def test_ties_and_signed_zeros_teacher_forced():
    """Descending F, ties by index, -0.0 == +0.0; also the staged API
    (sample / evaluate / set_fitness / update) ends where generation() does."""
    Nv, lam, obj = 17, 300, "rosenbrock"
    o, dev = oracle_and_device(Nv, lam)
    o.initialize()
    dev.initialize()
    for g in range(1, 4):
        o.prepare()
        o.evaluate(obj)
        F = forced(o["Value Vector"])
        o["Value Vector"] = F
        o.update(g)
        # the oracle ranks the forced vector descending, ties by index
        assert np.array_equal(o.sorting_index(), np.lexsort((np.arange(lam), -F))), g
        dev.sample()
        dev.evaluate(obj)
        dev.set_fitness(F)
        dev.update(g)
        assert_same_state(o, dev, g)
    assert dev.get_rng(0) == o.rng(0).get_bytes()
    dev.close()


def test_generator_state_between_stages():
    """The consume of a draw's normals is deferred past C's hand-off, but the
    state seen through the API never lags; a set_rng between sample and update
    is neither lost nor overwritten by a late consume."""
    Nv, lam, obj = 17, 300, "rosenbrock"
    o, dev = oracle_and_device(Nv, lam)
    o.initialize()
    dev.initialize()
    other = R.Rng(seed=4242).get_bytes()
    for g in range(1, 5):
        o.prepare()
        dev.sample()
        if g != 3:
            assert dev.get_rng(0) == o.rng(0).get_bytes(), g  # after sample() alone
        else:
            o.rng(0).set_bytes(other)
            dev.set_rng(0, other)
        o.evaluate(obj)
        dev.evaluate(obj)
        o.update(g)
        dev.update(g)
        assert dev.get_rng(0) == o.rng(0).get_bytes(), g
        if g == 3:
            assert dev.get_rng(0) == other
        assert_same_state(o, dev, g)
    dev.close()


@pytest.mark.parametrize("first", [1, 2])
def test_set_field_after_update_invalidates_the_handoff(first):
    """The hand-off of C issued at the end of an update (the first update
    takes the separate kernels, the second the fused launches) saw the old
    matrix: after set_field the next generation decomposes the new one."""
    Nv, lam, obj = 17, 300, "rosenbrock"
    o, dev = oracle_and_device(Nv, lam)
    for g in range(1, first + 1):
        o.generation(g, obj)
        dev.generation(g, obj)
    dev.synchronize()
    A = np.random.default_rng(5).standard_normal((Nv, Nv))
    M = A @ A.T / Nv + np.diag(np.linspace(0.5, 2.0, Nv))
    M = 0.5 * (M + M.T)
    assert not np.array_equal(M.reshape(-1), o["Covariance Matrix"])
    o["Covariance Matrix"] = M
    dev["Covariance Matrix"] = M
    o.generation(first + 1, obj)
    dev.generation(first + 1, obj)
    assert_same_state(o, dev, first + 1)
    dev.close()
