"""The stage timer the six population solvers share (kg::StageTimes,
korali_amd/csrc/kg_profile.hpp) through each solver's C-ABI: what two
generations record, that a read forgets, that a timer switched off records
nothing, and that timing changes no result.  The smallest shapes each solver
accepts; the stage names are the literals of the solvers' Stage / HostStage
sites.

A count is exact where the code passes the stage a fixed number of times per
generation, and a lower bound where it depends on stream windows, on retries
or on which eigensolver plan the handle chose."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AT_LEAST = "at least"


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)).view(np.uint64)


class Case:
    """One solver: make() -> a seeded device, step(dev, g) -> generation g,
    fields: what the solver's own GPU test compares, generators: the indices
    of its exported generator states, stages: every stage name of the solver
    with its count after two generations (an int, (AT_LEAST, n), or None for
    a count check() relates to others)."""
    rng = "rng_state"
    host_stages = ()

    def check(self, dev, counts):
        pass

    def state(self, dev):
        dev.synchronize()
        out = {name: bits(dev[name]) for name in self.fields}
        for which in self.generators:
            out["generator %d" % which] = getattr(dev, self.rng)(which)
        return out


class Cmaes(Case):
    # N = 4, lambda = 8, no bounds, the exact covariance mode, stage by stage
    # (sample, evaluate, update), so that the objective is a launch of its own
    rng = "get_rng"
    generators = (0, 1)
    host_stages = ("eigen_chase_host", "eigen_tridiag_host", "eigen_c_wait", "eigen_dsd_wait")
    stages = {
        "init": 1, "eigen": 2, "eigen_unpack": 2, "eigen_apply": 2, "eigen_chase_host": 2,
        # the tridiagonalisation on the host core (C published ahead, once more by the second update) ...
        "eigen_publish_c": None, "eigen_fetch_h": None, "eigen_c_wait": None, "eigen_tridiag_host": None,
        # ... or on the device
        "eigen_tridiag": None, "eigen_dsd_wait": None,
        "rng_polar": 2, "transform": 2, "rng_consume": 2, "objective": 2, "sort": 2, "mean_paths": 2,
        "covariance": 2, "sigma": 2, "rankmu_mfma": 0,
        # counts without a time: one launch of either kernel per update
        "adaptC_row": None, "adaptC_lane": None,
    }

    @property
    def fields(self):
        # the state tables tests/test_gpu_cmaes.py loads and compares, the
        # scalars its teacher-forced test adds, the population and its values
        from golden_util import CMAES_STATE_SCALARS, CMAES_STATE_VECTORS
        extra = ("Sample Population", "Value Vector", "Conjugate Evolution Path L2 Norm",
                 "Maximum Diagonal Covariance Matrix Element", "Minimum Diagonal Covariance Matrix Element",
                 "Current Min Standard Deviation", "Current Max Standard Deviation")
        return tuple(CMAES_STATE_VECTORS) + tuple(CMAES_STATE_SCALARS) + extra

    def make(self):
        from korali_amd.native import CmaesDevice
        return CmaesDevice(4, 8, initial_value=np.zeros(4), initial_std=np.ones(4), normal_seed=1337,
                           uniform_seed=1338, cov_mode="exact")

    def step(self, dev, g):
        if g == 1:
            dev.initialize()
        dev.sample()
        dev.evaluate("rosenbrock")
        dev.update(g)

    def check(self, dev, counts):
        host = [counts[s][1] for s in ("eigen_fetch_h", "eigen_c_wait", "eigen_tridiag_host")]
        device = [counts[s][1] for s in ("eigen_tridiag", "eigen_dsd_wait")]
        if counts["eigen_publish_c"][1]:
            assert counts["eigen_publish_c"][1] >= 2 and host == [2, 2, 2] and device == [0, 0]
        else:
            assert host == [0, 0, 0] and device == [2, 2]
        row, lane = counts["adaptC_row"], counts["adaptC_lane"]
        assert row[1] + lane[1] == 2 and row[0] == 0.0 and lane[0] == 0.0

    def state(self, dev):
        out = super().state(dev)
        out["Sorting Index"] = dev.sorting_index()
        return out


class Tmcmc(Case):
    rng = "get_rng"
    generators = (0, 1, 2, 3, 4, 5)
    fields = ("Chain Candidates", "Chain Candidates LogLikelihoods", "Chain Candidates LogPriors", "Chain Leaders",
              "Chain Leaders LogLikelihoods", "Chain Leaders LogPriors", "Chain Lengths", "Mean Theta",
              "Covariance Matrix", "Sample Database", "Sample LogLikelihood Database", "Num Selections",
              "Annealing Exponent", "Previous Annealing Exponent", "LogEvidence", "Coefficient Of Variation",
              "Max Loglikelihood", "Chain Count", "Accepted Samples Count", "Proposals Acceptance Rate",
              "Selection Acceptance Rate", "Model Evaluation Count", "Min Search Iterations")
    host_stages = ("min_search", "multinomial")
    stages = {
        "cholesky": 2, "prior_draw": 1, "rng_polar": (AT_LEAST, 1), "draw": (AT_LEAST, 1),
        "evaluate": (AT_LEAST, 2), "accept": (AT_LEAST, 2), "min_search": 2, "weights": 2, "multinomial": 2,
        "mean_cov": 2, "expand": 2, "hier_loglik": 0, "theta_denominators": 0,
    }

    def make(self):
        from korali_amd.native import TmcmcDevice
        return TmcmcDevice(3, 16, prior_min=[-5.0] * 3, prior_max=[5.0] * 3, prior_seeds=[1337, 1338, 1339],
                           multinomial_seed=1340, multivariate_seed=1341, uniform_seed=1342)

    def step(self, dev, g):
        dev.generation(g)


class Dea(Case):
    generators = (0, 1)
    stages = {"words": None, "propose": None, "evaluate": 2, "update": 2}

    @property
    def fields(self):
        import dea_ref
        return tuple(dea_ref.VECTORS + dea_ref.SCALARS)

    def make(self):
        from korali_amd.native import DeaDevice
        return DeaDevice(3, 8, [-1.0] * 3, [1.0] * 3, uniform_seed=1059, normal_seed=1058)

    def step(self, dev, g):
        dev.generation(g, "Rosenbrock")

    def check(self, dev, counts):
        # one of each per stream window; generation 1 draws without a window
        assert counts["words"][1] == counts["propose"][1] >= 2


class Mocmaes(Case):
    generators = (0, 1)
    stages = {"draw": 2, "evaluate": 2, "sort": 2, "update": 2, "parents": 2, "statistics": 2}

    @property
    def fields(self):
        import mocmaes_ref
        return tuple(mocmaes_ref.FIELDS + mocmaes_ref.SCALARS)

    def make(self):
        from korali_amd.native import MocmaesDevice
        return MocmaesDevice(3, 8, -1.0, 1.0, multinormal_seed=11, uniform_seed=12)

    def step(self, dev, g):
        dev.generation(g, "negative_rosenbrock_and_sphere")


class Nested(Case):
    generators = (0, 1)
    # generation 1 draws, evaluates and ranks the live set; every later attempt
    # (a generation repeats until a candidate is accepted) updates the bounds
    # when they are due, draws, evaluates and selects
    stages = {"bounds": (AT_LEAST, 1), "draw": (AT_LEAST, 2), "evaluate": None, "select": None}

    def __init__(self, method, L, N):
        self.method, self.L, self.N = method, L, N

    @property
    def fields(self):
        import nested_ref
        ref = nested_ref.NestedRef(self.N, self.L, -5.0, 5.0, batch_size=1, method=self.method, block_tries=0,
                                   likelihood="gaussian", proposal_update_frequency=10, uniform_seed=1011,
                                   normal_seed=2022)
        return tuple(ref.field_names(False))

    def make(self):
        from korali_amd.native import NestedDevice
        return NestedDevice(self.N, self.L, -5.0, 5.0, batch_size=1, method=self.method,
                            proposal_update_frequency=10, uniform_seed=1011, normal_seed=2022)

    def step(self, dev, g):
        dev.generation(g)

    def check(self, dev, counts):
        assert counts["draw"][1] == counts["evaluate"][1] == counts["select"][1]
        if self.method == "Box":  # (the Box method updates its bounds at every attempt)
            assert counts["bounds"][1] == counts["draw"][1] - 1


class Mcmc(Case):
    generators = (0, 1)
    stages = {"window": None, "chain": None, "consume": None}

    @property
    def fields(self):
        import mcmc_ref
        return tuple(mcmc_ref.FIELDS)

    def make(self):
        from korali_amd.native import McmcDevice
        return McmcDevice(3, [-0.1, -0.05, 0.0], [0.25, 0.3, 0.35], normal_seed=3001, uniform_seed=3002)

    def step(self, dev, g):
        assert dev.run(g, 1) == (1, [])

    def check(self, dev, counts):
        # one of each per launch; the two generations were two calls of one launch each
        assert dev.diagnostics()[0] == 1
        assert [counts[s][1] for s in ("window", "chain", "consume")] == [2, 2, 2]


CASES = {"cmaes": Cmaes(), "tmcmc": Tmcmc(), "dea": Dea(), "mocmaes": Mocmaes(), "nested-box": Nested("Box", 8, 2),
         "nested-ellipse": Nested("Ellipse", 16, 3), "mcmc": Mcmc()}


@pytest.fixture(params=sorted(CASES))
def case(request):
    return CASES[request.param]


def read_all(dev, case):
    return {s: dev.profile_read(s) for s in case.stages}


def test_two_generations_record_every_stage_they_pass_and_a_read_forgets(case):
    dev = case.make()
    try:
        dev.profile(True)
        for g in (1, 2):
            case.step(dev, g)
        dev.synchronize()
        counts = read_all(dev, case)
        for stage, want in case.stages.items():
            ms, n = counts[stage]
            assert math.isfinite(ms) and ms >= 0.0, (stage, ms)
            if isinstance(want, int):
                assert n == want, (stage, n)
            elif want is not None:
                assert n >= want[1], (stage, n)
            if n == 0:
                assert ms == 0.0, stage
        case.check(dev, counts)
        # (b) a stage read once is forgotten; a name nobody records reads as nothing
        for stage in case.stages:
            assert dev.profile_read(stage) == (0.0, 0), stage
        assert dev.profile_read("no such stage") == (0.0, 0)
        # (c) off means off
        dev.profile(False)
        case.step(dev, 3)
        dev.synchronize()
        for stage in case.stages:
            assert dev.profile_read(stage) == (0.0, 0), stage
    finally:
        dev.close()


def test_timing_changes_no_result(case):
    states = []
    for profiled in (True, False):
        dev = case.make()
        try:
            dev.profile(profiled)
            for g in (1, 2):
                case.step(dev, g)
            states.append(case.state(dev))
        finally:
            dev.close()
    timed, plain = states
    assert sorted(timed) == sorted(plain)
    for name in plain:
        if isinstance(plain[name], bytes):
            assert timed[name] == plain[name], name
        else:
            assert timed[name].shape == plain[name].shape and np.array_equal(timed[name], plain[name]), name


def test_cmaes_mark_a_second_begin_replaces_the_first():
    dev = CASES["cmaes"].make()
    try:
        assert dev.profile_mark("bracket", 0) == 0
        assert dev.profile_mark("bracket", 0) == 0
        assert dev.profile_mark("bracket", 1) == 0
        ms, n = dev.profile_read("bracket")
        assert n == 1 and math.isfinite(ms) and ms >= 0.0
        assert dev.profile_read("bracket") == (0.0, 0)
    finally:
        dev.close()


def test_cmaes_mark_an_end_without_a_begin_is_an_error():
    from korali_amd import native
    dev = CASES["cmaes"].make()
    try:
        with pytest.raises(native.KoraliDeviceError, match="not begun"):
            native.check(dev.profile_mark("bracket", 1))
        assert dev.profile_read("bracket") == (0.0, 0)  # (nothing was recorded)
        # ... and a pair after it is still one sample
        assert dev.profile_mark("bracket", 0) == 0 and dev.profile_mark("bracket", 1) == 0
        assert dev.profile_read("bracket")[1] == 1
    finally:
        dev.close()


def test_cmaes_mark_left_open_at_close():
    dev = CASES["cmaes"].make()
    assert dev.profile_mark("bracket", 0) == 0
    dev.close()  # (releases the open event)
    assert dev.h is None


def test_tmcmc_host_clock_stage():
    case = CASES["tmcmc"]
    dev = case.make()
    try:
        dev.profile(True)
        case.step(dev, 1)
        ms, n = dev.profile_read("min_search")
        assert n >= 1 and math.isfinite(ms) and ms >= 0.0
    finally:
        dev.close()
