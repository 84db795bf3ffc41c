"""GPU: the Hierarchical/Theta likelihood (korali_amd/csrc/kg_hier.hip: the
denominator and the Theta modes of k_hier_group, k_hier_finish) against
tests/hier_theta_ref.py, bit for bit; the status word and the argument checks;
whole TMCMC runs with the device completing a host-fed or the builtin
sub-problem log-likelihood against runs fed hier_theta_ref's values; and
phases 1, 2 and 3b through korali.Engine."""
import json

import numpy as np
import pytest

import hier_ref as H
import hier_theta_ref as T
from test_gpu_hier import (SCA_KEYS, VEC_KEYS, parameter_rows, phase1, psi_run, resumed, same, same_final_files,
                           samples)

pytestmark = pytest.mark.gpu

TILE = 256  # kg_hier.hip TPB: rows per LDS tile
SIZES = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]

# per D: the Psi experiment's conditional priors (every kind in one of them)
SPECS = {
    1: dict(kinds=[H.LAPLACE], index=[[0, 1]], const=[[0.0, 0.0]], nvar=2),
    2: dict(kinds=[H.NORMAL, H.LOGNORMAL], index=[[0, 1], [2, 3]], const=[[0.0, 0.0]] * 2, nvar=4),
    3: dict(kinds=[H.UNIFORM, H.EXPONENTIAL, H.CAUCHY], index=[[0, 1], [-1, 2], [3, 4]],
            const=[[0.0, 0.0], [0.1, 0.0], [0.0, 0.0]], nvar=5),
}


def theta_device(spec, psi_db, sub_db, lps, P=2, **kw):
    from korali_amd.native import TmcmcDevice
    N = len(spec["kinds"])
    kw.setdefault("prior_min", [-10.0] * N)
    kw.setdefault("prior_max", [10.0] * N)
    dev = TmcmcDevice(N, P, **kw)
    dev.set_hierarchical_theta(spec["kinds"], spec["index"], spec["const"], psi_db, sub_db, lps)
    return dev


class Ref:
    """hier_theta_ref with the Psi rows' parameters and the denominators formed once."""

    def __init__(self, spec, psi_db, sub_db, lps):
        self.spec, self.psi_db = spec, psi_db
        self.par = H.theta_new_params(spec["kinds"], spec["index"], spec["const"], psi_db)
        self.den = T.theta_denominators(spec["kinds"], spec["index"], spec["const"], psi_db, sub_db, lps,
                                        params=self.par)

    def loglik(self, X, sub=None):
        s = self.spec
        return np.array([T.theta_loglik(x, None if sub is None else sub[i], s["kinds"], s["index"], s["const"],
                                        self.psi_db, params=self.par, den=self.den) for i, x in enumerate(X)])


@pytest.mark.parametrize("K", SIZES)
@pytest.mark.parametrize("M", SIZES)
def test_theta_kernels_match_reference(M, K):
    D = 1 + (SIZES.index(M) + SIZES.index(K)) % 3  # every D at several M and several K
    spec = SPECS[D]
    rng = np.random.default_rng(10000 * D + 100 * M + K)
    psi_db, sub_db, lps = parameter_rows(spec, M, rng), samples(spec, K, rng), rng.uniform(-8.0, -0.5, K)
    X, sub = samples(spec, 3, rng), rng.uniform(-9.0, -1.0, 3)
    dev, ref = theta_device(spec, psi_db, sub_db, lps), Ref(spec, psi_db, sub_db, lps)
    den = dev.theta_denominators()
    assert den.shape == (M,) and np.all(np.isfinite(den))
    assert same(den, np.array(ref.den))
    assert np.all(np.isfinite(dev.theta_loglik(X, sub)))
    for s in (sub, None, np.array([np.inf, -np.inf, sub[2]])):
        assert same(dev.theta_loglik(X, s), ref.loglik(X, s))


def test_minus_inf_denominator_lognormal_and_uniform_without_width():
    # Psi row 1's Uniform holds no sub-sample: den_1 = -inf; a point outside it
    # is a NaN term, a point inside it a +inf one (test_hier_theta_ref_cpu.py);
    # a point outside every row has -inf terms beside the NaN, which never wins
    # logSumExp's `>`: the maximum stays -inf and is returned
    spec = dict(kinds=[H.UNIFORM], index=[[0, 1]], const=[[0.0, 0.0]])
    psi_db = np.array([[-1.0, 1.0], [5.0, 6.0], [-2.0, 2.0]])
    sub_db, lps = np.array([[0.5], [-0.25], [0.75]]), np.array([-1.0, -1.5, -2.0])
    dev, ref = theta_device(spec, psi_db, sub_db, lps), Ref(spec, psi_db, sub_db, lps)
    assert ref.den[1] == -np.inf and same(dev.theta_denominators(), np.array(ref.den))
    X, sub = np.array([[0.1], [5.5], [9.0]]), np.array([-1.0, -1.0, -1.0])
    want = ref.loglik(X, sub)
    assert np.isnan(want[0]) and want[1] == np.inf and want[2] == -np.inf
    assert same(dev.theta_loglik(X, sub), want) and same(dev.theta_loglik(X), ref.loglik(X))

    # a Uniform without width at row 1: its constant is NaN, only x = Minimum is
    # inside; a sub-sample there makes den_1 NaN, none makes it -inf
    psi_db = np.array([[-1.0, 1.0], [0.5, 0.5], [-2.0, 2.0]])
    for sub_db in (np.array([[0.5], [-0.25], [0.75]]), np.array([[0.25], [-0.25], [0.75]])):
        dev, ref = theta_device(spec, psi_db, sub_db, lps), Ref(spec, psi_db, sub_db, lps)
        assert not np.isfinite(ref.den[1]) and same(dev.theta_denominators(), np.array(ref.den))
        X = np.array([[0.5], [0.1], [3.0]])
        assert same(dev.theta_loglik(X, sub), ref.loglik(X, sub))

    # a LogNormal prior at x <= 0: every term is -inf and so is LL, with any finite sub log-likelihood
    spec = SPECS[2]
    rng = np.random.default_rng(5)
    psi_db, sub_db, lps = parameter_rows(spec, 70, rng), samples(spec, 40, rng), rng.uniform(-3, -1, 40)
    dev, ref = theta_device(spec, psi_db, sub_db, lps), Ref(spec, psi_db, sub_db, lps)
    X = np.array([[0.3, -1.0], [0.3, 0.0], [0.3, 0.7]])
    want = ref.loglik(X, sub)
    assert want[0] == -np.inf and want[1] == -np.inf and np.isfinite(want[2])
    assert same(dev.theta_loglik(X, sub), want)
    # ... and NaN below a +inf one
    s = np.array([np.inf, 0.0, np.inf])
    want = ref.loglik(X, s)
    assert np.isnan(want[0]) and want[1] == -np.inf and want[2] == np.inf
    assert same(dev.theta_loglik(X, s), want)


def test_invalid_psi_row_is_refused_with_its_row():
    from korali_amd.native import KoraliDeviceError
    spec = SPECS[2]
    rng = np.random.default_rng(6)
    psi_db, sub_db, lps = parameter_rows(spec, 9, rng), samples(spec, 5, rng), rng.uniform(-3, -1, 5)
    psi_db[4, 3] = 0.0
    psi_db[7, 1] = -1.0
    with pytest.raises(KoraliDeviceError) as e:
        theta_device(spec, psi_db, sub_db, lps)
    msg = str(e.value)
    assert "Incorrect Sigma parameter of LogNormal distribution: 0.000000." in msg
    assert "Psi sample 4, conditional prior 1" in msg


def nan_device(P=8):
    """Every candidate of the prior [-2, 2] is outside Psi row 1, whose denominator is -inf: LL is NaN."""
    spec = dict(kinds=[H.UNIFORM], index=[[0, 1]], const=[[0.0, 0.0]])
    psi_db = np.array([[-3.0, 3.0], [5.0, 6.0]])
    sub_db, lps = np.array([[0.5], [-0.25]]), np.array([-1.0, -1.5])
    return theta_device(spec, psi_db, sub_db, lps, P=P, prior_min=[-2.0], prior_max=[2.0], prior_seeds=[1])


def test_nan_log_posterior_is_reported_with_its_chain():
    from korali_amd.native import KoraliDeviceError
    d = nan_device()
    d.prepare(1)
    d.evaluate()  # the builtin sub log-likelihood, completed on the device
    with pytest.raises(KoraliDeviceError, match="Sample 0 returned NaN logPosterior evaluation."):
        d.synchronize()
    # host-fed: chain 0's prior is -inf and it is not evaluated; chain 1 is the first NaN
    d = nan_device()
    d.prepare(1)
    C = d["Chain Candidates"]
    C[0] = 7.0
    d["Chain Candidates"] = C
    d.evaluate_prior()
    lp = d["Chain Candidates LogPriors"]
    assert lp[0] == -np.inf and np.all(np.isfinite(lp[1:]))
    d.set_evaluations(lp, np.where(np.isinf(lp), -np.inf, -1.0))
    with pytest.raises(KoraliDeviceError, match="Sample 1 returned NaN logPosterior evaluation."):
        d.synchronize()
    # the status is cleared with the report; theta_loglik returns NaN as it is
    assert np.isnan(d.theta_loglik(np.array([[0.1]]), [-1.0])[0])
    d.synchronize()


def test_argument_checks():
    from korali_amd.native import KoraliDeviceError, TmcmcDevice
    spec = SPECS[1]
    psi, sub, lp = np.array([[0.0, 1.0], [0.5, 2.0]]), np.ones((3, 1)), np.zeros(3)
    mk = lambda N=1, **kw: TmcmcDevice(N, 4, prior_min=[0.0] * N, prior_max=[1.0] * N, **kw)
    args = (spec["kinds"], spec["index"], spec["const"])
    with pytest.raises(KoraliDeviceError, match="param_index out of range"):
        mk().set_hierarchical_theta(spec["kinds"], [[0, 2]], spec["const"], psi, sub, lp)
    with pytest.raises(KoraliDeviceError, match="kind entries"):
        mk().set_hierarchical_theta([6], spec["index"], spec["const"], psi, sub, lp)
    with pytest.raises(KoraliDeviceError, match="as many variables as conditional priors"):
        mk(N=2).set_hierarchical_theta(*args, psi, sub, lp)
    with pytest.raises(KoraliDeviceError, match="empty Psi database"):
        mk().set_hierarchical_theta(*args, np.ones((0, 2)), sub, lp)
    with pytest.raises(KoraliDeviceError, match="empty sub-experiment database"):
        mk().set_hierarchical_theta(*args, psi, np.ones((0, 1)), np.zeros(0))
    with pytest.raises(ValueError, match="one log-prior per sub-experiment sample"):
        mk().set_hierarchical_theta(*args, psi, sub, lp[:2])
    with pytest.raises(KoraliDeviceError, match="mTMCMC"):
        mk(version="mTMCMC").set_hierarchical_theta(*args, psi, sub, lp)
    with pytest.raises(KoraliDeviceError, match="Incorrect Width parameter of Laplace"):
        mk().set_hierarchical_theta(*args, np.array([[0.0, 1.0], [0.0, 0.0]]), sub, lp)
    d = mk()
    with pytest.raises(KoraliDeviceError, match="no Hierarchical/Theta likelihood"):
        d.theta_loglik(np.zeros((1, 1)))
    with pytest.raises(KoraliDeviceError, match="no Hierarchical/Theta likelihood"):
        d.theta_denominators()
    d.set_hierarchical_theta(*args, psi, sub, lp)
    with pytest.raises(KoraliDeviceError, match="already has a hierarchical likelihood"):
        d.set_hierarchical_theta(*args, psi, sub, lp)
    with pytest.raises(KoraliDeviceError, match="already has a hierarchical likelihood"):
        d.set_hierarchical("thetanew", *args, [psi])
    with pytest.raises(KoraliDeviceError, match="takes kg_tmcmc_theta_loglik"):
        d.hierarchical_loglik(np.zeros((1, 1)))
    with pytest.raises(KoraliDeviceError, match="needs kg_tmcmc_evaluate_prior first"):
        d.prepare(1)
        d.set_evaluations(np.zeros(4), np.zeros(4))
    d = mk()
    d.prepare(1)
    with pytest.raises(KoraliDeviceError, match="before the first kg_tmcmc_prepare"):
        d.set_hierarchical_theta(*args, psi, sub, lp)


# ------------------------------------------------------------------ sampler
def sampler_inputs():
    spec = SPECS[2]
    rng = np.random.default_rng(31)
    psi_db, sub_db, lps = parameter_rows(spec, 40, rng), samples(spec, 65, rng), rng.uniform(-3, -1, 65)
    kw = dict(prior_min=[-2.0, 0.2], prior_max=[2.0, 3.0], prior_seeds=[11, 12], multinomial_seed=15,
              multivariate_seed=16, uniform_seed=17, max_chain_length=2, default_burn_in=1)
    return spec, psi_db, sub_db, lps, kw


def host_generation(d, g, loglik):
    """One generation through the host protocol; loglik(X, todo) -> the values set_evaluations is given."""
    d.prepare(g)
    while True:
        d.evaluate_prior()
        pend, X, lp = d.pending(), d.candidates(), d["Chain Candidates LogPriors"]
        todo = [i for i in np.nonzero(pend)[0] if not (np.isinf(lp[i]) and lp[i] < 0)]
        ll = np.full(d.P, -np.inf)
        ll[todo] = loglik(X, todo)
        d.set_evaluations(lp, ll)
        if d.advance(g) == 0:
            break
    d.process(g)
    d.synchronize()


def assert_same_state(a, b, g):
    for key in VEC_KEYS + SCA_KEYS:
        assert same(a[key], b[key]), (g, key)
    for which in range(3 + a.N):
        assert a.get_rng(which) == b.get_rng(which), (g, which)


def test_sampler_completes_host_fed_sub_loglikelihoods():
    """Two handles, same seeds.  A has the Theta layout and is given a Python
    sub log-likelihood; B has no layout and is given hier_theta_ref's LL(x) of
    the same sub values."""
    from korali_amd.native import TmcmcDevice
    spec, psi_db, sub_db, lps, kw = sampler_inputs()
    N, P = 2, 96
    a, b = theta_device(spec, psi_db, sub_db, lps, P=P, **kw), TmcmcDevice(N, P, **kw)
    ref = Ref(spec, psi_db, sub_db, lps)
    sub_ll = lambda X, todo: np.array([-0.5 * (X[i][0] * X[i][0] + X[i][1] * X[i][1]) for i in todo])
    for g in range(1, 30):
        host_generation(a, g, sub_ll)
        host_generation(b, g, lambda X, todo: ref.loglik(X[todo], sub_ll(X, todo)))
        assert_same_state(a, b, g)
        if b["Previous Annealing Exponent"][0] >= 1.0:
            break
    assert g > 2 and b["Previous Annealing Exponent"][0] >= 1.0


def test_sampler_completes_the_builtin_sub_loglikelihood():
    """The builtin Gaussian kernel under a Theta layout: kg_tmcmc_generation,
    the same handle step by step, and a host-fed Theta handle given the sub
    values a layout-free handle's evaluate() forms for the same candidates."""
    from korali_amd.native import TmcmcDevice
    spec, psi_db, sub_db, lps, kw = sampler_inputs()
    N, P = 2, 96
    whole, steps, fed = (theta_device(spec, psi_db, sub_db, lps, P=P, **kw) for _ in range(3))
    plain = TmcmcDevice(N, P, **kw)
    plain.prepare(1)  # every chain pending, for good: evaluate() forms all P builtin values

    def builtin(X, todo):
        plain["Chain Candidates"] = X
        plain.evaluate()
        plain.synchronize()
        return plain["Chain Candidates LogLikelihoods"][todo]

    for g in range(1, 30):
        whole.generation(g)
        whole.synchronize()
        steps.prepare(g)
        steps.evaluate()
        while steps.advance(g):
            steps.evaluate()
        steps.process(g)
        steps.synchronize()
        host_generation(fed, g, builtin)
        assert_same_state(whole, steps, g)
        assert_same_state(whole, fed, g)
        if whole["Previous Annealing Exponent"][0] >= 1.0:
            break
    assert g > 2 and whole["Previous Annealing Exponent"][0] >= 1.0


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def phases(tmp_path_factory):
    """Phase 1 three times (the builtin Gaussian kernel) and phase 2."""
    import korali
    path = tmp_path_factory.mktemp("phases")
    subs = [phase1(path / ("sub%d" % i), 100 + i, 0.5 * i) for i in range(3)]
    korali.Engine().run(psi_run(path / "psi", subs))
    return path


Y = [0.3, 0.9, 1.4]


def custom_model(s):
    x = s["Parameters"]
    s["logLikelihood"] = -(abs(x[0] - 0.5) + 0.25 * x[1] * x[1])


def custom_loglik(x):
    return -(abs(x[0] - 0.5) + 0.25 * x[1] * x[1])


def reference_entries(x):
    return {"Reference Evaluations": [x[0] + x[1] * t for t in (0.0, 1.0, 2.0)], "Standard Deviation": [0.8] * 3}


def reference_model(s):
    for k, v in reference_entries(s["Parameters"]).items():
        s[k] = v


def reference_loglik(x):
    from korali_amd import libkorali as L
    return L._reference_loglikelihood("Normal", Y, reference_entries([float(v) for v in x]))


def theta_run(phases, variant, path, conduit=None):
    import korali
    e, psi = korali.Experiment(), korali.Experiment()
    assert psi.loadState(str(phases / "psi" / "latest"))
    e["Problem"]["Type"] = "Hierarchical/Theta"
    if variant == "custom":
        # a Python 'Likelihood Model' in place of the phase-1 run's builtin kernel
        d = json.load(open(phases / "sub0" / "latest"))
        del d["Problem"]["Likelihood Kernel"]
        e["Problem"]["Sub Experiment"] = d
        e["Problem"]["Sub Experiment"]["Problem"]["Likelihood Model"] = custom_model
    else:
        # run-phase3b.py: the loaded sub-experiment with its model re-assigned
        sub = korali.Experiment()
        assert sub.loadState(str(phases / "sub0" / "latest"))
        sub["Problem"]["Type"] = "Bayesian/Reference"
        sub["Problem"]["Likelihood Model"] = "Normal"
        sub["Problem"]["Reference Data"] = Y
        sub["Problem"]["Computational Model"] = reference_model
        e["Problem"]["Sub Experiment"] = sub
    e["Problem"]["Psi Experiment"] = psi
    e["Solver"]["Type"] = "Sampler/TMCMC"
    e["Solver"]["Population Size"] = 128
    e["Random Seed"] = 0xFEED
    e["File Output"]["Path"] = str(path)
    e["Console Output"]["Verbosity"] = "Silent"
    k = korali.Engine()
    if conduit:
        k["Conduit"]["Type"] = "Concurrent"
        k["Conduit"]["Concurrent Jobs"] = 3
    k.run(e)


def refill(variant):
    def f(r):
        if variant == "custom":
            r["Problem"]["Sub Experiment"]["Problem"]["Likelihood Model"] = custom_model
        else:
            r["Problem"]["Sub Experiment"]["Problem"]["Computational Model"] = reference_model
    return f


@pytest.mark.parametrize("variant", ["custom", "reference"])
def test_engine_phase_3b(phases, tmp_path, variant):
    theta_run(phases, variant, tmp_path / "theta")
    jt = json.load(open(tmp_path / "theta" / "latest"))
    js, jp = json.load(open(phases / "sub0" / "latest")), json.load(open(phases / "psi" / "latest"))
    assert jt["Is Finished"] is True and jt["Current Generation"] > 2
    # the sub-experiment's variables and distributions, the latter seeded from
    # its saved counter; the solver's generators from the experiment's own seed
    strip = lambda ds: [{k: v for k, v in d.items() if k not in ("Random Seed", "Range")} for d in ds]
    assert jt["Variables"] == js["Variables"] and len(jt["Variables"]) == 2
    assert strip(jt["Distributions"]) == strip(js["Distributions"]) and len(jt["Distributions"]) == 2
    assert [d["Random Seed"] for d in jt["Distributions"]] == [js["Random Seed"], js["Random Seed"] + 1]
    assert [jt["Solver"][g]["Random Seed"] for g in ("Multinomial Generator", "Multivariate Generator",
                                                     "Uniform Generator")] == [0xFEED, 0xFEED + 1, 0xFEED + 2]
    # the log-likelihood database, bit for bit
    kinds, index, const = [H.NORMAL, H.NORMAL], [[0, 1], [2, 3]], [[0.0, 0.0]] * 2
    spec = dict(kinds=kinds, index=index, const=const)
    ref = Ref(spec, np.array(jp["Solver"]["Sample Database"]), np.array(js["Solver"]["Sample Database"]),
              np.array(js["Solver"]["Sample LogPrior Database"]))
    model = custom_loglik if variant == "custom" else reference_loglik
    db, ll = np.array(jt["Solver"]["Sample Database"]), np.array(jt["Solver"]["Sample LogLikelihood Database"])
    assert db.shape == (128, 2) and np.all(np.isfinite(ll))
    assert same(ll, ref.loglik(db, [model(x) for x in db]))
    # resume from the middle generation, and the Concurrent conduit
    resumed(tmp_path / "theta", tmp_path / "theta_b", refill(variant))
    same_final_files(tmp_path / "theta", tmp_path / "theta_b")
    theta_run(phases, variant, tmp_path / "theta_c", conduit="Concurrent")
    same_final_files(tmp_path / "theta", tmp_path / "theta_c")
