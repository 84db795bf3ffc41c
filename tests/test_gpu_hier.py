"""GPU: the Hierarchical/Psi and Hierarchical/ThetaNew likelihood kernels
(korali_amd/csrc/kg_hier.hip) against tests/hier_ref.py, bit for bit, the
invalid-parameter / NaN status word, and a whole TMCMC run on the device
against the same run fed from the host with hier_ref's values."""
import os

import numpy as np
import pytest

import hier_ref as H

pytestmark = pytest.mark.gpu

TILE = 256  # kg_hier.hip TPB: rows per LDS tile

GROUP_SIZES = [(1, 2), (63, 64, 65), (257, 1, 130), (TILE - 1, TILE, TILE + 1)]

# per D: kinds, D x 2 parameter suppliers (-1: constant), constants, variables of a Psi point
SPECS = {
    1: dict(kinds=[H.NORMAL], index=[[0, 1]], const=[[0.0, 0.0]], nvar=2),
    3: dict(kinds=[H.LOGNORMAL, H.EXPONENTIAL, H.CAUCHY], index=[[0, -1], [-1, 1], [2, 3]],
            const=[[0.0, 0.8], [0.1, 0.0], [0.0, 0.0]], nvar=4),
    6: dict(kinds=[H.UNIFORM, H.NORMAL, H.EXPONENTIAL, H.LAPLACE, H.CAUCHY, H.LOGNORMAL],
            index=[[0, 1], [2, 3], [-1, 4], [5, -1], [6, 7], [8, 9]],
            const=[[0.0, 0.0], [0.0, 0.0], [-0.5, 0.0], [0.0, 1.3], [0.0, 0.0], [0.0, 0.0]], nvar=10),
}


def parameter_rows(spec, n, rng):
    """n rows of `nvar` values that are valid parameters where spec uses them
    (second parameters positive; a Uniform's Maximum above its Minimum)."""
    X = rng.normal(0.0, 0.7, (n, spec["nvar"]))
    for k, kind in enumerate(spec["kinds"]):
        ia, ib = spec["index"][k]
        if ib >= 0:
            X[:, ib] = rng.uniform(0.4, 2.5, n)
        if kind == H.UNIFORM and ia >= 0 and ib >= 0:
            X[:, ia] = rng.uniform(-6.0, -4.0, n)
            X[:, ib] = rng.uniform(4.0, 6.0, n)
    return X


def samples(spec, n, rng):
    """n values per conditional prior, inside every support"""
    cols = []
    for kind in spec["kinds"]:
        if kind == H.LOGNORMAL:
            cols.append(np.exp(rng.normal(0.0, 0.5, n)))
        elif kind == H.EXPONENTIAL:
            cols.append(rng.uniform(0.2, 3.0, n))
        else:
            cols.append(rng.normal(0.0, 1.0, n))
    return np.stack(cols, axis=1)


def psi_device(spec, groups, lps, P=2):
    from korali_amd.native import TmcmcDevice
    N = spec["nvar"]
    dev = TmcmcDevice(N, P, prior_min=[-10.0] * N, prior_max=[10.0] * N)
    dev.set_hierarchical("psi", spec["kinds"], spec["index"], spec["const"], groups, lps)
    return dev


def theta_device(spec, db, P=2):
    from korali_amd.native import TmcmcDevice
    N = len(spec["kinds"])
    dev = TmcmcDevice(N, P, prior_min=[-10.0] * N, prior_max=[10.0] * N)
    dev.set_hierarchical("thetanew", spec["kinds"], spec["index"], spec["const"], [db])
    return dev


def psi_ref(spec, X, groups, lps):
    return np.array([H.psi_loglik(x, spec["kinds"], spec["index"], spec["const"], groups, lps) for x in X])


def theta_ref(spec, X, db):
    par = H.theta_new_params(spec["kinds"], spec["index"], spec["const"], db)
    return np.array([H.theta_new_loglik(x, spec["kinds"], spec["index"], spec["const"], db, params=par) for x in X])


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("rows", [1, 70])
@pytest.mark.parametrize("sizes", GROUP_SIZES)
@pytest.mark.parametrize("D", [1, 3, 6])
def test_psi_kernel_matches_reference(D, sizes, rows):
    spec = SPECS[D]
    rng = np.random.default_rng(1000 * D + sum(sizes) + rows)
    groups = [samples(spec, K, rng) for K in sizes]
    lps = [rng.uniform(-8.0, -0.5, K) for K in sizes]
    X = parameter_rows(spec, rows, rng)
    dev = psi_device(spec, groups, lps)
    got = dev.hierarchical_loglik(X)
    assert np.all(np.isfinite(got))
    assert same(got, psi_ref(spec, X, groups, lps))


@pytest.mark.parametrize("rows", [1, 70])
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 130, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
@pytest.mark.parametrize("D", [1, 3, 6])
def test_theta_new_kernel_matches_reference(D, M, rows):
    spec = SPECS[D]
    rng = np.random.default_rng(77 * D + M + rows)
    db = parameter_rows(spec, M, rng)
    X = samples(spec, rows, rng)
    dev = theta_device(spec, db)
    got = dev.hierarchical_loglik(X)
    assert np.all(np.isfinite(got))
    assert same(got, theta_ref(spec, X, db))


def test_psi_infinite_terms_groups_and_bases():
    spec = SPECS[6]
    rng = np.random.default_rng(5)
    sizes = (70, 9, TILE + 3)
    X = parameter_rows(spec, 20, rng)

    def data():
        return [samples(spec, K, rng) for K in sizes], [rng.uniform(-8.0, -0.5, K) for K in sizes]

    # single -inf terms: LogNormal x <= 0, Exponential below its location (-0.5)
    groups, lps = data()
    groups[0][3, 5] = 0.0
    groups[0][64, 5] = -2.0
    groups[2][TILE, 2] = -0.75
    groups[2][0, 2] = -3.0
    ref = psi_ref(spec, X, groups, lps)
    assert np.all(np.isfinite(ref))
    assert same(psi_device(spec, groups, lps).hierarchical_loglik(X), ref)
    # a whole group of -inf
    groups[1][:, 5] = -1.0
    ref = psi_ref(spec, X, groups, lps)
    assert np.all(ref == -np.inf)
    assert same(psi_device(spec, groups, lps).hierarchical_loglik(X), ref)
    # one +inf base (a -inf log-prior in the database): +inf; with a -inf term in the same row: NaN
    groups, lps = data()
    lps[2][TILE + 1] = -np.inf
    ref = psi_ref(spec, X, groups, lps)
    assert np.all(ref == np.inf)
    assert same(psi_device(spec, groups, lps).hierarchical_loglik(X), ref)
    groups[2][TILE + 1, 5] = -1.0
    ref = psi_ref(spec, X, groups, lps)
    assert np.all(np.isnan(ref))
    assert same(psi_device(spec, groups, lps).hierarchical_loglik(X), ref)


def test_uniform_without_width():
    """Maximum <= Minimum: the constant is NaN (uniform.cpp.base:38-44)"""
    spec = dict(kinds=[H.UNIFORM, H.NORMAL], index=[[0, 1], [2, 3]], const=[[0.0, 0.0]] * 2, nvar=4)
    rng = np.random.default_rng(9)
    db = parameter_rows(spec, 67, rng)
    X = samples(spec, 12, rng)
    db[5, 0] = db[5, 1] = X[4, 0]   # point 4 sits on a zero-width interval: a NaN term below the max
    db[66, 0], db[66, 1] = 3.0, -3.0  # Maximum < Minimum: nothing is inside
    ref = theta_ref(spec, X, db)
    assert np.isnan(ref[4]) and np.isfinite(np.delete(ref, 4)).all()
    assert same(theta_device(spec, db).hierarchical_loglik(X), ref)
    # Psi: the evaluated point supplies the interval
    groups = [samples(spec, 5, rng), samples(spec, 66, rng)]
    lps = [rng.uniform(-3, -1, 5), rng.uniform(-3, -1, 66)]
    P = parameter_rows(spec, 6, rng)
    P[2, 0], P[2, 1] = 1.0, 1.0
    groups[1][65, 0] = 1.0
    P[3, 0], P[3, 1] = 2.0, -2.0
    ref = psi_ref(spec, P, groups, lps)
    assert ref[2] == -np.inf and ref[3] == -np.inf
    assert same(psi_device(spec, groups, lps).hierarchical_loglik(P), ref)


def test_invalid_parameter_is_reported_with_its_chain():
    from korali_amd.native import KoraliDeviceError
    spec = SPECS[1]
    rng = np.random.default_rng(3)
    groups = [samples(spec, 40, rng), samples(spec, 65, rng)]
    lps = [rng.uniform(-3, -1, 40), rng.uniform(-3, -1, 65)]
    X = parameter_rows(spec, 8, rng)
    X[5, 1] = 0.0
    X[7, 1] = -1.0
    dev = psi_device(spec, groups, lps)
    with pytest.raises(KoraliDeviceError) as e:
        dev.hierarchical_loglik(X)
    msg = str(e.value)
    assert "Incorrect Standard Deviation parameter of Normal distribution: 0.000000." in msg and "chain 5" in msg
    # the status is cleared with the report
    X[5, 1] = X[7, 1] = 1.0
    assert same(dev.hierarchical_loglik(X), psi_ref(spec, X, groups, lps))

    # a TMCMC chain: Standard Deviation 0 inside the prior is reported by the
    # next call that waits; outside it (log-prior -inf) the chain is not evaluated
    for lo, reported in ((-1.0, True), (0.5, False)):
        from korali_amd.native import TmcmcDevice
        d = TmcmcDevice(2, 16, prior_min=[-2.0, lo], prior_max=[2.0, 3.0], prior_seeds=[1, 2])
        d.set_hierarchical("psi", spec["kinds"], spec["index"], spec["const"], groups, lps)
        d.prepare(1)
        C = d["Chain Candidates"].reshape(16, 2)
        C[:, 1] = np.maximum(C[:, 1], 0.6)
        C[3, 1] = 0.0
        d["Chain Candidates"] = C
        d.evaluate()
        if reported:
            with pytest.raises(KoraliDeviceError) as e:
                d.synchronize()
            assert "Incorrect Standard Deviation parameter of Normal distribution: 0.000000." in str(e.value)
            assert "chain 3" in str(e.value)
        else:
            d.synchronize()
            ll = d["Chain Candidates LogLikelihoods"]
            assert ll[3] == -np.inf and np.isfinite(np.delete(ll, 3)).all()


def test_nan_log_posterior_is_reported():
    from korali_amd.native import KoraliDeviceError, TmcmcDevice
    spec = SPECS[1]
    rng = np.random.default_rng(4)
    groups = [samples(spec, 3, rng), samples(spec, 70, rng)]
    lps = [rng.uniform(-3, -1, 3), rng.uniform(-3, -1, 70)]
    lps[1][69] = -np.inf  # +inf base ...
    groups[1][69, 0] = np.inf  # ... plus a -inf density: NaN
    d = TmcmcDevice(2, 8, prior_min=[-2.0, 0.5], prior_max=[2.0, 3.0], prior_seeds=[1, 2])
    d.set_hierarchical("psi", spec["kinds"], spec["index"], spec["const"], groups, lps)
    d.prepare(1)
    d.evaluate()
    with pytest.raises(KoraliDeviceError) as e:
        d.synchronize()
    assert "Sample 0 returned NaN logPosterior evaluation." in str(e.value)


def test_argument_checks():
    from korali_amd.native import KoraliDeviceError, TmcmcDevice
    spec = SPECS[1]
    g = [np.ones((3, 1)), np.ones((2, 1))]
    lp = [np.zeros(3), np.zeros(2)]
    mk = lambda N=2, **kw: TmcmcDevice(N, 4, prior_min=[0.0] * N, prior_max=[1.0] * N, **kw)
    with pytest.raises(KoraliDeviceError, match="param_index out of range"):
        mk().set_hierarchical("psi", spec["kinds"], [[0, 2]], spec["const"], g, lp)
    with pytest.raises(KoraliDeviceError, match="kind entries"):
        mk().set_hierarchical("psi", [6], spec["index"], spec["const"], g, lp)
    with pytest.raises(KoraliDeviceError, match="group size of 0"):
        mk().set_hierarchical("psi", spec["kinds"], spec["index"], spec["const"], [g[0], np.ones((0, 1))],
                              [lp[0], np.zeros(0)])
    with pytest.raises(KoraliDeviceError, match="as many variables as conditional priors"):
        mk().set_hierarchical("thetanew", spec["kinds"], spec["index"], spec["const"], [np.ones((3, 2))])
    with pytest.raises(KoraliDeviceError, match="log-priors"):
        mk().set_hierarchical("psi", spec["kinds"], spec["index"], spec["const"], g)
    with pytest.raises(KoraliDeviceError, match="mTMCMC"):
        mk(version="mTMCMC").set_hierarchical("psi", spec["kinds"], spec["index"], spec["const"], g, lp)
    with pytest.raises(KoraliDeviceError, match="Incorrect Standard Deviation"):
        mk(N=1).set_hierarchical("thetanew", spec["kinds"], spec["index"], spec["const"],
                                 [np.array([[0.0, 1.0], [0.0, 0.0]])])
    d = mk()
    with pytest.raises(KoraliDeviceError, match="no hierarchical likelihood"):
        d.hierarchical_loglik(np.zeros((1, 2)))
    d.prepare(1)
    with pytest.raises(KoraliDeviceError, match="before the first kg_tmcmc_prepare"):
        d.set_hierarchical("psi", spec["kinds"], spec["index"], spec["const"], g, lp)


VEC_KEYS = ("Chain Leaders", "Chain Leaders LogLikelihoods", "Chain Leaders LogPriors", "Chain Candidates",
            "Chain Candidates LogLikelihoods", "Chain Candidates LogPriors", "Chain Lengths", "Mean Theta",
            "Covariance Matrix", "Cholesky Factor", "Sample Database", "Sample LogLikelihood Database",
            "Sample LogPrior Database", "Num Selections")
SCA_KEYS = ("Annealing Exponent", "Previous Annealing Exponent", "LogEvidence", "Coefficient Of Variation",
            "Max Loglikelihood", "Chain Count", "Accepted Samples Count", "Proposals Acceptance Rate",
            "Selection Acceptance Rate", "Database Entries", "Model Evaluation Count", "Current Burn In")


@pytest.mark.parametrize("shards", [0, 1])
def test_sampler_on_device_matches_host_fed_run(shards):
    """Two handles, same seeds: one evaluates the Psi likelihood on the
    device (kg_tmcmc_generation on odd generations, the step-wise calls on even
    ones), the other is fed hier_ref's values through the host protocol."""
    from korali_amd.native import TmcmcDevice
    N, P = 4, 96
    spec = dict(kinds=[H.NORMAL, H.LOGNORMAL], index=[[0, 1], [2, 3]], const=[[0.0, 0.0]] * 2, nvar=4)
    rng = np.random.default_rng(21)
    groups = [samples(spec, 40, rng), samples(spec, 65, rng)]
    lps = [rng.uniform(-3, -1, 40), rng.uniform(-3, -1, 65)]
    kw = dict(prior_min=[-2.0, 0.2, -1.0, 0.2], prior_max=[2.0, 3.0, 1.0, 2.0], prior_seeds=[11, 12, 13, 14],
              multinomial_seed=15, multivariate_seed=16, uniform_seed=17, max_chain_length=2, default_burn_in=1,
              shard_count=shards)
    dev, host = TmcmcDevice(N, P, **kw), TmcmcDevice(N, P, **kw)
    dev.set_hierarchical("psi", spec["kinds"], spec["index"], spec["const"], groups, lps)

    def finish(d, g):
        if shards:
            d.process_partial(g)
            d.process_finalize(g)
        else:
            d.process(g)

    for g in range(1, 13):
        if g % 2 and not shards:
            dev.generation(g)
        else:
            dev.prepare(g)
            dev.evaluate()
            if g % 2 == 0:
                while dev.advance(g):
                    dev.evaluate()
            finish(dev, g)
        host.prepare(g)
        while True:
            host.evaluate_prior()
            pend = host.pending()
            X = host.candidates()
            lp = host["Chain Candidates LogPriors"]
            ll = np.full(P, -np.inf)
            for i in np.nonzero(pend)[0]:
                if not (np.isinf(lp[i]) and lp[i] < 0):
                    ll[i] = H.psi_loglik(X[i], spec["kinds"], spec["index"], spec["const"], groups, lps)
            host.set_evaluations(lp, ll)
            if host.advance(g) == 0:
                break
        finish(host, g)
        dev.synchronize()
        host.synchronize()
        for key in VEC_KEYS:
            assert same(dev[key], host[key]), (g, key)
        for key in SCA_KEYS:
            assert same(dev[key], host[key]), (g, key)
        for which in range(3 + N):
            assert dev.get_rng(which) == host.get_rng(which), (g, which)
        if host["Previous Annealing Exponent"][0] >= 1.0:
            break
    assert g > 2


# ------------------------------------------------------------------ engine
def phase1(path, seed, shift):
    import korali
    e = korali.Experiment()
    e["Random Seed"] = seed
    e["Problem"]["Type"] = "Bayesian/Custom"
    e["Problem"]["Likelihood Kernel"] = "Gaussian"
    for d in range(2):
        e["Distributions"][d]["Name"] = "Uniform %d" % d
        e["Distributions"][d]["Type"] = "Univariate/Uniform"
        e["Distributions"][d]["Minimum"] = -4.0 + shift
        e["Distributions"][d]["Maximum"] = 5.0 + shift
        e["Variables"][d]["Name"] = "X%d" % d
        e["Variables"][d]["Prior Distribution"] = "Uniform %d" % d
    e["Solver"]["Type"] = "Sampler/TMCMC"
    e["Solver"]["Population Size"] = 128
    e["File Output"]["Path"] = str(path)
    e["Console Output"]["Verbosity"] = "Silent"
    korali.Engine().run(e)
    r = korali.Experiment()
    assert r.loadState(str(path / "latest"))
    return r


def psi_run(path, subs):
    import korali
    e = korali.Experiment()
    e["Random Seed"] = 0xC0FFEE
    e["Problem"]["Type"] = "Hierarchical/Psi"
    for i, s in enumerate(subs):
        e["Problem"]["Sub Experiments"][i] = s
    e["Problem"]["Conditional Priors"] = ["Conditional 0", "Conditional 1"]
    bounds = [(-3.0, 3.0), (0.2, 4.0), (-3.0, 3.0), (0.2, 4.0)]
    for i, (lo, hi) in enumerate(bounds):
        e["Variables"][i]["Name"] = "Psi %d" % i
        e["Variables"][i]["Prior Distribution"] = "Uniform %d" % i
        e["Distributions"][i]["Name"] = "Uniform %d" % i
        e["Distributions"][i]["Type"] = "Univariate/Uniform"
        e["Distributions"][i]["Minimum"] = lo
        e["Distributions"][i]["Maximum"] = hi
    for c in range(2):
        e["Distributions"][4 + c]["Name"] = "Conditional %d" % c
        e["Distributions"][4 + c]["Type"] = "Univariate/Normal"
        e["Distributions"][4 + c]["Mean"] = "Psi %d" % (2 * c)
        e["Distributions"][4 + c]["Standard Deviation"] = "Psi %d" % (2 * c + 1)
    e["Solver"]["Type"] = "Sampler/TMCMC"
    e["Solver"]["Population Size"] = 128
    e["File Output"]["Path"] = str(path)
    e["Console Output"]["Verbosity"] = "Silent"
    return e


def theta_new_run(path, psi):
    import korali
    e = korali.Experiment()
    e["Random Seed"] = 0xBEEF
    e["Problem"]["Type"] = "Hierarchical/ThetaNew"
    e["Problem"]["Psi Experiment"] = psi
    for i in range(2):
        e["Variables"][i]["Name"] = "Theta %d" % i
        e["Variables"][i]["Prior Distribution"] = "Uniform %d" % i
        e["Distributions"][i]["Name"] = "Uniform %d" % i
        e["Distributions"][i]["Type"] = "Univariate/Uniform"
        e["Distributions"][i]["Minimum"] = -6.0
        e["Distributions"][i]["Maximum"] = 6.0
    e["Solver"]["Type"] = "Sampler/TMCMC"
    e["Solver"]["Population Size"] = 128
    e["File Output"]["Path"] = str(path)
    e["Console Output"]["Verbosity"] = "Silent"
    return e


STATE_KEYS = VEC_KEYS + tuple(k for k in SCA_KEYS if k != "Database Entries")


def same_final_files(a, b):
    import json
    ja, jb = json.load(open(a / "latest")), json.load(open(b / "latest"))
    assert ja["Current Generation"] == jb["Current Generation"]
    keys = [k for k in STATE_KEYS if k in ja["Solver"]]  # the fields a result file carries
    assert len(keys) >= 20 and "Sample LogLikelihood Database" in keys and "LogEvidence" in keys
    for k in keys:
        assert ja["Solver"][k] == jb["Solver"][k], k
    for g in ("Multinomial Generator", "Multivariate Generator", "Uniform Generator"):
        assert ja["Solver"][g]["Range"] == jb["Solver"][g]["Range"], g
    assert [d.get("Range") for d in ja["Distributions"]] == [d.get("Range") for d in jb["Distributions"]]


def resumed(path_a, path_b, refill):
    """The run of path_a again from its middle generation's file."""
    import korali
    gens = sorted(f for f in os.listdir(path_a) if f.startswith("gen"))
    assert len(gens) >= 3
    r = korali.Experiment()
    assert r.loadState(str(path_a / gens[len(gens) // 2]))
    r["Preserve Random Number Generator States"] = True
    r["File Output"]["Path"] = str(path_b)
    refill(r)
    korali.Engine().run(r)


def test_engine_psi_then_theta_new(tmp_path):
    import json
    import korali
    subs = [phase1(tmp_path / ("sub%d" % i), 100 + i, 0.5 * i) for i in range(3)]
    kinds = [H.NORMAL, H.NORMAL]
    # --- phase 2: Psi
    korali.Engine().run(psi_run(tmp_path / "psi", subs))
    js = json.load(open(tmp_path / "psi" / "latest"))
    assert js["Is Finished"] is True
    groups = [np.array(json.loads(s.dump())["Solver"]["Sample Database"]) for s in subs]
    lps = [np.array(json.loads(s.dump())["Solver"]["Sample LogPrior Database"]) for s in subs]
    assert all(g.shape == (128, 2) for g in groups)
    db, ll = np.array(js["Solver"]["Sample Database"]), np.array(js["Solver"]["Sample LogLikelihood Database"])
    index, const = [[0, 1], [2, 3]], [[0.0, 0.0]] * 2
    ref = np.array([H.psi_loglik(x, kinds, index, const, groups, lps) for x in db])
    assert db.shape == (128, 4) and same(ll, ref)
    resumed(tmp_path / "psi", tmp_path / "psi_b", lambda r: None)
    same_final_files(tmp_path / "psi", tmp_path / "psi_b")
    # --- phase 3a: ThetaNew on the Psi result
    psi = korali.Experiment()
    assert psi.loadState(str(tmp_path / "psi" / "latest"))
    korali.Engine().run(theta_new_run(tmp_path / "theta", psi))
    jt = json.load(open(tmp_path / "theta" / "latest"))
    assert jt["Is Finished"] is True
    tdb, tll = np.array(jt["Solver"]["Sample Database"]), np.array(jt["Solver"]["Sample LogLikelihood Database"])
    par = H.theta_new_params(kinds, index, const, db)
    ref = np.array([H.theta_new_loglik(x, kinds, index, const, db, params=par) for x in tdb])
    assert tdb.shape == (128, 2) and same(tll, ref)
    resumed(tmp_path / "theta", tmp_path / "theta_b", lambda r: None)
    same_final_files(tmp_path / "theta", tmp_path / "theta_b")


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_distributed_conduit_shards_the_psi_chains(tmp_path):
    """Two ranks on the Distributed conduit (Host transport, sharing the
    device): each evaluates its own pending chains; every rank's state and the
    unsharded Sequential run are bit-identical (tools/distributed_hier_check.py)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for _ in range(3):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
               "--master-addr=127.0.0.1", "--master-port=%d" % free_port(),
               os.path.join(root, "tools", "distributed_hier_check.py"), str(tmp_path), "Host"]
        r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=300)
        if r.returncode == 0 or not ("EADDRINUSE" in r.stderr and "next_rendezvous" in r.stderr):
            break
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [json.load(open(tmp_path / ("rank%d.json" % k))) for k in range(2)]
    for gens in ("1", "3"):
        assert res[1][gens]["sharded"] == res[0][gens]["sharded"], gens
        s, u = res[0][gens]["sharded"], res[0][gens]["unsharded"]
        assert s["Current Generation"] == u["Current Generation"] == int(gens)
        assert s == u, gens
