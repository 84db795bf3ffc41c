"""Optimizer/MOCMAES on the device (kg_mocmaes_*, korali_amd/csrc/kg_mocmaes.hip)
against the reference's recorded run (tests/golden/mocmaes_golden.json.gz) and
against the NumPy restatement (tests/mocmaes_ref.py, itself checked against the
recording by tests/test_mocmaes_ref_golden.py).  Every comparison is exact."""
import numpy as np
import pytest

import mocmaes_ref as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def states():
    return mr.load_golden()


def recorded_device(states, **kw):
    from korali_amd.native import MocmaesDevice
    sv, var = states[0]["Solver"], states[0]["Variables"]
    kw.setdefault("parent_order", "Recorded")
    return MocmaesDevice(len(var), sv["Population Size"], [v["Lower Bound"] for v in var],
                         [v["Upper Bound"] for v in var], mu=sv["Mu Value"], num_objectives=2,
                         initial_value=[v["Initial Value"] for v in var],
                         initial_sdev=[v["Initial Standard Deviation"] for v in var],
                         multinormal_seed=sv["Multinormal Generator"]["Random Seed"],
                         uniform_seed=sv["Uniform Generator"]["Random Seed"], **kw)


def ranges(dev):
    return dev.rng_state(0).hex().upper(), dev.rng_state(1).hex().upper()


def load(dev, sv):
    for name in mr.FIELDS + mr.SCALARS:
        rname = mr.RECORDED_NAMES.get(name, name)
        if rname in sv:
            dev[name] = sv[rname]
    dev.set_rng_state(bytes.fromhex(sv["Multinormal Generator"]["Range"]), 0)
    dev.set_rng_state(bytes.fromhex(sv["Uniform Generator"]["Range"]), 1)


def check_exception_window(dev, sv, window):
    """What still has to hold where a value field is exempt."""
    N, K = dev.N, dev.K
    assert np.array_equal(dev["Sample Collection"], np.asarray(sv["Sample Collection"], dtype=np.float64).reshape(-1))
    for X, V in (("Sample Collection", "Sample Value Collection"), ("Current Sample Population", "Current Values")):
        want = [mr.negative_rosenbrock_and_sphere([float(v) for v in x]) for x in dev[X].reshape(-1, N)]
        assert np.array_equal(dev[V], np.asarray(want, dtype=np.float64).reshape(-1)), (window, V)
    assert K == 2


@pytest.fixture(scope="module")
def forced(states):
    dev = recorded_device(states)
    yield dev
    dev.close()


@pytest.mark.parametrize("k", range(1, 35))
def test_teacher_forced_against_the_recording(forced, states, k):
    dev, window = forced, 10 * k
    load(dev, states[k]["Solver"])
    for g in range(window + 1, window + 11):
        dev.generation(g, "negative_rosenbrock_and_sphere")
    dev.synchronize()
    sv = states[k + 1]["Solver"]
    assert mr.mismatches(lambda name: dev[name], ranges(dev), sv, window) == []
    if any(w == window for w, _ in mr.VALUE_EXCEPTIONS):
        check_exception_window(dev, sv, window)


def test_seeded_run_reproduces_every_recorded_state(states):
    """350 generations from the recorded seeds, checked at every recorded
    state.  An archive row whose recorded value differs in one of the listed
    windows (the recorder's `**2`, mr.VALUE_EXCEPTIONS) stays in the archive
    after that window.  Only such a row, known by its parameters, may differ
    from the recording in a later state's 'Sample Value Collection'; every
    other row equals it, and every value is the objective of its parameters."""
    dev = recorded_device(states)
    assert ranges(dev) == (states[0]["Solver"]["Multinormal Generator"]["Range"],
                           states[0]["Solver"]["Uniform Generator"]["Range"])
    excepted_rows = set()  # parameters of the archive rows that differed in a listed window
    for g in range(1, 351):
        dev.generation(g, "negative_rosenbrock_and_sphere")
        if g % 10:
            continue
        dev.synchronize()
        sv, window = states[g // 10]["Solver"], g - 10
        listed = (window, "Sample Value Collection") in mr.VALUE_EXCEPTIONS
        bad = mr.mismatches(lambda name: dev[name], ranges(dev), sv, window)
        if "Sample Value Collection" in bad or listed:
            # (lengths and 'Sample Collection' are compared by mismatches: a failure there stays in `bad`)
            X = np.asarray(sv["Sample Collection"], dtype=np.float64).reshape(-1, dev.N)
            want = np.asarray(sv["Sample Value Collection"], dtype=np.float64).reshape(-1, dev.K)
            got = dev["Sample Value Collection"].reshape(-1, dev.K)
            assert got.shape == want.shape, g
            differing = {tuple(X[r]) for r in np.flatnonzero((got != want).any(axis=1))}
            if listed:
                excepted_rows |= differing
            assert differing <= excepted_rows, g
            if "Sample Value Collection" in bad:
                bad.remove("Sample Value Collection")
            check_exception_window(dev, sv, window)
        assert bad == [], g
        if any(w == window for w, _ in mr.VALUE_EXCEPTIONS):
            check_exception_window(dev, sv, window)
    assert len(excepted_rows) <= 5  # "one or two elements" in each of three windows
    dev.close()


def quantised(X):
    """A host objective on a 0.25 grid: ties in nBetter, in the ranks and in the contributions."""
    return [[round(4.0 * v) / 4.0 for v in mr.negative_rosenbrock_and_sphere([float(t) for t in x])] for x in X]


# N, P, mu, K, generations, bound (in initial standard deviations), host objective, extra device settings
CASES = {
    "N1": (1, 4, 2, 2, 6, 8.0, None, {}),
    "N3-K3": (3, 32, 16, 3, 6, 8.0, None, {}),
    "N33-mu=P": (33, 33, 33, 2, 6, 8.0, None, {}),
    "N65-mu1": (65, 300, 1, 2, 6, 8.0, None, {}),
    "N128": (128, 300, 150, 2, 6, 8.0, None, {}),
    "N128-K3": (128, 128, 64, 3, 6, 8.0, None, {}),
    "tight-bounds": (3, 32, 16, 2, 6, 0.5, None, {}),
    "ties": (2, 33, 16, 2, 6, 8.0, quantised, {}),
    "multi-workgroup-sort": (2, 1100, 550, 2, 6, 8.0, None, {}),
    "archive-grows": (3, 32, 16, 2, 6, 8.0, None, {"archive_rows": 1}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_generations_equal_the_restatement(case):
    from korali_amd.native import MocmaesDevice
    N, P, mu, K, gens, bound, host, extra = CASES[case]
    sdev = [1.0 + 0.25 * (d % 3) for d in range(N)]
    lower, upper = [-bound * s for s in sdev], [bound * s for s in sdev]
    ref = mr.Mocmaes(lower, upper, P, mu=mu, num_objectives=K, initial_sdev=sdev, normal_seed=1234 + N,
                     uniform_seed=99 + P)
    dev = MocmaesDevice(N, P, lower, upper, mu=mu, num_objectives=K, initial_sdev=sdev, multinormal_seed=1234 + N,
                        uniform_seed=99 + P, **extra)
    uniform0 = ranges(dev)[1]
    assert ranges(dev) == (ref.normal.to_hex(), ref.uniform.to_hex())
    kernel = "negative_rosenbrock_and_sphere" if K == 2 else "negative_rosenbrock_and_two_spheres"
    windows = rounds = blocks = 0
    for g in range(1, gens + 1):
        ref.generation(values=host)
        blocks += ref.blocks_last
        if host:
            dev.prepare(g)
            dev.set_values(host(dev.candidates()))
            dev.update(g)
        else:
            dev.generation(g, kernel)
        dev.synchronize()
        assert mr.mismatches(lambda name: dev[name], ranges(dev), mr.as_recorded(ref), None) == [], g
        d = dev.diagnostics()
        windows, rounds = max(windows, d[0]), max(rounds, d[3])
        if g == 1 and mu < P:
            assert np.all(dev["Parent Index"] == 0)  # 'Current Non Dominated Sample Count' starts at 1
    if mu == P:
        assert ranges(dev)[1] == uniform0  # parentIdx = i: the uniform stream is not touched
    if case == "tight-bounds":
        # most draws are rejected, and some generation needs more blocks than the first window holds
        assert blocks > 2 * gens * P and windows > 1
    if 2 * P > 2048:
        assert rounds > 16  # the multi-workgroup sort ran, through more than one batch of queued rounds
    else:
        assert rounds == 0  # the one-workgroup sort
    if case == "archive-grows":
        rows = dev.field_size("Sample Collection") // N
        assert rows > 1 and dev.diagnostics()[2] >= rows + P  # more rows than the first allocation's one
    dev.close()


def test_fields_round_trip():
    from korali_amd.native import MocmaesDevice
    N, P, mu, K = 3, 8, 4, 2
    dev = MocmaesDevice(N, P, -1.0, 1.0, mu=mu, num_objectives=K)
    dev.initialize()
    rng = np.random.default_rng(5)
    dev["Sample Collection"] = rng.normal(size=(5, N))
    for name in mr.FIELDS + mr.SCALARS + ["Finished Sample Count"]:
        n = dev.field_size(name)
        v = rng.normal(size=n)
        dev[name] = v
        assert np.array_equal(dev[name], v), name
    assert dev.field_size("Sample Collection") == 5 * N and dev.field_size("Sample Value Collection") == 5 * K
    dev["Sample Collection"] = np.zeros(0)
    assert dev.field_size("Sample Value Collection") == 0
    with pytest.raises(Exception, match="unknown MOCMAES field"):
        dev["No Such Field"]
    with pytest.raises(Exception, match="size mismatch"):
        dev["Current Sigma"] = np.zeros(P + 1)
    dev.close()


def test_both_generator_states_export_and_import():
    from oracle import refcpu
    from korali_amd.native import MocmaesDevice
    dev = MocmaesDevice(2, 8, -1.0, 1.0, multinormal_seed=11, uniform_seed=12)
    a, b = refcpu.Rng(seed=11), refcpu.Rng(seed=12)
    assert ranges(dev) == (a.to_hex(), b.to_hex())
    for _ in range(1000):
        a.get()
        b.get()
    dev.set_rng_state(b.get_bytes(), 0)
    dev.set_rng_state(a.get_bytes(), 1)
    assert ranges(dev) == (b.to_hex(), a.to_hex())
    dev.close()


def test_infeasible_configuration_is_reported():
    """Bounds no draw can meet: the reference would redraw forever; the device stops at max_windows."""
    from korali_amd.native import KoraliDeviceError, MocmaesDevice
    dev = MocmaesDevice(2, 8, [5.0, 5.0], [5.0 + 1e-300, 5.0 + 1e-300], initial_sdev=[1.0, 1.0], max_windows=2)
    with pytest.raises(KoraliDeviceError, match="no feasible draw after 2 windows"):
        dev.prepare(1)
    dev.close()
