"""tests/mocmaes_ref.py against the reference's recorded MOCMAES run
(tests/golden/mocmaes_golden.json.gz: 36 states, one every 10 generations),
and its vectorised sort against the literal one."""
import numpy as np
import pytest

import mocmaes_ref as mr


@pytest.fixture(scope="module")
def states():
    return mr.load_golden()


def _getter(m):
    return lambda name: m.f[name]


def _check_exception_window(m, sv, window):
    # what still has to hold where a value field is exempt
    assert np.array_equal(m.f["Sample Collection"], np.asarray(sv["Sample Collection"]).reshape(-1, m.N))
    assert np.array_equal(m.f["Current Sample Population"], np.asarray(sv["Current Sample Population"]))
    for X, V in (("Sample Collection", "Sample Value Collection"), ("Current Sample Population", "Current Values")):
        want = [m.objective([float(v) for v in x]) for x in m.f[X]]
        assert np.array_equal(m.f[V], np.asarray(want, dtype=np.float64).reshape(-1, m.K))


@pytest.mark.parametrize("k", range(35))
def test_window_reproduces(states, k):
    m = mr.recorded_setup(states)
    window = 10 * k
    if k > 0:
        m.load(states[k]["Solver"])
    for _ in range(10):
        m.generation()
    sv = states[k + 1]["Solver"]
    assert mr.mismatches(_getter(m), (m.normal.to_hex(), m.uniform.to_hex()), sv, window) == []
    if any(w == window for w, _ in mr.VALUE_EXCEPTIONS):
        _check_exception_window(m, sv, window)


def test_exceptions_are_value_only(states):
    # every listed exception names an objective-value field of an existing window
    assert len(mr.VALUE_EXCEPTIONS) == 4
    for window, name in mr.VALUE_EXCEPTIONS:
        assert window % 10 == 0 and 0 <= window < 350
        assert name in ("Sample Value Collection", "Current Values")


def test_snapshot_order_does_not_reproduce(states):
    # the switch is needed: with the snapshot's slot order the first window fails
    m = mr.recorded_setup(states, parent_order="descending")
    for _ in range(10):
        m.generation()
    assert mr.mismatches(_getter(m), (m.normal.to_hex(), m.uniform.to_hex()), states[1]["Solver"], 0) != []


def test_recorded_values_are_the_objective(states):
    rows = bad = 0
    for s in states[1:]:
        sv = s["Solver"]
        for x, v in zip(sv["Current Sample Population"], sv["Current Values"]):
            rows += 1
            bad += mr.negative_rosenbrock_and_sphere(x) != v
    assert rows == 1120 and bad <= 1


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("n", [1, 2, 7, 64, 128])
@pytest.mark.parametrize("grid", [False, True])
def test_vectorised_sort_equals_literal(K, n, grid):
    rng = np.random.default_rng(1000 * K + n + (7 if grid else 0))
    v = rng.normal(size=(n, K))
    if grid:
        v = np.round(v * 4.0) / 4.0  # ties in nBetter and in the contributions
    if n >= 7:
        v[n // 2:n // 2 + 2] = -np.inf  # the first generation's 'Previous Values'
    assert mr.sort_vectorised(v.tolist()) == mr.sort_literal(v.tolist())
