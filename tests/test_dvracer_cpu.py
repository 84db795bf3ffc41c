"""CPU checks of the dVRACER restatement (tests/dvracer_ref.py) against
independent definitions, and of the engine's configuration handling of
`Agent / Discrete / dVRACER` before it reaches the device."""
import numpy as np
import pytest

import dvracer_ref as D

f32, f64 = np.float32, np.float64


def policies(K, seed, n=20):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        q = rng.normal(0, 1.5, K).astype(f32)
        invT = f32(rng.uniform(0.05, 1.0))
        yield q, invT, np.concatenate([[f32(0.3)], q, [invT]]).astype(f32)


def softmax64(q, invT):
    z = np.asarray(q, f64) * f64(invT)
    e = np.exp(z - z.max())
    return e / e.sum()


@pytest.mark.parametrize("K", [1, 2, 3, 7])
def test_softmax_sums_to_one_and_is_shift_invariant(K):
    for q, invT, row in policies(K, K):
        p, q2, t2 = D.softmax_policy(row, K)
        assert p.dtype == f32 and np.array_equal(q2, q) and t2 == invT
        assert abs(f64(p.astype(f64).sum()) - 1.0) <= 4 * np.finfo(f32).eps
        np.testing.assert_allclose(p, softmax64(q, invT), rtol=1e-5, atol=1e-7)
        # a shift of every q by a power of two leaves q_i - max q, and so p, unchanged
        shifted = row.copy()
        shifted[1:1 + K] += f32(4.0)
        if np.array_equal((shifted[1:1 + K] - f32(4.0)).astype(f32), q):
            assert np.array_equal(D.softmax_policy(shifted, K)[0], p)
        np.testing.assert_allclose(D.softmax_policy(shifted, K)[0], p, rtol=2e-6, atol=1e-7)


def central(f, x, i, h=1e-6):
    a, b = np.array(x, f64), np.array(x, f64)
    a[i] += h
    b[i] -= h
    return (f(a) - f(b)) / (2 * h)


@pytest.mark.parametrize("K", [2, 3, 7])
def test_importance_weight_gradient_matches_central_differences(K):
    rng = np.random.default_rng(10 + K)
    for q, invT, row in policies(K, 20 + K):
        p_cur = D.softmax_policy(row, K)[0]
        p_old = rng.dirichlet(np.ones(K)).astype(f32)
        a = int(rng.integers(K))

        def w(x):
            return softmax64(x[:K], x[K])[a] / (f64(p_old[a]) + 1e-8)

        x0 = np.concatenate([q, [invT]]).astype(f64)
        g = D.importance_weight_gradient(q, invT, p_cur, p_old, a)
        if w(x0) < 1000.0:  # (not clamped)
            ref = np.array([central(w, x0, i) for i in range(K + 1)])
            np.testing.assert_allclose(g, ref, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize("K", [2, 3, 7])
def test_kl_gradient_matches_central_differences(K):
    rng = np.random.default_rng(30 + K)
    for q, invT, row in policies(K, 40 + K):
        p_cur = D.softmax_policy(row, K)[0]
        p_old = rng.dirichlet(np.ones(K)).astype(f32)

        def kl(x):
            pc = softmax64(x[:K], x[K])
            po = p_old.astype(f64)
            return float(np.sum(po * np.log(po / pc)))

        x0 = np.concatenate([q, [invT]]).astype(f64)
        ref = np.array([central(kl, x0, i) for i in range(K + 1)])
        # the written gradient treats sum_j pOld_j as 1; the float32 Dirichlet draw sums to 1 within 1e-7
        np.testing.assert_allclose(D.kl_gradient(q, invT, p_cur, p_old), ref, rtol=2e-4,
                                   atol=2e-5 * max(1.0, np.abs(ref).max()))


def test_categorical_edges():
    p = np.array([0.2, 0.3, 0.1, 0.4], f32)
    b = D.boundaries(p)
    assert D.categorical(p, f32(0.0)) == 0 and D.categorical(p, np.nextafter(p[0], f32(0))) == 0
    assert D.categorical(p, p[0]) == 1  # x < curSum is strict
    assert D.categorical(p, b[-1]) == 3 and D.categorical(p, f32(0.999999)) == 3
    assert D.categorical(p, np.nextafter(b[-1], f32(0))) == 2
    assert D.categorical(np.array([1.0], f32), f32(0.7)) == 0  # K = 1: no comparison at all
    assert D.categorical(np.array([0.0, 1.0], f32), f32(0.0)) == 1


def test_testing_picks_the_first_maximum():
    assert D.testing_index(np.array([0.2, 0.4, 0.4], f32)) == 1
    assert D.testing_index(np.array([0.5, 0.5], f32)) == 0
    row = np.array([0.0, 1.0, 1.0, 0.5, 0.7], f32)  # equal q: equal p
    assert D.testing_index(D.softmax_policy(row, 3)[0]) == 0


def test_sigmoid_forward_and_backward():
    x = np.linspace(-6, 6, 41).astype(f32)
    y = D.sigmoid(x)
    np.testing.assert_allclose(y, 1.0 / (1.0 + np.exp(-x.astype(f64))), rtol=3e-7)
    h = 1e-3
    fd = (1.0 / (1.0 + np.exp(-(x.astype(f64) + h))) - 1.0 / (1.0 + np.exp(-(x.astype(f64) - h)))) / (2 * h)
    g = np.full_like(x, 1.7)
    np.testing.assert_allclose(D.sigmoid_backward(g, y), 1.7 * fd, rtol=1e-5, atol=1e-7)


def test_importance_weight_clamp():
    p_cur = np.array([0.25, 0.75], f32)
    assert D.importance_weight(p_cur, np.array([0.0, 1.0], f32), 0) == f32(1024.0)  # 0.25 / 1e-8
    assert D.importance_weight(p_cur, np.array([0.5, 0.5], f32), 0) == f32(f32(0.25) / f32(f32(0.5) + f32(1e-8)))
    g = D.importance_weight_gradient(np.array([0.1, 0.2], f32), f32(0.5), p_cur, np.array([0.0, 1.0], f32), 0)
    assert g[0] == f32(f64(f32(1024.0)) * (1.0 - f64(p_cur[0])) * 0.5)


def test_forward_backward_consistent():
    """the local forward / backward (sigmoid on the last output) against a finite difference of the forward"""
    S, H, L, K = 3, 8, 2, 3
    rng = np.random.default_rng(1)
    th = D.initial_hyperparameters(S, H, L, K, rng.uniform(-1, 1, D.hyperparameter_count(S, H, L, K)), 1.0)
    X = rng.standard_normal((5, S)).astype(f32)
    out, acts = D.forward(th, X, S, H, L, K)
    assert out.shape == (5, K + 2) and np.all((out[:, K + 1] > 0) & (out[:, K + 1] < 1))
    G = rng.standard_normal(out.shape).astype(f32)
    grad = D.backward(th, acts, out, G, S, H, L, K)
    for j in rng.integers(0, th.size, 12):
        a, b = th.astype(f64), th.astype(f64)
        a[j] += 1e-3
        b[j] -= 1e-3
        fa = D.forward(a.astype(f32), X, S, H, L, K)[0].astype(f64)
        fb = D.forward(b.astype(f32), X, S, H, L, K)[0].astype(f64)
        assert abs(np.sum(G * (fa - fb)) / 2e-3 - grad[j]) <= 2e-2 * max(1.0, abs(grad[j]))


# ------------------------------------------------------------------ engine
def experiment(**kw):
    from dvracer_cases import cartpole_dvracer
    return cartpole_dvracer(max_generations=1, **kw)


def run_fails(e, msg):
    import korali
    with pytest.raises(korali.KoraliError, match=msg):
        korali.Engine().run(e)


def test_possible_actions_empty_set():
    e = experiment()
    e["Problem"]["Possible Actions"] = []
    run_fails(e, r"No possible actions have been defined for the discrete RL problem \(empty set detected\)")


def test_possible_actions_wrong_vector_size():
    e = experiment()
    e["Problem"]["Possible Actions"] = [[-10.0], [10.0, 1.0]]
    run_fails(e, r"For possible action 1, incorrect vector size provided. Expected: 1, Provided: 2\.")


def test_problem_and_solver_types_must_match():
    e = experiment()
    e["Problem"]["Type"] = "Reinforcement Learning / Continuous"
    run_fails(e, "dVRACER requires a problem of type 'Reinforcement Learning / Discrete'")
    from vracer_cases import cartpole_vracer
    v = cartpole_vracer(max_generations=1)
    v["Problem"]["Type"] = "Reinforcement Learning / Discrete"
    run_fails(v, "VRACER requires a problem of type 'Reinforcement Learning / Continuous'")


def test_too_many_possible_actions_and_action_variables():
    e = experiment()
    e["Problem"]["Possible Actions"] = [[float(i)] for i in range(8)]
    run_fails(e, "up to 7 'Possible Actions'")
    e = experiment(kernel=None)
    for i in range(5, 9):
        e["Variables"][i]["Name"] = f"Extra {i}"
        e["Variables"][i]["Type"] = "Action"
    e["Problem"]["Possible Actions"] = [[0.0] * 5, [1.0] * 5]
    run_fails(e, "up to 4 action variables")


@pytest.mark.parametrize("edit,msg", [
    (lambda e: e["Solver"]["Policy"].__setitem__("Distribution", "Normal"), "Unrecognized settings"),
    (lambda e: e["Solver"].__setitem__("Mini Batch Sise", 3), "Unrecognized settings"),
    (lambda e: e["Problem"].__setitem__("Possible Action", [[1.0]]), "Unrecognized settings"),
    (lambda e: e["Solver"]["Neural Network"].__setitem__("Optimizer", "AdaGrad"), "not supported by the device path"),
    (lambda e: e["Solver"].__setitem__("Time Sequence Length", 2), "Time Sequence Length"),
    (lambda e: e["Problem"].__setitem__("Agents Per Environment", 2), "Agents Per Environment"),
    (lambda e: e["Problem"].__setitem__("Environment Kernel", "Pendulum"), "Unknown 'Environment Kernel'"),
])
def test_configuration_errors_before_device(edit, msg):
    e = experiment()
    edit(e)
    run_fails(e, msg)


def test_initial_exploration_noise_is_optional_and_unused():
    """dVRACER.config keeps the variable key; neither its absence nor a value is an error (the run then
    goes on to the device, which this machine may lack: only configuration errors are excluded here)"""
    import korali
    e = experiment()
    e["Variables"][4]["Initial Exploration Noise"] = 0.5
    e["Problem"]["Possible Actions"] = []
    run_fails(e, "empty set detected")  # (reached after the variables were accepted)
    assert korali is not None


@pytest.mark.parametrize("K", [2, 7])
def test_dvracer_policy_description(K):
    from korali_amd import libkorali
    e = experiment()
    e["Problem"]["Possible Actions"] = [[float(i)] for i in range(K)]
    d = libkorali._dvracer_policy_description(e)
    pol = d["Solver"]["Policy"]
    assert pol["Parameter Count"] == K + 1
    assert pol["Parameter Scaling"] == [1.0] * (K + 1) and pol["Parameter Shifting"] == [0.0] * (K + 1)
    assert pol["Parameter Transformation Masks"] == ["Identity"] * K + ["Sigmoid"]
    assert d["Layer Sizes"] == [4, 32, 32, K + 2]
    assert d["Hyperparameter Count"] == D.hyperparameter_count(4, 32, 2, K)
    assert d["Problem"]["State Vector Size"] == 4 and d["Problem"]["Action Vector Size"] == 1
    assert d["Problem"]["State Vector Indexes"] == [0, 1, 2, 3] and d["Problem"]["Action Vector Indexes"] == [4]
