"""tests/supervisor_ref.py against calculus, hand-computed optimizer steps and
the sine-wave example (no GPU)."""
import numpy as np
import pytest

import supervisor_ref as SR

f32, f64 = np.float32, np.float64


def lin(n):
    return {"Type": "Layer/Linear", "Output Channels": n}


def act(fn, alpha=1.0, beta=0.0):
    return {"Type": "Layer/Activation", "Function": fn, "Alpha": alpha, "Beta": beta}


def numeric_gradient(f, x, h=1e-6):
    g = np.zeros_like(x)
    for i in range(x.size):
        d = np.zeros_like(x)
        d.flat[i] = h
        g.flat[i] = (f(x + d) - f(x - d)) / (2 * h)
    return g


TRUE_DERIVATIVES = [("Elementwise/Tanh", 1.0, 0.0), ("Elementwise/ReLU", 0.2, 0.0), ("Elementwise/Logistic", 1.0, 0.0),
                    ("Elementwise/SoftReLU", 1.0, 0.0), ("Elementwise/Linear", 0.7, 0.3), ("Elementwise/Log", 1.0, 0.0)]


@pytest.mark.parametrize("fn,alpha,beta", TRUE_DERIVATIVES)
def test_backward_is_the_derivative(fn, alpha, beta):
    """float64 mode: d sum(G * output) / d theta by central differences = backward(G), through Linear,
    the activation (fused position and output position) and Linear again"""
    I, O, B = 3, 2, 4
    layers = [lin(5), act(fn, alpha, beta), lin(O), act(fn, alpha, beta)]
    rng = np.random.default_rng(0)
    theta = rng.uniform(0.1, 1.0, SR.hyperparameter_count(I, layers))  # positive: Log's argument stays positive
    if fn != "Elementwise/Log":
        theta *= rng.choice([-1.0, 1.0], theta.size)
    X, G = rng.uniform(0.2, 1.0, (B, I)), rng.standard_normal((B, O))
    if fn == "Elementwise/Log":
        for W, b in SR.unpack(theta, I, layers).values():
            b += 2.0
    f = lambda t: float((G * SR.forward(t, X, I, layers, None, f64)[-1]).sum())
    grad, _ = SR.backward(theta, SR.forward(theta, X, I, layers, None, f64), G, I, layers, None, f64)
    num = numeric_gradient(f, theta)
    assert np.allclose(grad, num, rtol=1e-6, atol=1e-8), np.abs(grad - num).max()


@pytest.mark.parametrize("mask", ["Softplus", "Tanh", "Sigmoid", "Absolute"])
def test_output_mask_backward_is_the_derivative(mask):
    I, O, B = 3, 2, 5
    layers = [lin(4), act("Elementwise/Tanh"), lin(O)]
    out = {"Scale": [2.0, 0.5], "Shift": [0.25, -1.0], "Transformation Mask": [mask, "Identity"]}
    rng = np.random.default_rng(1)
    theta = rng.uniform(-1, 1, SR.hyperparameter_count(I, layers))
    SR.unpack(theta, I, layers)[3][1][0] = 3.0  # the masked output's bias: away from 0 (Absolute)
    X, G = rng.standard_normal((B, I)), rng.standard_normal((B, O))
    f = lambda t: float((G * SR.forward(t, X, I, layers, out, f64)[-1]).sum())
    vals = SR.forward(theta, X, I, layers, out, f64)
    assert np.all(np.abs(vals[-2][:, 0]) > 0.5)
    grad, _ = SR.backward(theta, vals, G, I, layers, out, f64)
    num = numeric_gradient(f, theta)
    assert np.allclose(grad, num, rtol=1e-6, atol=1e-8), np.abs(grad - num).max()


def test_softmax_and_softsign_are_the_literal_formulas():
    rng = np.random.default_rng(2)
    z, g = rng.standard_normal((4, 6)), rng.standard_normal((4, 6))
    y = SR.activation("Softmax", z, 1.0, 0.0, f64)
    assert np.allclose(y, np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)) and np.allclose(y.sum(axis=1), 1.0)
    # the diagonal of the Jacobian only (activation.cpp.base:311-313)
    assert np.array_equal(SR.activation_backward("Softmax", g, y, z, 1.0, f64), g * y * (1.0 - y))
    full = np.einsum("bi,bij->bj", g, np.einsum("bi,ij->bij", y, np.eye(6)) - np.einsum("bi,bj->bij", y, y))
    assert not np.allclose(SR.activation_backward("Softmax", g, y, z, 1.0, f64), full)
    y = SR.activation("Elementwise/SoftSign", z, 1.0, 0.0, f64)
    assert np.array_equal(y, z / (1.0 + np.abs(z)))
    # with the layer's OUTPUT where the derivative 1 / (1 + |z|)^2 has the input (:307-309)
    assert np.array_equal(SR.activation_backward("Elementwise/SoftSign", g, y, z, 1.0, f64), g / ((1.0 + np.abs(y)) * (1.0 + np.abs(y))))
    assert not np.allclose(SR.activation_backward("Elementwise/SoftSign", g, y, z, 1.0, f64), g / (1.0 + np.abs(z)) ** 2)


def test_bias_gradient_is_the_column_sum_and_loss_is_half_mean():
    I, O, B = 2, 3, 7
    layers = [lin(O)]
    rng = np.random.default_rng(3)
    theta = rng.standard_normal(SR.hyperparameter_count(I, layers))
    X, S = rng.standard_normal((B, I)), rng.standard_normal((B, O))
    vals = SR.forward(theta, X, I, layers, None, f64)
    g, loss = SR.mse_gradient(S, vals[-1], f64)
    assert np.array_equal(g, S - vals[-1]) and np.isclose(loss, (g * g).sum() / (2 * B))
    grad, _ = SR.backward(theta, vals, g, I, layers, None, f64)
    assert np.allclose(SR.unpack(grad, I, layers)[1][1], g.sum(axis=0))
    assert np.allclose(SR.unpack(grad, I, layers)[1][0], g.T @ X)


# one step from th = 0.5, g = 2, eta = 0.1 and zero state, by hand (the reference ASCENDS along g)
def test_adam_step_by_hand():
    st = SR.new_state("Adam", 1, f64)
    th = SR.optimizer_step("Adam", [0.5], [2.0], st, 0.1, f64)
    m, v = -f64(f32(1.0) - f32(0.9)) * 2.0, f64(f32(1.0) - f32(0.999)) * 4.0  # (1.0f - beta in float32)
    f1, f2 = f64(f32(1.0) / (f32(1.0) - f32(0.9))), f64(f32(1.0) / (f32(1.0) - f32(0.999)))
    assert np.isclose(st["first_moment"][0], m) and np.isclose(st["second_moment"][0], v)
    assert np.isclose(th[0], 0.5 - f64(f32(0.1)) / (np.sqrt(v * f2) + 1e-8) * m * f1)
    assert abs(th[0] - 0.6) < 1e-6  # a full step of eta towards +g


def test_adabelief_step_by_hand():
    st = SR.new_state("AdaBelief", 1, f64)
    th = SR.optimizer_step("AdaBelief", [0.5], [2.0], st, 0.1, f64)
    m = -f64(f32(1.0) - f32(0.9)) * 2.0
    c = f64(f32(1.0) - f32(0.999)) * (2.0 + m) ** 2
    assert np.isclose(st["first_moment"][0], m) and np.isclose(st["second_central_moment"][0], c)
    assert np.isclose(th[0], 0.5 - 0.1 / (np.sqrt(c * 1000.0) + 1e-8) * (m * 10.0), rtol=1e-5)


def test_madgrad_step_by_hand():
    st = SR.new_state("MADGRAD", 1, f64)
    th = SR.optimizer_step("MADGRAD", [0.5], [2.0], st, 0.1, f64)
    s, v = f64(f32(0.1)) * 2.0, -f64(f32(0.1)) * 4.0
    z = 0.0 - 1.0 / (np.cbrt(v) + f64(f32(1e-8))) * s
    assert np.isclose(st["s"][0], s) and np.isclose(st["v"][0], v) and np.isclose(st["z"][0], z)
    assert np.isclose(th[0], (1 - f64(f32(0.9))) * 0.5 + f64(f32(0.9)) * z) and z > 0


def test_rmsprop_step_by_hand():
    st = SR.new_state("RMSProp", 1, f64)
    th = SR.optimizer_step("RMSProp", [0.5], [2.0], st, 0.1, f64)
    r = (1 - f64(f32(0.999))) * 4.0
    v = f64(f32(0.1)) / (np.sqrt(r) + f64(f32(1e-8))) * -2.0
    assert np.isclose(st["r"][0], r) and np.isclose(st["v"][0], v) and np.isclose(th[0], 0.5 - v) and th[0] > 0.5


def test_adagrad_step_by_hand():
    st = SR.new_state("Adagrad", 1, f64)
    th = SR.optimizer_step("Adagrad", [0.5], [2.0], st, 0.1, f64)
    assert st["s"][0] == 4.0 and np.isclose(th[0], 0.5 + f64(f32(0.1)) / np.sqrt(4.0 + f64(f32(1e-8))) * 2.0)
    assert abs(th[0] - 0.6) < 1e-6


def test_l2_importance_is_truncated():
    assert SR.l2_importance(0.05) == 0.0 and SR.l2_importance(1e-4) == 0.0 and SR.l2_importance(2.7) == 2.0
    I, layers = 1, [lin(1)]
    X, S, th = np.ones((1, 1)), np.ones((1, 1)), np.asarray([0.3, 0.1])
    a, _, _ = SR.train(th, X, S, I, layers, eta=0.1, l2=SR.l2_importance(0.05), dtype=f64)
    b, _, _ = SR.train(th, X, S, I, layers, eta=0.1, l2=None, dtype=f64)
    assert np.array_equal(a, b)


def test_float32_mode_follows_float64_mode():
    I, O, B = 3, 2, 6
    layers = [lin(8), act("Elementwise/Tanh"), lin(O)]
    out = {"Scale": [2.0, 0.5], "Shift": [0.25, -1.0], "Transformation Mask": ["Softplus", "Sigmoid"]}
    rng = np.random.default_rng(4)
    th = rng.uniform(-1, 1, SR.hyperparameter_count(I, layers)).astype(f32)
    X, S = rng.standard_normal((B, I)).astype(f32), rng.standard_normal((B, O)).astype(f32)
    a, _, la = SR.train(th, X, S, I, layers, out, "Adam", 0.01, 3, dtype=f32)
    b, _, lb = SR.train(th, X, S, I, layers, out, "Adam", 0.01, 3, dtype=f64)
    assert a.dtype == f32 and b.dtype == f64 and np.allclose(a, b, rtol=1e-3, atol=1e-5) and np.isclose(la, lb, rtol=1e-4)


def test_initial_hyperparameters_layout_and_scale():
    I = 3
    layers = [dict(lin(4), **{"Weight Scaling": 1.0}), act("Elementwise/Tanh"), dict(lin(2), **{"Weight Scaling": 0.5})]
    th = SR.initial_hyperparameters(I, layers, 1234)
    P = SR.unpack(th, I, layers)
    assert th.dtype == f32 and th.size == 3 * 4 + 4 + 4 * 2 + 2
    assert np.all(P[1][1] == 0) and np.all(P[3][1] == 0)
    assert np.all(np.abs(P[1][0]) <= np.sqrt(6.0 / 7.0)) and np.all(np.abs(P[3][0]) <= 0.5 * np.sqrt(6.0 / 6.0))
    assert np.abs(P[1][0]).max() > 0.3 and np.array_equal(th, SR.initial_hyperparameters(I, layers, 1234))
    assert not np.array_equal(th, SR.initial_hyperparameters(I, layers, 1235))


def sine_wave(n, rng):
    x = rng.uniform(0, 2 * np.pi, n)
    return x, np.tanh(np.exp(np.sin(x))) * 5.0


def test_sine_wave_example_reaches_its_threshold():
    """examples/learning/supervised/sineWave/run-ffn.py: batch 500, two Tanh layers of 32, Adam, learning
    rate 0.005, 10 generations of 200 steps, the script's seed for the data; its own threshold is 0.05"""
    rs = np.random.RandomState(0xC0FFEE)
    x, y = sine_wave(500, rs)
    I, layers = 1, [lin(32), act("Elementwise/Tanh"), lin(32), act("Elementwise/Tanh"), lin(1)]
    theta = SR.initial_hyperparameters(I, layers, 0xC0FFEE)
    theta, _, loss = SR.train(theta, x[:, None], y[:, None], I, layers, None, "Adam", 0.005, 2000, dtype=f32)
    xt, yt = sine_wave(100, rs)
    mse = np.mean((SR.forward(theta, xt[:, None], I, layers, None, f32)[-1][:, 0].astype(f64) - yt) ** 2)
    assert mse < 0.05, mse
