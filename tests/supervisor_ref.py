"""NumPy restatement of Learner/DeepSupervisor on a Supervised Learning
problem (feed-forward, one timestep) -- TEST INFRASTRUCTURE ONLY.

Restated from the reference (paths relative to the korali root):
  solver/learner/deepSupervisor/deepSupervisor.cpp.base      the step loop :97-161
  neuralNetwork/layer/linear/linear.cpp.base                 :28-49, :219-232, :284-292, :337-350
  neuralNetwork/layer/activation/activation.cpp.base         :147-209, :270-314 ("Korali" engine)
  neuralNetwork/layer/output/output.cpp.base                 :141-162, :175-212
  solver/learner/deepSupervisor/optimizers/f*.cpp            processResult

Two modes.  dtype=float32 mirrors the reference's operations one by one (the
same operation order per element, the same double stages in the Output
layer; products through NumPy's float32 matmul).  dtype=float64 evaluates
the same formulas in double throughout: the value a float32 evaluation is
measured against.

A network is a list of layers after the input, in the reference's JSON form:
{"Type": "Layer/Linear", "Output Channels": n, "Weight Scaling": s} and
{"Type": "Layer/Activation", "Function": f, "Alpha": a, "Beta": b}; `out` is
the Output layer's {"Scale": [...], "Shift": [...], "Transformation Mask": [...]}.
Values are kept per layer, layer 0 being the input, the Output layer last.
"""
import os
import sys

import numpy as np

f32, f64 = np.float32, np.float64


def widths(input_size, layers):
    w = [input_size]
    for ly in layers:
        w.append(int(ly["Output Channels"]) if ly["Type"] == "Layer/Linear" else w[-1])
    return w


def hyperparameter_count(input_size, layers):
    w = widths(input_size, layers)
    return sum(w[i] * w[i + 1] + w[i + 1] for i, ly in enumerate(layers) if ly["Type"] == "Layer/Linear")


def unpack(theta, input_size, layers):
    """{layer number: (W (OC x IC), b)} views of the flat vector, [W, b] per Linear layer"""
    w, k, out = widths(input_size, layers), 0, {}
    for i, ly in enumerate(layers):
        if ly["Type"] != "Layer/Linear":
            continue
        ic, oc = w[i], w[i + 1]
        out[i + 1] = (theta[k:k + ic * oc].reshape(oc, ic), theta[k + ic * oc:k + ic * oc + oc])
        k += ic * oc + oc
    return out


def initial_hyperparameters(input_size, layers, seed):
    """linear.cpp.base:28-49 with the network's Univariate/Uniform(-1, 1) generator (gsl_ran_flat on
    GSL's mt19937, seeded with `seed`); each layer's own "Weight Scaling" (default 1)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import refcpu as R

    rng = R.Rng(seed=seed)
    w, theta = widths(input_size, layers), []
    for i, ly in enumerate(layers):
        if ly["Type"] != "Layer/Linear":
            continue
        ic, oc = w[i], w[i + 1]
        xavier = f32(f64(np.sqrt(f32(6.0))) / np.sqrt(f64(oc + ic)))  # :36: float / sqrt(size_t) in double, rounded once
        scaled = f64(f32(ly.get("Weight Scaling", 1.0)) * xavier)  # float * float, then * double
        theta += [f32(scaled * rng.flat(-1.0, 1.0)) for _ in range(oc * ic)]
        theta += [f32(0.0)] * oc
    return np.asarray(theta, f32)


# ------------------------------------------------------------- activations
def activation(fn, x, alpha, beta, T):
    one, alpha, beta = T(1.0), T(alpha), T(beta)
    if fn == "Elementwise/Tanh":
        return np.tanh(x)
    if fn == "Elementwise/ReLU":
        return np.where(x > 0, x, x * alpha)
    if fn == "Elementwise/Logistic":
        return one / (one + np.exp(-x))
    if fn == "Elementwise/SoftReLU":
        return np.log(one + np.exp(x))
    if fn == "Elementwise/SoftSign":
        return x / (one + np.abs(x))
    if fn == "Elementwise/Linear":
        return x * alpha + beta
    if fn == "Elementwise/Log":
        return np.log(x)
    if fn == "Softmax":  # logSumExp, auxiliar/math.hpp:205-225
        mx = x.max(axis=1, keepdims=True)
        lse = mx + np.log(np.exp(x - mx).sum(axis=1, keepdims=True, dtype=T))
        return np.exp(x - lse)
    raise ValueError(fn)


def activation_backward(fn, g, y, z, alpha, T):
    """the reference's backward: the gradient with respect to the activation's input z from the one
    with respect to its value y.  Softmax: the diagonal term only; SoftSign: with the VALUE where the
    derivative has the input (both literal)"""
    one, alpha = T(1.0), T(alpha)
    if fn == "Elementwise/Tanh":
        return g * (one - y * y)
    if fn == "Elementwise/ReLU":
        return np.where(z > 0, g, g * alpha)
    if fn in ("Elementwise/Logistic", "Softmax"):
        return g * y * (one - y)
    if fn == "Elementwise/SoftReLU":
        e = np.exp(y)
        return g * (e - one) / e
    if fn == "Elementwise/SoftSign":
        return g / ((one + np.abs(y)) * (one + np.abs(y)))
    if fn == "Elementwise/Linear":
        return g * alpha
    if fn == "Elementwise/Log":
        return g / z
    raise ValueError(fn)


def _mask(out, n):
    m = (out or {}).get("Transformation Mask") or []
    return list(m) if len(m) else ["Identity"] * n


def output_forward(src, out, T):
    """output.cpp.base:141-162; float32 mode keeps the reference's double stages"""
    n = src.shape[1]
    x = np.array(src, T)
    for j, m in enumerate(_mask(out, n)):
        c = x[:, j]
        if m == "Absolute":
            c = np.abs(c)
        elif m == "Sigmoid":
            c = (1.0 / (1.0 + np.exp(-c).astype(f64))).astype(T)
        elif m == "Softplus":
            c = (0.5 * (c.astype(f64) + np.sqrt(1.0 + (c * c).astype(f64)))).astype(T)
        elif m == "Tanh":
            c = np.tanh(c)
        x[:, j] = c
    if out and len(out.get("Scale") or []):
        x = x * np.asarray(out["Scale"], T)
    if out and len(out.get("Shift") or []):
        x = x + np.asarray(out["Shift"], T)
    return x.astype(T)


def output_backward(G, outv, src, out, T):
    """output.cpp.base:175-212"""
    n = src.shape[1]
    x, g = np.array(outv, T), np.array(G, T)
    if out and len(out.get("Shift") or []):
        x = x - np.asarray(out["Shift"], T)
    if out and len(out.get("Scale") or []):
        s = np.asarray(out["Scale"], T)
        x, g = x / s, g * s
    for j, m in enumerate(_mask(out, n)):
        xc, gc = x[:, j], g[:, j]
        if m == "Absolute":
            gc = np.where(np.signbit(xc) != np.signbit(src[:, j]), -gc, gc)
        elif m == "Tanh":
            gc = gc * (T(1.0) - xc * xc)
        elif m == "Softplus":
            nnx = (xc.astype(f64) - 0.25 / xc.astype(f64)).astype(T)
            r = nnx / np.sqrt(nnx * nnx + T(1.0))
            gc = (gc.astype(f64) * 0.5 * (1.0 + r.astype(f64))).astype(T)
        elif m == "Sigmoid":
            gc = ((gc * xc).astype(f64) * (1.0 - xc.astype(f64))).astype(T)
        g[:, j] = gc
    return g.astype(T)


# ----------------------------------------------------------------- network
def forward(theta, X, input_size, layers, out=None, dtype=f32):
    """the values of every layer: [X, layer 1, ..., the Output layer's]"""
    T = dtype
    P = unpack(np.asarray(theta, T), input_size, layers)
    vals = [np.asarray(X, T).reshape(-1, input_size)]
    for i, ly in enumerate(layers):
        x = vals[-1]
        if ly["Type"] == "Layer/Linear":
            W, b = P[i + 1]
            vals.append(((x @ W.T).astype(T) + b).astype(T))
        else:
            vals.append(np.asarray(activation(ly["Function"], x, ly.get("Alpha", 1.0), ly.get("Beta", 0.0), T), T))
    vals.append(output_forward(vals[-1], out, T))
    return vals


def backward(theta, vals, G, input_size, layers, out=None, dtype=f32):
    """(the hyperparameter gradient, {layer: gradient with respect to its values})"""
    T = dtype
    theta = np.asarray(theta, T)
    P = unpack(theta, input_size, layers)
    grad = np.zeros_like(theta)
    GP = unpack(grad, input_size, layers)
    last = len(layers) + 1
    g = output_backward(G, vals[last], vals[last - 1], out, T)
    gl = {last - 1: g}
    for l in range(last - 1, 0, -1):
        ly = layers[l - 1]
        if ly["Type"] == "Layer/Linear":
            W, _ = P[l]
            GP[l][0][...] = (g.T @ vals[l - 1]).astype(T)
            GP[l][1][...] = np.add.accumulate(g, axis=0, dtype=T)[-1]  # linear.cpp.base:347-349: row after row
            g = (g @ W).astype(T)
        else:
            g = np.asarray(activation_backward(ly["Function"], g, vals[l], vals[l - 1], ly.get("Alpha", 1.0), T), T)
        gl[l - 1] = g
    return grad, gl


def mse_gradient(solution, output, dtype=f32):
    """deepSupervisor.cpp.base:124-136: (solution - output, sum g^2 / (2 N))"""
    T = dtype
    g = (np.asarray(solution, T) - np.asarray(output, T)).astype(T)
    s = np.add.accumulate((g * g).astype(T).ravel(), dtype=T)[-1]  # element after element
    return g, T(s / (T(g.shape[0]) * T(2.0)))


def l2_importance(value):
    """the generated parser reads "L2 Regularization"/"Importance" through get<int>()"""
    return float(int(value))


# -------------------------------------------------------------- optimizers
STATE = {"Adam": ("first_moment", "second_moment"), "AdaBelief": ("first_moment", "second_central_moment"),
         "MADGRAD": ("s", "v", "z"), "RMSProp": ("r", "v"), "Adagrad": ("s",)}


def new_state(name, n, dtype=f32):
    st = {k: np.zeros(n, dtype) for k in STATE[name]}
    st["count"] = 0
    st["beta1_pow"], st["beta2_pow"] = f32(1.0), f32(1.0)
    return st


def optimizer_step(name, theta, grad, st, eta, dtype=f32):
    """one processResult; returns the new hyperparameters and updates `st`.  The scalar factors
    (powers of beta, their reciprocals) are float32 in both modes: they are the step's inputs."""
    T = dtype
    th, g, eta, one = np.asarray(theta, T), np.asarray(grad, T), T(f32(eta)), T(1.0)
    b1, b2, eps = T(f32(0.9)), T(f32(0.999)), T(f32(1e-8))
    nb1, nb2 = T(f32(1.0) - f32(0.9)), T(f32(1.0) - f32(0.999))
    if name == "Adam":  # fAdam.cpp:64-90
        st["count"] += 1
        st["beta1_pow"], st["beta2_pow"] = f32(st["beta1_pow"] * f32(0.9)), f32(st["beta2_pow"] * f32(0.999))
        f1 = T(f32(1.0) / (f32(1.0) - st["beta1_pow"]))
        f2 = T(f32(1.0) / (f32(1.0) - st["beta2_pow"]))
        m = b1 * st["first_moment"] - nb1 * g
        v = b2 * st["second_moment"] + nb2 * g * g
        st["first_moment"], st["second_moment"] = m.astype(T), v.astype(T)
        return (th - eta / (np.sqrt(v * f2) + eps) * m * f1).astype(T)
    if name == "AdaBelief":  # fAdaBelief.cpp:25-52
        st["count"] += 1
        f2 = T(f32(1.0) / (f32(1.0) - np.power(f32(0.999), f32(st["count"]))))
        f1 = T(f32(1.0) / (f32(1.0) - np.power(f32(0.9), f32(st["count"]))))
        m = (b1 * st["first_moment"] - nb1 * g).astype(T)
        corrected, diff = m * f1, g + m
        c = (b2 * st["second_central_moment"] + nb2 * diff * diff).astype(T)
        st["first_moment"], st["second_central_moment"] = m, c
        return (th - eta / (np.sqrt(c * f2) + eps) * corrected).astype(T)
    if name == "MADGRAD":  # fMadGrad.cpp:54-73 (the optimizer's _initialValues are zeros)
        s = (st["s"] + eta * g).astype(T)
        v = (st["v"] - eta * (g * g)).astype(T)
        z = (T(0.0) - (one / (np.cbrt(v) + eps)) * s).astype(T)
        st["s"], st["v"], st["z"] = s, v, z
        st["count"] += 1
        return ((one - T(f32(0.9))) * th + T(f32(0.9)) * z).astype(T)
    if name == "RMSProp":  # fRMSProp.cpp:52-68
        decay = T(f32(0.999))
        r = ((one - decay) * (g * g) + decay * st["r"]).astype(T)
        v = ((eta / (np.sqrt(r) + eps)) * -g).astype(T)
        st["r"], st["v"] = r, v
        st["count"] += 1
        return (th - v).astype(T)
    if name == "Adagrad":  # fAdagrad.cpp:38-53
        s = (st["s"] + (g * g)).astype(T)
        st["s"] = s
        st["count"] += 1
        return (th + (eta / np.sqrt(s + eps)) * g).astype(T)
    raise ValueError(name)


def train(theta, X, S, input_size, layers, out=None, optimizer="Adam", eta=1e-3, steps=1, state=None, l2=None,
          dtype=f32):
    """DeepSupervisor::runGeneration's step loop with the Mean Squared Error loss; returns
    (hyperparameters, state, the last step's loss)"""
    T = dtype
    theta = np.asarray(theta, T)
    st = state if state is not None else new_state(optimizer, theta.size, T)
    loss = T(0.0)
    for _ in range(steps):
        vals = forward(theta, X, input_size, layers, out, T)
        g, loss = mse_gradient(S, vals[-1], T)
        grad, _ = backward(theta, vals, g, input_size, layers, out, T)
        if l2 is not None:
            grad = (grad - T(f32(l2)) * theta).astype(T)
        theta = optimizer_step(optimizer, theta, grad, st, eta, T)
    return theta, st, loss
