"""The DeepSupervisor device kernels (korali_amd/csrc/kg_supervisor.hip), stage
by stage against float64 inside derived forward-error bounds.

Teacher-forced like tests/test_gpu_vracer_update_f64.py: every stage is
recomputed in float64 from the float32 values the device itself read (its
own upstream results, read back through kg_supervisor_get_field), and the
device's result must lie within the bound of tests/vracer_f64.py's model:
gamma_K sum |a||b| for the products (any summation order), one counted
rounding per elementwise operation, and for the math library the ulp bounds
of the OpenCL numerical compliance table that file cites (exp 3, log 3,
tanh 5, cbrt 2, pow 16 ulp; ulp(y) <= 2 u |y|).  Nothing here is measured.

A training step cannot be stopped half way, so its gradient is obtained
beforehand from the same state with forward + backward_direct: the kernels
are deterministic, the step recomputes the same bits (asserted).
"""
import numpy as np
import pytest

import supervisor_ref as SR
import vracer_f64 as F

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
U, TINY, Err = F.U, F.TINY, F.Err


def lin(n, ws=1.0):
    return {"Type": "Layer/Linear", "Output Channels": n, "Weight Scaling": ws}


def act(fn, alpha=1.0, beta=0.0):
    return {"Type": "Layer/Activation", "Function": fn, "Alpha": alpha, "Beta": beta}


# ------------------------------------------------------------ error model
def exp3(a):
    a = F._err(a)
    v = np.exp(a.v)
    hi = v * np.exp(a.e)
    return Err(v, (hi - v) + 6.0 * U * hi + TINY)


def log3(a):
    a = F._err(a)
    assert np.all(a.v - a.e > 0)
    v = np.log(a.v)
    d = np.log1p(a.e / (a.v - a.e))
    return Err(v, d + 6.0 * U * (np.abs(v) + d) + TINY)


def cbrt2(a):
    a = F._err(a)
    v = np.cbrt(a.v)
    d = np.maximum(np.cbrt(a.v + a.e) - v, v - np.cbrt(a.v - a.e))
    return Err(v, d + 4.0 * U * (np.abs(v) + d) + TINY)


def absE(a):
    a = F._err(a)
    return Err(np.abs(a.v), a.e)


def where(c, a, b):
    a, b = F._err(a), F._err(b)
    return Err(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def act_fwd(fn, z, alpha, beta):
    """activation.cpp.base:147-209 of the float32 values z, operation by operation"""
    z = np.asarray(z, f64)
    if fn == "Elementwise/Tanh":
        return F.tanh5(Err(z))
    if fn == "Elementwise/ReLU":
        return where(z > 0, Err(z), F.mul(z, f64(f32(alpha))))
    if fn == "Elementwise/Logistic":
        return F.div(1.0, F.add(1.0, exp3(Err(-z))))
    if fn == "Elementwise/SoftReLU":
        return log3(F.add(1.0, exp3(Err(z))))
    if fn == "Elementwise/SoftSign":
        return F.div(z, F.add(1.0, np.abs(z)))
    if fn == "Elementwise/Linear":
        return F.add(F.mul(z, f64(f32(alpha))), f64(f32(beta)))
    if fn == "Elementwise/Log":
        return log3(Err(z))
    if fn == "Softmax":  # max exact; n-term sum in any order; log; two subtractions; exp
        mx = z.max(axis=1, keepdims=True)
        e = exp3(F.sub(z, mx))
        n = z.shape[1]
        s = Err(e.v.sum(axis=1, keepdims=True), (e.e.sum(axis=1, keepdims=True) + F.gamma(n) * (e.v + e.e).sum(axis=1, keepdims=True)))
        return exp3(F.sub(z, F.add(mx, log3(s))))
    raise ValueError(fn)


def act_bwd(fn, g, y, z, alpha):
    """activation.cpp.base:270-314; g may carry a bound (the product in front of it)"""
    y, z = np.asarray(y, f64), np.asarray(z, f64)
    if fn == "Elementwise/Tanh":
        return F.mul(g, F.sub(1.0, F.mul(y, y)))
    if fn == "Elementwise/ReLU":
        return where(z > 0, g, F.mul(g, f64(f32(alpha))))
    if fn in ("Elementwise/Logistic", "Softmax"):
        return F.mul(F.mul(g, y), F.sub(1.0, y))
    if fn == "Elementwise/SoftReLU":
        e = exp3(Err(y))
        return F.div(F.mul(g, F.sub(e, 1.0)), e)
    if fn == "Elementwise/SoftSign":
        a = F.add(1.0, np.abs(y))
        return F.div(g, F.mul(a, a))
    if fn == "Elementwise/Linear":
        return F.mul(g, f64(f32(alpha)))
    if fn == "Elementwise/Log":
        return F.div(g, z)
    raise ValueError(fn)


def _cols(out, n):
    m = (out or {}).get("Transformation Mask") or ["Identity"] * n
    sc = np.asarray(out["Scale"], f32).astype(f64) if out and len(out.get("Scale") or []) else None
    sh = np.asarray(out["Shift"], f32).astype(f64) if out and len(out.get("Shift") or []) else None
    return np.asarray(m), sc, sh


def out_fwd(src, out):
    """output.cpp.base:141-162: float roundings counted, the double stages as D"""
    src = np.asarray(src, f64)
    m, sc, sh = _cols(out, src.shape[1])
    e = exp3(Err(-src))
    sg = F._rnd(1.0 / (1.0 + e.v), e.e + F.D)  # |d/de 1 / (1 + e)| <= 1
    xx = F.mul(src, src)
    spv = 0.5 * (src + np.sqrt(1.0 + xx.v))
    sp = F._rnd(spv, 0.25 * xx.e + F.D * np.abs(spv))  # slope in xx: 1 / (4 sqrt(1 + xx)) <= 1/4
    x = where(m == "Sigmoid", sg, where(m == "Softplus", sp, where(m == "Tanh", F.tanh5(Err(src)),
              where(m == "Absolute", Err(np.abs(src)), Err(src)))))
    if sc is not None:
        x = F.mul(x, sc)
    if sh is not None:
        x = F.add(x, sh)
    return x


def out_bwd(G, outv, src, out):
    """output.cpp.base:175-212"""
    outv, src = np.asarray(outv, f64), np.asarray(src, f64)
    m, sc, sh = _cols(out, src.shape[1])
    x, g = Err(outv), Err(np.asarray(G, f64))
    if sh is not None:
        x = F.sub(x, sh)
    if sc is not None:
        x, g = F.div(x, sc), F.mul(g, sc)
    flip = np.signbit(x.v) != np.signbit(src)
    assert np.all(np.abs(x.v[:, m == "Absolute"]) > 4 * x.e[:, m == "Absolute"]), "Absolute column too close to 0"
    ab = Err(np.where(flip, -g.v, g.v), g.e)
    th = F.mul(g, F.sub(1.0, F.mul(x, x)))
    xs = where(m == "Softplus", x, Err(np.ones_like(x.v)))
    nv = xs.v - 0.25 / xs.v
    nnx = F._rnd(nv, xs.e * (1.0 + 0.25 / (np.abs(xs.v) - xs.e) ** 2) + F.D * np.abs(nv))
    r = F.div(nnx, F.sqrt(F.add(F.mul(nnx, nnx), 1.0)))
    pv = g.v * 0.5 * (1.0 + r.v)
    sp = F._rnd(pv, 0.5 * (np.abs(g.v) + g.e) * r.e + 0.5 * (1.0 + np.abs(r.v)) * g.e + F.D * np.abs(pv))
    gx = F.mul(g, x)
    sv = gx.v * (1.0 - x.v)
    sg = F._rnd(sv, (np.abs(gx.v) + gx.e) * x.e + np.abs(1.0 - x.v) * gx.e + F.D * np.abs(sv))
    return where(m == "Sigmoid", sg, where(m == "Softplus", sp, where(m == "Tanh", th, where(m == "Absolute", ab, g))))


def assert_within(name, got, ref):
    r = F.check(got, ref)
    assert r.max(initial=0.0) <= 1.0, f"{name}: err / bound = {r.max():.3g} at {np.unravel_index(r.argmax(), r.shape)}"


# ------------------------------------------------------------ the walk
def device(I, layers, O, B, NI=None, out=None, **kw):
    from korali_amd.supervisor import SupervisorDevice

    out = out or {}
    return SupervisorDevice(I, O, layers, B, NI, output_scale=out.get("Scale"), output_shift=out.get("Shift"),
                            output_mask=out.get("Transformation Mask"), **kw)


def draw_theta(I, layers, rng, positive=False):
    th = rng.uniform(-1, 1, SR.hyperparameter_count(I, layers)).astype(f32)
    w = SR.widths(I, layers)
    for l, (W, b) in SR.unpack(th, I, layers).items():
        W *= f32(np.sqrt(3.0 / w[l - 1]))  # unit-variance pre-activations
    return np.abs(th) if positive else th


def check_pass(dev, I, layers, O, B, theta, X, G=None, out=None, field="output"):
    """forward of X (B rows) and backward of G (default: none) on `dev`, every stage within its bound.
    Returns (the layers' values, the hyperparameter gradient) as the device holds them.
    field="inference_output": B is the inference batch size, the values are the second pipeline's."""
    last = len(layers) + 1
    dev.set("hyperparameters", theta)
    P = SR.unpack(np.asarray(theta, f32), I, layers)
    w = SR.widths(I, layers) + [O]
    res = dev.forward(X)
    vals = [dev.get(f"{field}:{l}").reshape(B, w[l]) for l in range(last + 1)]
    assert np.array_equal(vals[0], np.asarray(X, f32).reshape(B, I)) and np.array_equal(vals[last], res)
    for l in range(1, last):
        ly = layers[l - 1]
        if ly["Type"] == "Layer/Linear":
            ref = F.dot(vals[l - 1], P[l][0].astype(f64).T, bias=P[l][1])
        else:
            ref = act_fwd(ly["Function"], vals[l - 1], ly["Alpha"], ly["Beta"])
        assert_within(f"forward, layer {l} ({ly.get('Function', 'Linear')})", vals[l], ref)
    assert_within("Output layer forward", vals[last], out_fwd(vals[last - 1], out))
    if G is None:
        return vals, None
    dev.backward_direct(G)
    grad = dev.get("gradient")
    GP = SR.unpack(grad, I, layers)
    gl = lambda l: dev.get(f"output_gradient:{l}").reshape(B, w[l])
    cur = gl(last - 1)
    assert_within("Output layer backward", cur, out_bwd(G, vals[last], vals[last - 1], out))
    l = last - 1
    while l >= 1:
        ly = layers[l - 1]
        if ly["Type"] == "Layer/Activation":
            if l - 1 == 0:
                break
            ref = act_bwd(ly["Function"], Err(cur), vals[l], vals[l - 1], ly["Alpha"])
            cur = gl(l - 1)
            assert_within(f"backward, layer {l} ({ly['Function']})", cur, ref)
            l -= 1
            continue
        dW, db = F.weight_gradient(cur, vals[l - 1])
        assert_within(f"weight gradient, layer {l}", GP[l][0], dW)
        assert_within(f"bias gradient, layer {l}", GP[l][1][:, None], db)
        if l - 1 == 0:
            break
        d = F.dot(cur, P[l][0])
        pv = layers[l - 2]
        if pv["Type"] == "Layer/Activation" and pv["Function"] != "Softmax":
            if l - 2 == 0:
                break
            ref = act_bwd(pv["Function"], d, vals[l - 1], vals[l - 2], pv["Alpha"])
            cur = gl(l - 2)
            assert_within(f"data gradient, layer {l}, with {pv['Function']}'s derivative", cur, ref)
            l -= 2
        else:
            cur = gl(l - 1)
            assert_within(f"data gradient, layer {l}", cur, d)
            l -= 1
    return vals, grad


def run_case(I, hidden, O, B, seed=0, out=None, positive=False, output_activation=None):
    layers = list(hidden) + [lin(O)] + ([act(output_activation)] if output_activation else [])
    rng = np.random.default_rng(seed)
    theta = draw_theta(I, layers, rng, positive)
    X = (rng.uniform(0.1, 1, (B, I)) if positive else rng.standard_normal((B, I))).astype(f32)
    G = rng.standard_normal((B, O)).astype(f32)
    dev = device(I, layers, O, B, out=out)
    try:
        check_pass(dev, I, layers, O, B, theta, X, G, out)
        return dev
    except BaseException:
        dev.close()
        raise


# ------------------------------------------------------------- products
def test_every_dimension_one():
    run_case(1, [lin(1), act("Elementwise/Tanh"), lin(1), act("Elementwise/Tanh")], 1, 1).close()


@pytest.mark.parametrize("B", [127, 128, 129])
def test_tile_edges(B):
    """widths 127 -> 128 -> 129 -> 127 -> 128: every dimension of the three products one below, at and
    one above the 128 tile; K = 127, 129 are no multiples of the k-step 16"""
    dev = run_case(127, [lin(128), act("Elementwise/Tanh"), lin(129), act("Elementwise/Tanh"), lin(127),
                         act("Elementwise/Tanh")], 128, B, seed=B)
    assert dev.scalar("tile") == 128 and dev.scalar("k_step") == 16
    dev.close()


def test_aligned_multi_tile():
    """every stride and offset a multiple of four floats: the float4 loads; 2 x 2 tiles"""
    run_case(128, [lin(256), act("Elementwise/Tanh")], 128, 256).close()


def test_aligned_k_132_falls_back_inside_a_tile():
    """every width and the batch 132: aligned strides and bases, so the full tiles load as float4 for
    k < 128 and element by element for the last 4 (all three products); the second tiles are edges"""
    run_case(132, [lin(132), act("Elementwise/Tanh"), lin(132), act("Elementwise/Tanh")], 132, 132).close()


def test_aligned_weight_gradient_split():
    """128-wide layers, a batch of 520: the weight gradients run the float4 path in three slabs of 176,
    176 and 168 rows (k starting at 176 and 352; the last slab ends in a half step)"""
    dev = run_case(128, [lin(128), act("Elementwise/Tanh")], 128, 520)
    for l in (1, 3):
        s, c = int(dev.scalar(f"weight_gradient_splits:{l}")), int(dev.scalar(f"weight_gradient_chunk:{l}"))
        assert (s, c) == (3, 176)
    dev.close()


def test_inference_pipeline():
    """the second pipeline (Inference Batch Size rows) against the same bounds, and apart from the
    training pipeline's values"""
    I, O, B, NI = 5, 3, 9, 130
    layers = [lin(7), act("Elementwise/Tanh"), lin(6), act("Softmax"), lin(O), act("Elementwise/Logistic")]
    out = {"Scale": [2.0, 0.5, 1.5], "Shift": [0.25, -1.0, 0.0], "Transformation Mask": ["Softplus", "Identity", "Tanh"]}
    rng = np.random.default_rng(5)
    theta = draw_theta(I, layers, rng)
    X, Xi = rng.standard_normal((B, I)).astype(f32), rng.standard_normal((NI, I)).astype(f32)
    dev = device(I, layers, O, B, NI=NI, out=out)
    tv, _ = check_pass(dev, I, layers, O, B, theta, X, out=out)
    iv, _ = check_pass(dev, I, layers, O, NI, theta, Xi, out=out, field="inference_output")
    again = [dev.get(f"output:{l}") for l in range(len(layers) + 2)]
    assert all(np.array_equal(a.ravel(), b) for a, b in zip(tv, again)), "the inference pass wrote into the training pipeline"
    assert iv[-1].shape == (NI, O)
    dev.close()


def test_weight_gradient_uneven_split():
    """a batch of 600 over small layers: three slabs of 208, 208 and 184 rows"""
    dev = run_case(3, [lin(5), act("Elementwise/Tanh")], 2, 600)
    for l in (1, 3):
        s, c = int(dev.scalar(f"weight_gradient_splits:{l}")), int(dev.scalar(f"weight_gradient_chunk:{l}"))
        assert s > 1 and 600 % c != 0 and (s - 1) * c < 600 <= s * c and c % 16 == 0
    dev.close()


@pytest.mark.parametrize("width", [1, 70])
def test_softmax_rows(width):
    run_case(6, [lin(width), act("Softmax"), lin(4), act("Elementwise/Tanh")], width, 9, output_activation="Softmax").close()


# ------------------------------------- activations, masks, optimizers, losses
ACTIVATIONS = [("Elementwise/Tanh", 1.0, 0.0), ("Elementwise/ReLU", 0.1, 0.0), ("Elementwise/Logistic", 1.0, 0.0),
               ("Elementwise/SoftReLU", 1.0, 0.0), ("Elementwise/SoftSign", 1.0, 0.0), ("Elementwise/Linear", 0.7, 0.3),
               ("Elementwise/Log", 1.0, 0.0), ("Softmax", 1.0, 0.0)]


@pytest.mark.parametrize("fn,alpha,beta", ACTIVATIONS)
def test_activation(fn, alpha, beta):
    """fused behind a Linear layer (forward and, one layer down, backward) and alone as the output activation"""
    layers = [lin(7), act(fn, alpha, beta), lin(6), act(fn, alpha, beta), lin(3), act(fn, alpha, beta)]
    rng = np.random.default_rng(1)
    positive = fn == "Elementwise/Log"
    theta = draw_theta(5, layers, rng, positive)
    if positive:  # keep every Linear layer's values positive: log of them, then positive weights again
        for W, b in SR.unpack(theta, 5, layers).values():
            b += f32(3.0)
    X = (rng.uniform(0.1, 1, (9, 5)) if positive else rng.standard_normal((9, 5))).astype(f32)
    dev = device(5, layers, 3, 9)
    check_pass(dev, 5, layers, 3, 9, theta, X, rng.standard_normal((9, 3)).astype(f32))
    dev.close()


@pytest.mark.parametrize("mask", ["Identity", "Absolute", "Softplus", "Tanh", "Sigmoid"])
def test_output_mask(mask):
    out = {"Scale": [2.0, 0.5, 1.5], "Shift": [0.25, -1.0, 0.0], "Transformation Mask": [mask, "Identity", mask]}
    run_case(4, [lin(6), act("Elementwise/Tanh")], 3, 11, seed=3, out=out).close()


def _opt_err(name, th, g, st, eta, dev, l2=None):
    """processResult of the float32 inputs, operation by operation -> {field: Err}, 'theta'"""
    th, g = np.asarray(th, f64), Err(np.asarray(g, f64))
    eta, eps = f64(f32(eta)), f64(f32(1e-8))
    if l2 is not None:
        g = F.sub(g, F.mul(f64(f32(l2)), th))
    if name == "Adam":
        m, v, t = F.adam(th, g.v, st["first_moment"], st["second_moment"], eta, f32(dev.scalar("beta1_pow")),
                         f32(dev.scalar("beta2_pow")), None)
        assert l2 is None
        return {"first_moment": m, "second_moment": v, "theta": t}
    b1, b2 = f64(f32(0.9)), f64(f32(0.999))
    nb1, nb2 = f64(f32(1.0) - f32(0.9)), f64(f32(1.0) - f32(0.999))
    if name == "AdaBelief":
        n = dev.scalar("model_evaluation_count")
        pw = lambda b: Err(b ** n, 32.0 * U * b ** n)  # powf: 16 ulp
        f2, f1 = F.div(1.0, F.sub(1.0, pw(b2))), F.div(1.0, F.sub(1.0, pw(b1)))
        m = F.sub(F.mul(b1, st["first_moment"].astype(f64)), F.mul(nb1, g))
        corrected, diff = F.mul(m, f1), F.add(g, m)
        c = F.add(F.mul(b2, st["second_central_moment"].astype(f64)), F.mul(F.mul(nb2, diff), diff))
        t = F.sub(th, F.mul(F.div(eta, F.add(F.sqrt(F.mul(c, f2)), eps)), corrected))
        return {"first_moment": m, "second_central_moment": c, "theta": t}
    if name == "MADGRAD":
        s = F.add(st["s"].astype(f64), F.mul(eta, g))
        v = F.sub(st["v"].astype(f64), F.mul(eta, F.mul(g, g)))
        z = F.sub(0.0, F.mul(F.div(1.0, F.add(cbrt2(v), eps)), s))
        mom = f64(f32(0.9))
        t = F.add(F.mul(f64(f32(1.0) - f32(0.9)), th), F.mul(mom, z))
        return {"s": s, "v": v, "z": z, "theta": t}
    if name == "RMSProp":
        d = f64(f32(0.999))
        r = F.add(F.mul(f64(f32(1.0) - f32(0.999)), F.mul(g, g)), F.mul(d, st["r"].astype(f64)))
        v = F.mul(F.div(eta, F.add(F.sqrt(r), eps)), Err(-g.v, g.e))
        return {"r": r, "v": v, "theta": F.sub(th, v)}
    s = F.add(st["s"].astype(f64), F.mul(g, g))
    return {"s": s, "theta": F.add(th, F.mul(F.div(eta, F.sqrt(F.add(s, eps))), g))}


@pytest.mark.parametrize("name,l2", [("Adam", None), ("AdaBelief", None), ("MADGRAD", None), ("RMSProp", 2.0),
                                     ("Adagrad", None)])
def test_optimizer_step(name, l2):
    """one Mean Squared Error step from a state in mid-training: the loss, the L2 term, the optimizer"""
    I, O, B = 4, 2, 13
    layers = [lin(6), act("Elementwise/Tanh"), lin(O)]
    rng = np.random.default_rng(7)
    theta = draw_theta(I, layers, rng)
    X, S = rng.standard_normal((B, I)).astype(f32), rng.standard_normal((B, O)).astype(f32)
    eta = 0.01
    dev = device(I, layers, O, B, optimizer=name, learning_rate=eta, l2_enabled=l2 is not None,
                 l2_importance=0.0 if l2 is None else SR.l2_importance(l2 + 0.7))
    st = {}
    for k in SR.STATE[name]:
        st[k] = (rng.uniform(0.01, 0.1, theta.size) * (-1.0 if name == "MADGRAD" and k == "v" else 1.0)).astype(f32)
        dev.set(k, st[k])
    if name in ("Adam", "AdaBelief"):
        dev.set_scalar("beta1_pow", f32(0.9) ** 3), dev.set_scalar("beta2_pow", f32(0.999) ** 3)
        dev.set_scalar("model_evaluation_count", 3)
    dev.set_training_data(X, S)
    vals, _ = check_pass(dev, I, layers, O, B, theta, X)
    G = (S - vals[-1]).astype(f32)  # one IEEE subtraction: the device's bits
    dev.backward_direct(G)
    grad = dev.get("gradient")
    loss = dev.train(1)
    n = G.size
    lref = F.div(F.dot(G.reshape(1, n), G.reshape(n, 1).astype(f64)), f64(B) * 2.0)
    assert_within("loss", np.asarray([[loss]]), lref)
    ref = _opt_err(name, theta, grad, st, eta, dev, l2)
    if l2 is not None:
        assert_within("gradient with the L2 term", dev.get("gradient"), F.sub(grad.astype(f64), F.mul(f64(f32(l2)), theta.astype(f64))))
    else:
        assert np.array_equal(dev.get("gradient"), grad), "the step's gradient differs from backward_direct's"
    for k in SR.STATE[name]:
        assert_within(f"{name} {k}", dev.get(k), ref[k])
    assert_within(f"{name} hyperparameters", dev.hyperparameters, ref["theta"])
    assert not np.array_equal(dev.hyperparameters, theta)
    dev.close()


def test_direct_gradient():
    from korali_amd.supervisor import KoraliDeviceError

    I, O, B = 4, 2, 13
    layers = [lin(6), act("Elementwise/Tanh"), lin(O)]
    rng = np.random.default_rng(9)
    theta = draw_theta(I, layers, rng)
    X, S = rng.standard_normal((B, I)).astype(f32), rng.standard_normal((B, O)).astype(f32)
    dev = device(I, layers, O, B, NI=5, loss="Direct Gradient", learning_rate=0.01)
    dev.set_training_data(X, S)
    dev.set("hyperparameters", theta)
    with pytest.raises(KoraliDeviceError, match="no forward pass"):
        dev.train(1)
    dev.forward(X[:5])  # the inference batch size: still no pass of Training Batch Size rows
    with pytest.raises(KoraliDeviceError, match="no forward pass"):
        dev.train(1)
    with pytest.raises(KoraliDeviceError, match=r"Batch size \(4\) of input is not within the configured batch sizes"):
        dev.forward(X[:4])
    _, grad = check_pass(dev, I, layers, O, B, theta, X, S)
    dev.train(1)
    assert np.array_equal(dev.get("gradient"), grad)
    m, _, t = F.adam(theta, grad, np.zeros_like(theta), np.zeros_like(theta), f64(f32(0.01)), f32(0.9), f32(0.999), None)
    assert_within("first step", dev.hyperparameters, t)
    dev.close()


def test_fifty_steps_twice_are_identical():
    I, O, B = 3, 2, 300
    layers = [lin(40), act("Elementwise/Tanh"), lin(33), act("Elementwise/ReLU", 0.1), lin(O)]
    rng = np.random.default_rng(11)
    theta = draw_theta(I, layers, rng)
    X, S = rng.standard_normal((B, I)).astype(f32), rng.standard_normal((B, O)).astype(f32)
    res = []
    for _ in range(2):
        dev = device(I, layers, O, B, learning_rate=0.01, hyperparameters=theta)
        dev.set_training_data(X, S)
        loss = dev.train(50)
        res.append((dev.hyperparameters, loss))
        dev.close()
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    assert np.all(np.isfinite(res[0][0])) and not np.array_equal(res[0][0], theta)
