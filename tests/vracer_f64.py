"""Float64 reference of the VRACER policy update's stages with forward error
bounds for float32 arithmetic -- TEST INFRASTRUCTURE ONLY.

Each stage takes the float32 values the implementation under test read
(its own upstream results), recomputes the stage's output in float64 and
returns an `Err`: the float64 value and, per element, a bound on how far a
correct float32 evaluation may lie from it.  Nothing here is measured on any
implementation; the bounds follow from the standard model of IEEE float32,
fl(x op y) = (x op y)(1 + d), |d| <= u = 2^-24 (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., sections 2.2, 3.1, 4.2):

* a sum of K products in ANY order, every product and partial sum rounded
  (or fused, which rounds less often), differs from the exact sum by at most
  gamma_K sum_k |a_k| |b_k|, gamma_n = n u / (1 - n u).  Zero terms (the
  padding of a tile, of a lane's share) add nothing: 0 * x and s + 0 are
  exact.  Adding a bias is one more term: gamma_(K+1) (... + |bias|);
* every operation may flush a subnormal result to zero (the matrix units
  do): at most 2^-126 per operation;
* the epilogues' roundings are counted one by one by `Err`'s operations
  (running error analysis, second-order terms kept), each line noted below;
* tanhf is taken as accurate to 5 ulp, the bound of the OpenCL numerical
  compliance table that the device's math library follows; ulp(y) <= 2 u |y|.

`check` turns an observed array and an `Err` into err / bound ratios; a
correct implementation gives ratios <= 1 everywhere.
"""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
D = 2.0 ** -50  # a few float64 roundings, relative (the stages evaluated in double)


def gamma(n):
    return n * U / (1.0 - n * U)


class Err:
    """float64 value v and the bound e on |float32 evaluation - v|"""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, f64)
        self.e = np.broadcast_to(np.asarray(e, f64), self.v.shape)

    @property
    def T(self):
        return Err(self.v.T, self.e.T)


def _err(x):
    return x if isinstance(x, Err) else Err(np.asarray(x, f64))


def _rnd(v, e):
    """one float32 rounding of a result whose exact-arithmetic error is e"""
    return Err(v, e + U * (np.abs(v) + e) + TINY)


def add(a, b):
    a, b = _err(a), _err(b)
    return _rnd(a.v + b.v, a.e + b.e)


def sub(a, b):
    a, b = _err(a), _err(b)
    return _rnd(a.v - b.v, a.e + b.e)


def mul(a, b):
    a, b = _err(a), _err(b)
    return _rnd(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)


def div(a, b):
    a, b = _err(a), _err(b)
    den = np.abs(b.v) - b.e
    assert np.all(den > 0), "divisor not bounded away from zero"
    v = a.v / b.v
    return _rnd(v, (a.e + np.abs(v) * b.e) / den)


def sqrt(a):
    a = _err(a)
    assert np.all(a.v >= 0)
    v = np.sqrt(a.v)
    return _rnd(v, np.maximum(np.sqrt(a.v + a.e) - v, v - np.sqrt(np.maximum(a.v - a.e, 0.0))))


def dot(A, Bm, bias=None, dA=None):
    """sum_k A[m][k] Bm[k][n] (+ bias[n]) of float32 operands, any order.
    dA: A itself is only known to within dA (a float64 recomputation of a
    value that cannot be read): its bound times the absolute co-factor is
    added, and the rounding term uses |A| + dA."""
    A, Bm = np.asarray(A, f64), np.asarray(Bm, f64)
    K = A.shape[1]
    v = A @ Bm
    absA = np.abs(A) if dA is None else np.abs(A) + dA
    mag = absA @ np.abs(Bm)
    n = K
    if bias is not None:
        b = np.asarray(bias, f64)
        v, mag, n = v + b, mag + np.abs(b), K + 1
    e = gamma(n) * mag + n * TINY
    if dA is not None:
        e = e + np.asarray(dA, f64) @ np.abs(Bm)
    return Err(v, e)


def tanh5(z):
    """tanhf(z~) of a z~ within z.e of z.v: tanh is 1-Lipschitz, then 5 ulp of
    the result (which includes the rounding to float32)"""
    v = np.tanh(z.v)
    return Err(v, z.e + 10.0 * U * (np.abs(v) + z.e) + TINY)


def dtanh(y):
    """1 - y y in float32: two roundings; the error is absolute, about 2 u,
    however small the factor itself is"""
    return sub(1.0, mul(y, y))


# ------------------------------------------------------------------ stages
def hidden_layer(Aprev, W, b):
    """tanh(A W^T + b): the input layer (K = S, k_vr_fwd_in and its fused
    forms) and the hidden layers (K = H, EP_BIAS_TANH).  Roundings: the K + 1
    term sum, then tanhf."""
    return tanh5(dot(Aprev, np.asarray(W, f64).T, bias=b))


def output_layer(Alast, W, b, scale, shift, soft):
    """k_vr_fwd_out: the K + 1 term sum z; Softplus 0.5 (z + sqrt(1 + z^2)) in
    double (slope in (0, 1): the sum's error passes at most unchanged; the
    double roundings D) rounded to float32 once; then x * scale and + shift,
    one rounding each."""
    z = dot(Alast, np.asarray(W, f64).T, bias=b)
    sp = 0.5 * (z.v + np.sqrt(1.0 + z.v * z.v))
    spr = _rnd(sp, z.e + D * np.abs(sp))
    x = Err(np.where(soft, spr.v, z.v), np.where(soft, spr.e, z.e))
    return add(mul(x, np.asarray(scale, f64)), np.asarray(shift, f64))


def output_gradient(G, out, scale, shift, soft):
    """k_vr_bwd_out's dZ from loss_gradient and policy_output, elementwise:
    x = (out - shift) / scale (two roundings), g = G * scale (one); Softplus
    columns: nnx = x - 0.25 / x (two more), then g * 0.5 (1 + nnx / sqrt(nnx^2 + 1))
    in double (the factor's slope in nnx is at most 0.5), rounded once."""
    scale, shift = np.asarray(scale, f64), np.asarray(shift, f64)
    x = div(sub(np.asarray(out, f64), shift), scale)
    g = mul(np.asarray(G, f64), scale)
    xs = Err(np.where(soft, x.v, 1.0), np.where(soft, x.e, 0.0))  # (Softplus outputs are positive)
    nnx = sub(xs, div(0.25, xs))
    fv = 0.5 * (1.0 + nnx.v / np.sqrt(nnx.v * nnx.v + 1.0))
    fe = 0.5 * nnx.e + D
    v = g.v * fv
    gs = _rnd(v, np.abs(g.v) * fe + fv * g.e + g.e * fe + D * np.abs(v))
    return Err(np.where(soft, gs.v, g.v), np.where(soft, gs.e, g.e))


def hidden_gradient(Dl, W, a_prev, dD=None):
    """(sum_o Dl[b][o] W[o][i]) (1 - a^2): the last hidden layer's from dZ
    (K = O, k_vr_bwd_out) and EP_DTANH's (K = H).  Roundings: the K term sum,
    the factor's two, the product's one."""
    return mul(dot(Dl, W, dA=dD), dtanh(np.asarray(a_prev, f64)))


def weight_gradient(Dl, Aprev, dD=None):
    """dW[o][i] = sum_b Dl[b][o] A[b][i] and db[o] = sum_b Dl[b][o], K = B
    (k_vr_wgrad_small's lane sums and tree, EP_STORE with A column-major,
    k_vr_wgrad_adam).  db's B terms take the same gamma_B (no products)."""
    Dl = np.asarray(Dl, f64)
    dDT = None if dD is None else np.asarray(dD, f64).T
    return dot(Dl.T, Aprev, dA=dDT), dot(Dl.T, np.ones((Dl.shape[0], 1)), dA=dDT)


B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)


def adam(theta, grad, m1, m2, eta, b1p, b2p, l2imp=None):
    """vr_adam_elem (fAdam::processResult) from the float32 gradient,
    parameters, moments and the update's eta and beta powers; every operation
    of the source line is one `Err` operation, in its order.  l2imp: the L2
    term g - l2imp * theta first.  Returns (m, v, theta')."""
    th, g = np.asarray(theta, f64), _err(np.asarray(grad, f64))
    if l2imp is not None:
        g = sub(g, mul(f64(f32(l2imp)), th))
    f1 = div(1.0, sub(1.0, f64(b1p)))
    f2 = div(1.0, sub(1.0, f64(b2p)))
    omb1, omb2 = f64(f32(1.0) - B1), f64(f32(1.0) - B2)  # (exact in float32: Sterbenz)
    m = sub(mul(f64(B1), np.asarray(m1, f64)), mul(omb1, g))
    v = add(mul(f64(B2), np.asarray(m2, f64)), mul(mul(omb2, g), g))
    step = mul(mul(div(f64(eta), add(sqrt(mul(v, f2)), f64(EPS))), m), f1)
    return m, v, sub(th, step)


def check(got, ref):
    """err / bound per element (0 where both vanish, inf where the bound is 0
    and the value differs)"""
    got = np.asarray(got, f64)
    assert got.shape == ref.v.shape, (got.shape, ref.v.shape)
    err = np.abs(got - ref.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / ref.e)
    assert not np.any(np.isnan(r))
    return r


# -------------------------------------------------------- the whole update
def update_ratios(o):
    """Every stage check of one update.  `o` holds what the implementation
    under test read and wrote, float32, hidden width unpadded:
      S, A, H, L, B, scale, shift, soft;
      layers: [(W, b)] before the update; X (2B x S); acts: L arrays (2B x H);
      out (2B x O); G, dZ (B x O); dH: {layer: B x H} (a layer that cannot be
      read is left out: its float64 recomputation stands in, with its bound);
      grads: [(dW, db)]; and for Adam theta0, m0, v0, grad, m, v, theta (flat),
      eta, b1p, b2p, l2imp (None: no L2).
    Returns {stage: ratio array}."""
    L, B = o["L"], o["B"]
    layers, acts = o["layers"], o["acts"]
    r = {}
    r["input layer"] = check(acts[0], hidden_layer(o["X"], *layers[0]))
    for l in range(1, L):
        r[f"hidden forward {l}"] = check(acts[l], hidden_layer(acts[l - 1], *layers[l]))
    r["output layer"] = check(o["out"], output_layer(acts[L - 1], *layers[L], o["scale"], o["shift"], o["soft"]))
    r["dZ"] = check(o["dZ"], output_gradient(o["G"], o["out"][:B], o["scale"], o["shift"], o["soft"]))
    # backward on the B mini-batch rows; cur / dcur: layer l's gradient as read, or recomputed with its bound
    ref = hidden_gradient(o["dZ"], layers[L][0], acts[L - 1][:B])
    dW, db = weight_gradient(o["dZ"], acts[L - 1][:B])
    r["dW out"], r["db out"] = check(o["grads"][L][0], dW), check(o["grads"][L][1][:, None], db)
    for l in range(L - 1, -1, -1):
        if l in o["dH"]:
            r[f"dH {l}"] = check(o["dH"][l], ref)
            cur, dcur = o["dH"][l], None
        else:
            cur, dcur = ref.v, ref.e
        prev = acts[l - 1][:B] if l > 0 else o["X"][:B]
        dW, db = weight_gradient(cur, prev, dD=dcur)
        r[f"dW {l}"], r[f"db {l}"] = check(o["grads"][l][0], dW), check(o["grads"][l][1][:, None], db)
        if l > 0:
            ref = hidden_gradient(cur, layers[l][0], prev, dD=dcur)
    m, v, th = adam(o["theta0"], o["grad"], o["m0"], o["v0"], o["eta"], o["b1p"], o["b2p"], o["l2imp"])
    r["Adam m"], r["Adam v"], r["Adam theta"] = check(o["m"], m), check(o["v"], v), check(o["theta"], th)
    return r


def unpack(theta, S, H, L, A):
    """[(W (out x in), b)] per layer of a flat hyperparameter-shaped vector"""
    s = [S] + [H] * L + [1 + 2 * A]
    out, k = [], 0
    for i in range(len(s) - 1):
        ic, oc = s[i], s[i + 1]
        out.append((theta[k:k + ic * oc].reshape(oc, ic), theta[k + ic * oc:k + ic * oc + oc]))
        k += ic * oc + oc
    return out


def backward_f32(layers, acts, X, out, G, scale, shift, soft):
    """oracle/vracer_ref.py's `backward` with its intermediates kept: the same
    float32 NumPy operations in the same order (the CPU test asserts that the
    gradient equals vracer_ref.backward's bit for bit).  Returns (dZ,
    {layer: dH}, [(dW, db)])."""
    x = ((out - shift) / scale).astype(f32)
    g = (np.asarray(G, f32) * scale).astype(f32)
    nnx = (x - f32(0.25) / x).astype(f64)
    gs = (g.astype(f64) * 0.5 * (1.0 + nnx / np.sqrt(nnx * nnx + 1.0))).astype(f32)
    g = np.where(soft, gs, g).astype(f32)
    dZ, dH, grads = g, {}, [None] * len(layers)
    ins = [X] + list(acts)
    for li in range(len(layers) - 1, -1, -1):
        W, _ = layers[li]
        a = ins[li]
        grads[li] = ((g.T @ a).astype(f32), g.sum(axis=0, dtype=f32))
        if li > 0:
            g = ((g @ W) * (f32(1.0) - a * a)).astype(f32)
            dH[li - 1] = g
    return dZ, dH, grads


# (hidden, L, B, S, A, kind): each the smallest shape that reaches a branch of
# the update's kernels (tests/test_gpu_vracer_update_f64.py says which)
CASES = [
    (64, 1, 2, 4, 1, "cartpole"),
    (64, 2, 37, 4, 1, "cartpole"),
    (100, 2, 36, 4, 1, "clipped"),
    (320, 3, 260, 4, 1, "cartpole"),
    (64, 2, 64, 12, 2, "host"),
    (100, 2, 37, 3, 2, "host_l2"),
]
L2_IMPORTANCE = 1e-2
