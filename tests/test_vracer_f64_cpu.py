"""tests/vracer_f64.py checked on the CPU: at every shape of the GPU test the
oracle's float32 NumPy restatement (oracle/vracer_ref.py forward / backward /
Adam.step) lies within every stage's bound, and three subtly wrong variants
of it (a dropped k-term, a dropped batch row, an omitted (1 - y^2) factor)
leave the bound on at least half of the elements they touch."""
import numpy as np
import pytest

import vracer_f64 as F
import vracer_ref as V

f32 = np.float32
NOISE = 0.7


def restatement(H, L, B, S, A, kind, seed=5):
    """One update's values as the float32 restatement forms them, in the
    layout of vracer_f64.update_ratios."""
    rng = np.random.default_rng(seed)
    n = V.hyperparameter_count(S, H, L, A)
    theta = (V.initial_hyperparameters(S, H, L, A, rng.uniform(-1, 1, n), output_scaling=1.0)
             + 0.15 * rng.standard_normal(n) / np.sqrt(H)).astype(f32)
    shift = np.full(A, 0.25, f32) if kind == "clipped" else None
    scale, sh, soft = V.output_transform(A, NOISE, shift)
    X = rng.uniform(-1, 1, (2 * B, S)).astype(f32)
    out, acts = V.forward(theta, X, S, H, L, A, NOISE, shift)
    G = (rng.standard_normal((B, 1 + 2 * A)) * 0.5).astype(f32)
    layers = F.unpack(theta, S, H, L, A)
    dZ, dH, grads = F.backward_f32(layers, [a[:B] for a in acts[1:]], X[:B], out[:B], G, scale, sh, soft)
    grad = np.concatenate([np.concatenate([w.ravel(), b]) for w, b in grads]).astype(f32)
    ref = V.backward(theta, [a[:B] for a in acts], out[:B], G, S, H, L, A, NOISE, shift)
    assert np.array_equal(grad, ref)  # backward_f32 is vracer_ref.backward with its intermediates kept
    l2 = F.L2_IMPORTANCE if kind == "host_l2" else None
    ad = V.Adam(n)
    ad.m = (1e-2 * rng.standard_normal(n)).astype(f32)
    ad.v = (1e-4 * rng.uniform(0, 1, n)).astype(f32)
    ad.b1p, ad.b2p, ad.eta = f32(0.9) * f32(0.9), f32(0.999) * f32(0.999), f32(1e-4)
    m0, v0 = ad.m.copy(), ad.v.copy()
    theta1 = ad.step(theta, grad if l2 is None else (grad - f32(l2) * theta).astype(f32))
    return dict(S=S, A=A, H=H, L=L, B=B, scale=scale, shift=sh, soft=soft, layers=layers, X=X, acts=acts[1:],
                out=out, G=G, dZ=dZ, dH=dH, grads=grads, theta0=theta, m0=m0, v0=v0, grad=grad, m=ad.m, v=ad.v,
                theta=theta1, eta=ad.eta, b1p=ad.b1p, b2p=ad.b2p, l2imp=l2)


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: "-".join(map(str, c)))
def test_float32_restatement_lies_within_every_bound(case):
    o = restatement(*case)
    ratios = F.update_ratios(o)
    worst = {k: float(r.max()) for k, r in ratios.items()}
    print(f"restatement {case}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert set(worst) >= {"input layer", "output layer", "dZ", "dW out", "dW 0", "db 0", "Adam theta"}
    assert all(f"dH {l}" in worst for l in range(case[1]))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
    # with the last hidden layer's gradient unreadable (the device at L = 3)
    # its recomputation stands in, and the stages after it still hold
    if case[1] >= 2:
        del o["dH"][case[1] - 1]
        for k, r in F.update_ratios(o).items():
            assert r.max() <= 1.0, (k, float(r.max()))


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: "-".join(map(str, c)))
def test_mutants_leave_the_bound(case):
    """Each mutant changes one stage of the restatement; the share of the
    touched elements outside the bound must be at least one half."""
    H, L, B, S, A, _ = case
    o = restatement(*case)
    ins = [o["X"]] + list(o["acts"])
    share = {}
    # 1. the last k-term dropped in the deepest tanh layer's sum
    l = L - 1
    W, b = o["layers"][l]
    mut = np.tanh((ins[l][:, :-1] @ W[:, :-1].T + b).astype(f32)).astype(f32)
    share["k-term"] = np.mean(F.check(mut, F.hidden_layer(ins[l], W, b)) > 1.0)
    # 2. the last batch row dropped in that layer's weight gradient
    g, a = o["dH"][l], ins[l][:B]
    mut = (g[:-1].T @ a[:-1]).astype(f32)
    share["batch row"] = np.mean(F.check(mut, F.weight_gradient(g, a)[0]) > 1.0)
    # 3. (1 - y^2) omitted on one column of the last hidden layer's gradient
    WL = o["layers"][L][0]
    y = ins[L][:B]
    mut = (o["dZ"] @ WL[:, :1]).astype(f32)
    ref = F.hidden_gradient(o["dZ"], WL, y)
    share["1 - y^2"] = np.mean(F.check(mut, F.Err(ref.v[:, :1], ref.e[:, :1])) > 1.0)
    print(f"mutants {case}: " + ", ".join(f"{k} {v:.2f}" for k, v in share.items()))
    for k, v in share.items():
        assert v >= 0.5, (k, v)
