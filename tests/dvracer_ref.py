"""dVRACER restatement — TEST INFRASTRUCTURE ONLY.

A NumPy float32 restatement of the reference's discrete agent
(`Agent / Discrete / dVRACER`), the checker of the discrete handles of
korali_amd/csrc/kg_vracer.hip.  It reuses oracle/vracer_ref.py for everything
the two agents share (the `Agent` bookkeeping of agent.cpp.base, philox, the
CartPole, fAdam) and restates what differs (paths relative to the korali
root's source/modules):

* the network's output: V, K Q-values, the inverse temperature; Identity x
  (1 + K), Sigmoid; scale 1, shift 0; output weight scaling 0.001
  (solver/agent/discrete/dVRACER/dVRACER.cpp.base:21-51); the Sigmoid of
  neuralNetwork/layer/output/output.cpp.base:149 (forward) and :208-209
  (backward);
* dVRACER::runPolicy (dVRACER.cpp.base:156-222): the softmax with the maximum
  subtracted, the float sum in index order, p_i = e_i * (1 / sum);
* Discrete::getAction (solver/agent/discrete/discrete.cpp.base:15-78): the
  categorical walk (training) and the first maximum (testing);
* calculateImportanceWeight (:80-95), calculateImportanceWeightGradient
  (:97-132), calculateKLDivergenceGradient (:134-163) in the written
  precision (`1.` / `1.0` literals promote a product to double; `klGrad[i] -=`
  rounds per term);
* dVRACER::calculatePolicyGradients (dVRACER.cpp.base:83-154).

The uniform of an action comes from philox4x32-10 (one block per environment
and step, purpose tag 0x4441) instead of GSL's stream, a deviation by design
like the action noise of the continuous agent.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import vracer_ref as V  # noqa: E402

f32 = np.float32
f64 = np.float64
NON_TERMINAL, TERMINAL, TRUNCATED = V.NON_TERMINAL, V.TERMINAL, V.TRUNCATED


# ----------------------------------------------------------------- network
def layer_sizes(S, H, L, K):
    return [S] + [H] * L + [2 + K]


def hyperparameter_count(S, H, L, K):
    s = layer_sizes(S, H, L, K)
    return sum(s[i] * s[i + 1] + s[i + 1] for i in range(len(s) - 1))


def initial_hyperparameters(S, H, L, K, uniforms, output_scaling=0.001):
    """linear.cpp.base:28-49 with dVRACER's Output Weights Scaling 0.001 (dVRACER.cpp.base:33)."""
    s = layer_sizes(S, H, L, K)
    out, k = [], 0
    for i in range(len(s) - 1):
        ic, oc = s[i], s[i + 1]
        scale = f32(output_scaling if i == len(s) - 2 else 1.0)
        xav = f32(np.sqrt(f32(6.0)) / np.sqrt(f32(oc + ic)))
        u = np.asarray(uniforms[k:k + ic * oc], dtype=f32)
        k += ic * oc
        out.append((scale * xav * u).astype(f32))
        out.append(np.zeros(oc, f32))
    return np.concatenate(out)


def unpack(theta, S, H, L, K):
    s = layer_sizes(S, H, L, K)
    layers, k = [], 0
    for i in range(len(s) - 1):
        ic, oc = s[i], s[i + 1]
        W = theta[k:k + ic * oc].reshape(oc, ic)
        k += ic * oc
        layers.append((W, theta[k:k + oc]))
        k += oc
    return layers


def sigmoid(x):
    """output.cpp.base:149 with a float x: std::exp(-x) is float, 1. + and 1. / are double."""
    x = np.asarray(x, f32)
    return (1.0 / (1.0 + np.exp(-x).astype(f32).astype(f64))).astype(f32)


def sigmoid_backward(g, y):
    """output.cpp.base:208-209: g * x in float, times the double (1. - x); y the transformed output."""
    g, y = np.asarray(g, f32), np.asarray(y, f32)
    return ((g * y).astype(f32).astype(f64) * (1.0 - y.astype(f64))).astype(f32)


def forward(theta, X, S, H, L, K):
    """The critic/policy network of a discrete agent; returns (out, acts)."""
    layers = unpack(theta, S, H, L, K)
    acts = [np.asarray(X, dtype=f32)]
    h = acts[0]
    for W, b in layers[:-1]:
        h = np.tanh((h @ W.T + b).astype(f32)).astype(f32)
        acts.append(h)
    W, b = layers[-1]
    out = (h @ W.T + b).astype(f32)
    out[:, 1 + K] = sigmoid(out[:, 1 + K])
    return out, acts


def backward(theta, acts, out, G, S, H, L, K):
    layers = unpack(theta, S, H, L, K)
    g = np.asarray(G, f32).copy()
    g[:, 1 + K] = sigmoid_backward(g[:, 1 + K], out[:, 1 + K])
    grads = [None] * (2 * len(layers))
    for li in range(len(layers) - 1, -1, -1):
        W, b = layers[li]
        a = acts[li]
        grads[2 * li] = (g.T @ a).astype(f32)
        grads[2 * li + 1] = g.sum(axis=0, dtype=f32)
        if li > 0:
            g = ((g @ W) * (f32(1.0) - a * a)).astype(f32)
    return np.concatenate([x.ravel() for x in grads]).astype(f32)


# ------------------------------------------------------------- policy math
def softmax_policy(row, K):
    """dVRACER::runPolicy (dVRACER.cpp.base:174-218) of one output row: (p, q, invT)."""
    row = np.asarray(row, f32)
    q, invT = row[1:1 + K].copy(), f32(row[1 + K])
    maxq = f32(-np.inf)
    for i in range(K):
        if q[i] > maxq:
            maxq = q[i]
    p = np.zeros(K, f32)
    s = f32(0.0)
    for i in range(K):
        p[i] = f32(np.exp(f32(invT * f32(q[i] - maxq))))
        s = f32(s + p[i])
    inv = f32(f32(1.0) / s)
    for i in range(K):
        p[i] = f32(p[i] * inv)
    return p, q, invT


def categorical(p, x):
    """discrete.cpp.base:46-52"""
    cur, idx = f32(0.0), 0
    K = len(p)
    for idx in range(K - 1):
        cur = f32(cur + f32(p[idx]))
        if f32(x) < cur:
            return idx
    return K - 1


def boundaries(p):
    """the cumulative sums the categorical walk compares x with"""
    out, cur = [], f32(0.0)
    for i in range(len(p) - 1):
        cur = f32(cur + f32(p[i]))
        out.append(cur)
    return np.array(out, f32)


def testing_index(p):
    """discrete.cpp.base:64-65: std::max_element, the first maximum"""
    return int(np.argmax(np.asarray(p)))


def importance_weight(p_cur, p_old, a):
    """discrete.cpp.base:80-95"""
    iw = f32(f32(p_cur[a]) / f32(f32(p_old[a]) + f32(0.00000001)))
    if iw > f32(1024.0):
        iw = f32(1024.0)
    if iw < f32(-1024.0):
        iw = f32(-1024.0)
    return iw


def importance_weight_gradient(q, invT, p_cur, p_old, a):
    """discrete.cpp.base:97-132; returns K + 1 values (q, invT)."""
    K = len(q)
    iw = importance_weight(p_cur, p_old, a)
    g = np.zeros(K + 1, f32)
    qp = f32(0.0)
    for i in range(K):
        if i == a:
            g[i] = f32(f64(iw) * (1.0 - f64(p_cur[i])) * f64(invT))
        else:
            g[i] = f32(f32(-iw * f32(p_cur[i])) * f32(invT))
        qp = f32(qp + f32(f32(q[i]) * f32(p_cur[i])))
    g[K] = f32(iw * f32(f32(q[a]) - qp))
    return g


def kl_gradient(q, invT, p_cur, p_old):
    """discrete.cpp.base:134-163; returns K + 1 values (q, invT)."""
    K = len(q)
    invT = f32(invT)
    g = np.zeros(K + 1, f32)
    for i in range(K):
        for j in range(K):
            if i == j:
                g[i] = f32(f64(g[i]) - f64(f32(invT * f32(p_old[j]))) * (1.0 - f64(p_cur[i])))
            else:
                g[i] = f32(g[i] + f32(f32(invT * f32(p_old[j])) * f32(p_cur[i])))
    qp = f32(0.0)
    for j in range(K):
        qp = f32(qp + f32(f32(q[j]) * f32(p_cur[j])))
    for j in range(K):
        g[K] = f32(g[K] - f32(f32(p_old[j]) * f32(f32(q[j]) - qp)))
    return g


def action_uniform(seed, env_step, e):
    """The device's action uniform of environment e at environment step env_step."""
    r = V.philox4x32((env_step & 0xFFFFFFFF, env_step >> 32, e, 0x4441), seed & 0xFFFFFFFF, seed >> 32)
    return f32(f32(r[0] >> 8) * f32(5.9604644775390625e-08))


# --------------------------------------------------------------- the agent
def pack(q, invT, p, idx):
    """a discrete policy_t as one vector: [q (K), invT, p (K), action index]"""
    return np.concatenate([np.asarray(q, f32), [f32(invT)], np.asarray(p, f32), [f32(idx)]]).astype(f32)


class Agent(V.Agent):
    """vracer_ref.Agent's replay memory and REF-ER bookkeeping with the
    discrete policy.  The replay fields exp_pol / cur_pol hold pack(...) of the
    experience's / the current policy (the current one keeps the experience's
    action index)."""

    def __init__(self, S, K, H=64, L=2, theta=None, possible_actions=None, **kw):
        self.K = K
        self.actions = np.asarray(possible_actions, f32).reshape(K, -1)
        super().__init__(S, self.actions.shape[1], H, L, theta, **kw)

    def policy(self, X):
        out, _ = forward(self.theta, np.atleast_2d(X), self.S, self.H, self.L, self.K)
        return out

    def unpacked(self, v):
        K = self.K
        return v[:K], f32(v[K]), v[K + 1:2 * K + 1], int(v[2 * K + 1])

    def field(self, name):
        """replay fields in the device's layout"""
        K, er = self.K, self.er
        if name in ("exp_policy", "cur_policy"):
            return np.stack([v[:K + 1] for v in er[name[:3] + "_pol"]]).astype(f32)
        if name in ("exp_action_probabilities", "cur_action_probabilities"):
            return np.stack([v[K + 1:2 * K + 1] for v in er[name[:3] + "_pol"]]).astype(f32)
        if name == "action_index":
            return np.array([int(v[2 * K + 1]) for v in er["exp_pol"]], np.int32)
        raise KeyError(name)

    def train_policy(self, mb):
        """dVRACER::trainPolicy (dVRACER.cpp.base:59-81) for a sorted mini-batch; returns (G, grad)."""
        er, K, B = self.er, self.K, len(mb)
        X = np.stack([er["state"][i] for i in mb])
        out, acts = forward(self.theta, X, self.S, self.H, self.L, K)
        delta = 0
        for b in range(B):
            if b > 0 and mb[b] == mb[b - 1]:
                continue
            e = mb[b]
            p, q, invT = softmax_policy(out[b], K)
            _, _, p_old, a = self.unpacked(er["exp_pol"][e])
            iw = importance_weight(p, p_old, a)
            tiw = min(self.iw_trunc, iw)
            onp = bool(iw > f32(1.0) / self.cutoff and iw < self.cutoff)
            if er["onp"][e] and not onp:
                delta += 1
            if not er["onp"][e] and onp:
                delta -= 1
            er["cur_pol"][e] = pack(q, invT, p, a)
            er["v"][e] = out[b, 0]
            er["tv"][e] = f32(0.0)
            er["iw"][e] = iw
            er["onp"][e] = onp
            er["tiw"][e] = tiw
        for b in range(B):
            if b > 0 and mb[b] == mb[b - 1]:
                continue
            e = mb[b]
            if er["term"][e] == TRUNCATED:
                er["tv"][e] = self.policy(er["tstate"][e])[0, 0]
        self.off_count += delta
        self.off_ratio = f32(f32(self.off_count) / f32(self.size()))
        self.cutoff = f32(self.cutoff_scale / f32(f32(1.0) + f32(self.anneal * f32(self.update_count))))
        rmb = [mb[B - 1]] + [mb[i] for i in range(B - 2, -1, -1) if er["ep_id"][mb[i]] != er["ep_id"][mb[i + 1]]]
        for end in rmb:
            start = max(end - er["ep_pos"][end], 0)
            ret = f32(0.0)
            if er["term"][end] == TRUNCATED:
                ret = er["tv"][end]
            if er["term"][end] == NON_TERMINAL:
                ret = er["ret"][end + 1]
            for c in range(end, start - 1, -1):
                v = er["v"][c]
                ret = f32(v + f32(er["tiw"][c] * f32(f32(self.scaled_reward(c) + f32(self.gamma * ret)) - v)))
                er["ret"][c] = ret
        # calculatePolicyGradients (dVRACER.cpp.base:83-154)
        G = np.zeros((B, 2 + K), f32)
        for b, e in enumerate(mb):
            V_ = er["v"][e]
            q, invT, p_cur, _ = self.unpacked(er["cur_pol"][e])
            _, _, p_old, a = self.unpacked(er["exp_pol"][e])
            G[b, 0] = f32(er["ret"][e] - V_)
            if er["onp"][e]:
                qr = self.scaled_reward(e)
                if er["term"][e] == NON_TERMINAL:
                    qr = f32(qr + f32(self.gamma * er["ret"][e + 1]))
                if er["term"][e] == TRUNCATED:
                    qr = f32(qr + f32(self.gamma * er["tv"][e]))
                loss = f32(qr - V_)
                pg = importance_weight_gradient(q, invT, p_cur, p_old, a)
                G[b, 1:] = (f32(self.beta * loss) * pg).astype(f32)
            klg = kl_gradient(q, invT, p_cur, p_old)
            G[b, 1:] = (G[b, 1:] + f32(-(f32(1.0) - self.beta)) * klg).astype(f32)
        if not np.all(np.isfinite(G)):
            raise FloatingPointError("Gradient loss returned an invalid value")
        grad = backward(self.theta, acts, out, G, self.S, self.H, self.L, K)
        if self.l2[0]:
            grad = (grad - self.l2[1] * self.theta).astype(f32)
        self.adam.eta = self.lr
        self.theta = self.adam.step(self.theta, grad)
        self.update_count += 1
        self.lr = f32(self.lr0 / f32(f32(1.0) + f32(self.anneal * f32(self.update_count))))
        if self.off_ratio > self.off_target:
            self.beta = f32(f32(f32(1.0) - self.lr) * self.beta)
        else:
            self.beta = f32(f32(f32(f32(1.0) - self.lr) * self.beta) + self.lr)
        return G, grad


class Rollouts(V.Rollouts):
    """vracer_ref.Rollouts with the discrete agent's categorical actions:
    step(uniforms) takes one uniform per environment; the Possible Action's
    component 0 is the CartPole's force."""

    def probabilities(self):
        """the action probabilities of every environment's current state"""
        X = np.stack([self.scaled_state(e, c.u) for e, c in enumerate(self.carts)])
        out = self.agent.policy(X)
        return [softmax_policy(out[e], self.agent.K)[0] for e in range(self.E)]

    def step(self, uniforms, record=None):
        ag, K = self.agent, self.agent.K
        X = np.stack([self.scaled_state(e, c.u) for e, c in enumerate(self.carts)])
        out = ag.policy(X)
        finished = []
        for e, cart in enumerate(self.carts):
            b = self.buf[e]
            p, q, invT = softmax_policy(out[e], K)
            idx = categorical(p, uniforms[e])
            if record is not None:
                record.append((e, p, idx))
            act = ag.actions[idx].copy()
            b["states"].append(X[e].copy())
            b["actions"].append(act)
            b["pols"].append(pack(q, invT, p, idx))
            b["vals"].append(out[e, 0])
            failed = cart.advance(act[0])
            r = f32(cart.reward(self.env_id(e)))
            b["rewards"].append(r)
            b["cum"] = f32(b["cum"] + r)
            if failed:
                finished.append((e, TERMINAL))
            elif cart.step >= self.T:
                finished.append((e, TRUNCATED))
        new, rewards = 0, []
        for e, term in finished:
            b = self.buf[e]
            ag.process_episode(self.env_id(e), b["states"], b["actions"], b["rewards"], b["pols"], b["vals"], term,
                               tstate=self.scaled_state(e, self.carts[e].u))
            new += len(b["rewards"])
            rewards.append(b["cum"])
        for e, _ in finished:
            self._launch(e, self.next_sample)
            self.next_sample += 1
        return new, rewards


def testing_episodes(theta, sample_ids, launch_ids, S, H, L, K, actions, max_steps):
    """Agent::testingGeneration with the CartPole: the first most probable action per step."""
    actions = np.asarray(actions, f32).reshape(K, -1)
    rewards = []
    for sid, lid in zip(sample_ids, launch_ids):
        cp = V.CartPole()
        cp.reset(int(sid) * 1024 + int(lid))
        total = f32(0.0)
        for _ in range(max_steps):
            out, _ = forward(theta, cp.u.astype(f32)[None, :], S, H, L, K)
            p, _, _ = softmax_policy(out[0], K)
            done = cp.advance(float(actions[testing_index(p), 0]))
            total = f32(total + f32(cp.reward(0)))
            if done:
                break
        rewards.append(total)
    return np.array(rewards, f32)
