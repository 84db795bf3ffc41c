"""Every kernel of the VRACER policy update (korali_amd/csrc/kg_vracer.hip)
against float64 at the shapes where the kernels have edges, with the error
bounds of tests/vracer_f64.py (theorems about float32 sums, nothing tuned);
the drawn mini-batches of every draw path against the oracle's ids; and the
graph-replayed update at more than 8 state variables."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import vracer_f64 as F  # noqa: E402
import vracer_ref as V  # noqa: E402
from vracer_replay import close, device, fill_replay, fill_synthetic, load_replay  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.mark.parametrize("ahead", ["1", "0"])
def test_graph_replayed_updates_equal_kernel_launches_12_states(monkeypatch, ahead):
    """test_gpu_vracer.py's graph-against-launches equality with a host
    environment's 12 state and 2 action variables: the graph's input layer
    with the mini-batches drawn ahead must take every state variable (more
    than k_vr_gather_in holds), as k_vr_minibatch + k_vr_fwd_in do; bit for bit."""
    Sx, Ax, glen = 12, 2, "4"
    ag, th = fill_synthetic(Sx, Ax, 64, 2, 60, 11)
    runs = []
    monkeypatch.setenv("KORALI_AMD_VR_FUSED", "0")
    monkeypatch.setenv("KORALI_AMD_VR_DRAW_AHEAD", ahead)
    for g in (glen, "0"):
        monkeypatch.setenv("KORALI_AMD_VR_GRAPH", g)
        d = device(state_size=Sx, action_size=Ax, hidden_size=64, hidden_layers=2, environments=8,
                   mini_batch_size=64, replay_maximum_size=600, replay_start_size=100, hyperparameters=th,
                   host_environment=True)
        load_replay(d, ag)
        d.train_policy(11)
        d.train_policy(int(glen))  # the captured graph replayed again
        runs.append((d.hyperparameters, d.get("retrace")[:ag.size()], d.get("importance_weight")[:ag.size()],
                     d.get("loss_gradient"), d.get("adam_first_moment")))
        d.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ------------------------------------------------ every stage against float64

CLIP = (np.array([-0.5], f32), np.array([0.5], f32))
E = 8

# what each of vracer_f64.CASES reaches (hidden, L, B, S, A):
#   64, 1, 2     the L == 1 path (the output layer's wgrad alone in k_vr_multi); K = 2: scalar staging,
#                M = 4 and 2, the MFMA k extent rounded up from 2 to 8
#   64, 2, 37    odd B: scalar staging for K = B, M edges 37 / 74, uneven wgrad lanes
#   100, 2, 36   hidden width padded to 128 through umap; full (vector) and edge (scalar) tiles in one grid;
#                vector staging with kc = 36 and its zero-fill loop; Clipped Normal
#   320, 3, 260  two K panels both ways (320 = 256 + 64, 260 = 256 + 4); k_vr_fwd_out's second trip of
#                columns; the dH ping-pong swapping twice
#   64, 2, 64, 12, 2   a host environment with more than 8 state variables
#   100, 2, 37, 3, 2   L2 regularisation in Adam, on real and padded parameters


def device_layout(S, H, PH, L, O):
    """the positions of the user's hyperparameters in the device's padded layout"""
    su, sd = [S] + [H] * L + [O], [S] + [PH] * L + [O]
    real = []
    for l in range(L + 1):
        w = np.zeros((sd[l + 1], sd[l]), bool)
        w[:su[l + 1], :su[l]] = True
        b = np.zeros(sd[l + 1], bool)
        b[:su[l + 1]] = True
        real += [w.ravel(), b]
    return np.concatenate(real)


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: "-".join(map(str, c)))
def test_update_stages_lie_within_float64_bounds(case):
    """Three forced updates (sorted ids, one duplicate); after each, every
    stage of vracer_f64.update_ratios on the device's own intermediates:
    err / bound <= 1 everywhere.  The gather is exact; padded hidden units
    are exactly 0 in the activations, the hidden gradients, the gradient, the
    Adam moments and the hyperparameters."""
    H, L, B, S, A, kind = case
    O = 1 + 2 * A
    kw = dict(state_size=S, action_size=A, hidden_size=H, hidden_layers=L, environments=E, mini_batch_size=B,
              replay_maximum_size=600, replay_start_size=100)
    if kind in ("cartpole", "clipped"):
        ag, th = fill_replay(H, L, E, 90, 600, bounds=CLIP if kind == "clipped" else None)
        if kind == "clipped":
            kw.update(policy_distribution="Clipped Normal", action_lower_bound=-0.5, action_upper_bound=0.5)
    else:
        ag, th = fill_synthetic(S, A, H, L, 60, 11)
        kw.update(host_environment=True)
        if kind == "host_l2":
            kw.update(l2_regularization_enabled=True, l2_regularization_importance=F.L2_IMPORTANCE)
    d = device(hyperparameters=th, **kw)
    load_replay(d, ag)
    PH, rows = int(d.scalar("padded_hidden_size")), max(E, 2 * B)
    assert PH == (H + 63) // 64 * 64
    real = device_layout(S, H, PH, L, O)
    scale, shift, soft = V.output_transform(A, 1.0, ag.shift())
    states, tstates = np.stack(ag.er["state"]), np.stack(ag.er["tstate"])
    rng = np.random.default_rng(9)
    theta0, m0, v0 = d.hyperparameters, d.get("adam_first_moment"), d.get("adam_second_moment")
    b1p, b2p = f32(1.0), f32(1.0)
    worst = {}
    for u in range(3):
        ids = np.sort(rng.integers(0, ag.size() - 1, B)).astype(np.uint32)
        if B > 2 or u == 1:
            ids[1] = ids[0]  # a duplicate entry
            ids.sort()
        d.train_minibatch(ids)
        b1p, b2p = f32(b1p * F.B1), f32(b2p * F.B2)  # as the oracle's Adam schedules them
        assert f32(d.scalar("adam_beta1_pow")) == b1p and f32(d.scalar("adam_beta2_pow")) == b2p
        assert f32(d.scalar("adam_eta")) == f32(1e-4)
        X = d.get("mini_batch_states").reshape(2 * B, S)
        assert np.array_equal(d.get("mini_batch"), ids)
        assert np.array_equal(X[:B], states[ids]) and np.array_equal(X[B:], tstates[ids])
        acts = d.get("activations").reshape(L, rows, PH)[:, :2 * B]
        dHa = d.get("hidden_gradient_a").reshape(B, PH)
        dHb = d.get("hidden_gradient_b").reshape(B, PH)
        assert not acts[:, :, H:].any() and not dHa[:, H:].any() and not dHb[:, H:].any()
        dH = {(L - 1) % 2: dHa[:, :H]}  # (the ping-pong: vr_field's comment in kg_vracer.hip)
        if L >= 2:
            dH[(L - 2) % 2] = dHb[:, :H]
        dev = {n: d.get("device_" + n) for n in ("hyperparameters", "gradient", "adam_first_moment",
                                                  "adam_second_moment")}
        post = {n: d.get(n) for n in dev}
        for n in dev:
            assert not dev[n][~real].any(), n                # padded entries exactly 0
            assert np.array_equal(dev[n][real], post[n]), n  # the user layout is the device's, gathered
        o = dict(S=S, A=A, H=H, L=L, B=B, scale=scale, shift=shift, soft=soft, layers=F.unpack(theta0, S, H, L, A),
                 X=X, acts=[acts[l, :, :H] for l in range(L)], out=d.get("policy_output").reshape(rows, O)[:2 * B],
                 G=d.get("loss_gradient").reshape(B, O), dZ=d.get("output_layer_gradient").reshape(B, O), dH=dH,
                 grads=F.unpack(post["gradient"], S, H, L, A), theta0=theta0, m0=m0, v0=v0, grad=post["gradient"],
                 m=post["adam_first_moment"], v=post["adam_second_moment"], theta=post["hyperparameters"],
                 eta=f32(1e-4), b1p=b1p, b2p=b2p, l2imp=F.L2_IMPORTANCE if kind == "host_l2" else None)
        assert np.all(np.isfinite(o["G"])) and np.any(o["G"] != 0)
        for k, r in F.update_ratios(o).items():
            worst[k] = max(worst.get(k, 0.0), float(r.max()))
        theta0, m0, v0 = post["hyperparameters"], post["adam_first_moment"], post["adam_second_moment"]
    d.close()
    print(f"device {case}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    # input layer, L - 1 hidden forwards, output layer, dZ; dW / db of L + 1 layers; the readable dH; Adam's three
    assert len(worst) == (L + 2) + 2 * (L + 1) + min(L, 2) + 3
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# --------------------------------------- drawn mini-batches, every sort form
SEED = 77
_synthetic = {}


def synthetic_agent():
    """one replay memory for every draw test (read only: the oracle side only sizes the draw)"""
    if "ag" not in _synthetic:
        _synthetic["ag"] = fill_synthetic(4, 1, 64, 2, 60, 11)
    return _synthetic["ag"]


_ids = {}


def oracle_ids(ag, ctr, B):
    if (ctr, B) not in _ids:
        _ids[ctr, B] = np.array(ag.minibatch_ids(V.minibatch_uniforms(SEED, ctr, B)), np.uint32)
    return _ids[ctr, B]


# path: environment, updates per train_policy call
PATHS = {
    "k_vr_minibatch": (dict(KORALI_AMD_VR_GRAPH="0"), 1),
    "draw_ahead_graph_of_1": (dict(KORALI_AMD_VR_GRAPH="1"), 1),
    "draw_ahead_graph_of_2": (dict(KORALI_AMD_VR_GRAPH="2"), 2),
    "k_vr_minibatch_in": (dict(KORALI_AMD_VR_GRAPH="0", KORALI_AMD_VR_DRAW_IN="1"), 1),
    "k_vr_fwd_fused": (dict(KORALI_AMD_VR_GRAPH="0", KORALI_AMD_VR_FUSED="1"), 1),
}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("B", [2, 37, 100, 260, 1024])
def test_drawn_mini_batches_match_oracle(monkeypatch, B, path):
    """generateMiniBatch's sorted ids on every draw path and every form of the
    sort (in-wave shuffles, LDS stages, the strided loop of the 256-thread
    callers above 256 keys; padding keys at sizes that are no power of two):
    equal to the oracle's for the same seed, draw counter and replay size,
    after the first and the second call (the counter's advance)."""
    ag, th = synthetic_agent()
    env, per_call = PATHS[path]
    for k, v in {"KORALI_AMD_VR_FUSED": "0", "KORALI_AMD_VR_DRAW_IN": "0", "KORALI_AMD_VR_DRAW_AHEAD": "1", **env}.items():
        monkeypatch.setenv(k, v)
    d = device(state_size=4, action_size=1, hidden_size=64, hidden_layers=2, environments=E, mini_batch_size=B,
               replay_maximum_size=600, replay_start_size=100, hyperparameters=th, host_environment=True, seed=SEED)
    load_replay(d, ag)
    for call in range(2):
        d.train_policy(per_call)
        done = (call + 1) * per_call
        assert np.array_equal(d.get("mini_batch"), oracle_ids(ag, (done - 1) * B, B)), call
        assert d.scalar("mini_batch_counter") == done * B
    assert np.all(np.isfinite(d.hyperparameters))
    d.close()


def test_update_with_1024_rows_matches_oracle():
    """Mini Batch Size 1024 (k_vr_meta with two rows per thread): one forced
    update against the oracle, test_gpu_vracer.py's tolerances."""
    B = 1024
    ag, th = fill_synthetic(4, 1, 64, 2, 60, 11)
    d = device(state_size=4, action_size=1, hidden_size=64, hidden_layers=2, environments=E, mini_batch_size=B,
               replay_maximum_size=600, replay_start_size=100, hyperparameters=th, host_environment=True)
    load_replay(d, ag)
    ids = np.sort(np.random.default_rng(5).integers(0, ag.size() - 1, B)).astype(np.uint32)
    G, grad = ag.train_policy([int(i) for i in ids])
    d.train_minibatch(ids)
    close(d.get("loss_gradient").reshape(B, -1), G, 1e-3, 1e-4)
    close(d.get("gradient"), grad, 2e-3, 2e-3 * np.abs(grad).max())
    close(d.hyperparameters, ag.theta, 1e-4, 1e-6)
    assert np.array_equal(d.get("on_policy")[:ag.size()], np.array(ag.er["onp"], np.int32))
    close(d.get("retrace")[:ag.size()], np.array(ag.er["ret"], f32), 1e-4, 1e-5)
    close(d.get("importance_weight")[:ag.size()], np.array(ag.er["iw"], f32), 1e-4, 1e-6)
    assert d.scalar("off_policy_count") == ag.off_count
    d.close()


def test_walks_beyond_the_staging_space_equal_one_thread_walks(monkeypatch):
    """A mini-batch whose retrace walks hold more entries than k_vr_meta's LDS
    staging space (6144): 256 rows over 140 episodes of 48 to 60 steps, each
    episode's last entry among them.  Retrace values and loss gradient equal
    the one-thread walks' bit for bit."""
    B, n_eps = 256, 140
    ag, th = fill_synthetic(4, 1, 64, 2, n_eps, 13, max_size=8192, steps=(48, 61))
    pos = np.array(ag.er["ep_pos"])
    last = np.flatnonzero(np.append(pos[1:] == 0, True))  # every episode's last entry
    assert last.size == n_eps and int((pos[last] + 1).sum()) > 6144
    rng = np.random.default_rng(3)
    ids = np.sort(np.concatenate([last, rng.integers(0, ag.size() - 1, B - n_eps)])).astype(np.uint32)
    runs = []
    for staged in ("1", "0"):
        monkeypatch.setenv("KORALI_AMD_VR_STAGED", staged)
        d = device(state_size=4, action_size=1, hidden_size=64, hidden_layers=2, environments=E, mini_batch_size=B,
                   replay_maximum_size=8192, replay_start_size=100, hyperparameters=th, host_environment=True)
        load_replay(d, ag)
        d.train_minibatch(ids)
        assert d.get("meta_phase_ticks")[4] > 6144  # (the walked entries of this update)
        runs.append((d.get("retrace")[:ag.size()], d.get("loss_gradient"), d.hyperparameters))
        d.close()
    assert np.any(runs[0][0] != np.array(ag.er["ret"], f32))  # the walks rewrote the retrace values
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
