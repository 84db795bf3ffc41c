"""Replay memories for the VRACER GPU tests: an oracle agent (oracle/vracer_ref.py)
filled by CartPole rollouts or by synthetic episodes of a host environment's
shapes, and its replay memory loaded into a device agent through the C-ABI's
fields.  Shared by test_gpu_vracer.py and test_gpu_vracer_update_f64.py."""
import numpy as np

import vracer_ref as V

f32 = np.float32


def device(**kw):
    from korali_amd.vracer import VracerDevice
    return VracerDevice(**kw)


def close(a, b, rtol, atol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    # NaN on both sides is agreement (a NaN rescaling sigma, see
    # test_environment_steps_match_oracle); NaN on one side is not
    both = np.isnan(a) & np.isnan(b)
    assert not np.any(np.isnan(a) ^ np.isnan(b)), "NaN on one side only"
    a, b = np.where(both, 0.0, a), np.where(both, 0.0, b)
    err = np.abs(a - b) - (atol + rtol * np.abs(b))
    assert err.max() <= 0, f"max excess {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"


def theta_for(H, L, seed, spread=0.15, S=4, A=1):
    n = V.hyperparameter_count(S, H, L, A)
    rng = np.random.default_rng(seed)
    th = V.initial_hyperparameters(S, H, L, A, rng.uniform(-1, 1, n))
    return (th + spread * rng.standard_normal(n) / np.sqrt(H)).astype(f32)


def fill_replay(H, L, E, steps, max_size, seed=3, bounds=None, **agent_kw):
    """An oracle agent's replay memory filled by its own CartPole rollouts
    (S = 4, A = 1) with the device's action-noise stream."""
    th = theta_for(H, L, seed)
    ag = V.Agent(4, 1, H, L, th, max_size=max_size, bounds=bounds, **agent_kw)
    ro = V.Rollouts(ag, E, max_steps=40)
    for s in range(steps):
        ro.step(V.action_noise(seed, s, E, 1))
    return ag, th


def fill_synthetic(Sx, Ax, H, L, n_eps, seed, bounds=None, max_size=600, steps=(1, 30), **agent_kw):
    """An oracle agent's replay memory filled with synthetic episodes of Sx
    state and Ax action variables (a host environment's shapes): states and
    rewards from a seeded generator, actions drawn from the agent's own
    policy (clipped to the bounds), the policy and value stored as
    processEpisode stores them; terminal and truncated endings alternate.
    steps: the episode lengths are drawn from [steps[0], steps[1])."""
    n = V.hyperparameter_count(Sx, H, L, Ax)
    rng = np.random.default_rng(seed)
    th = (V.initial_hyperparameters(Sx, H, L, Ax, rng.uniform(-1, 1, n))
          + 0.15 * rng.standard_normal(n) / np.sqrt(H)).astype(f32)
    ag = V.Agent(Sx, Ax, H, L, th, max_size=max_size, bounds=bounds, **agent_kw)
    for ep in range(n_eps):
        T = int(rng.integers(steps[0], steps[1]))
        states = rng.uniform(-1, 1, (T, Sx)).astype(f32)
        out = ag.policy(states)
        acts = (out[:, 1:1 + Ax] + out[:, 1 + Ax:] * rng.standard_normal((T, Ax)).astype(f32)).astype(f32)
        if bounds is not None:
            acts = np.clip(acts, bounds[0], bounds[1]).astype(f32)
        rewards = rng.normal(0, 1, T).astype(f32)
        term = V.TERMINAL if ep % 2 else V.TRUNCATED
        ag.process_episode(ep % 3, states, acts, rewards, out[:, 1:], out[:, 0], term,
                           tstate=rng.uniform(-1, 1, Sx).astype(f32))
    return ag, th


def load_replay(d, ag):
    er, n = ag.er, ag.size()
    d.set("state", np.stack(er["state"]))
    d.set("action", np.stack(er["action"]))
    d.set("reward", np.array(er["reward"], f32))
    d.set("environment_id", np.array(er["env"]))
    d.set("termination", np.array(er["term"]))
    d.set("truncated_state", np.stack(er["tstate"]))
    d.set("exp_policy", np.stack(er["exp_pol"]))
    d.set("cur_policy", np.stack(er["cur_pol"]))
    d.set("exp_state_value", np.array(er["exp_v"], f32))
    d.set("state_value", np.array(er["v"], f32))
    d.set("retrace", np.array(er["ret"], f32))
    d.set("importance_weight", np.array(er["iw"], f32))
    d.set("truncated_importance_weight", np.array(er["tiw"], f32))
    d.set("truncated_state_value", np.array(er["tv"], f32))
    d.set("on_policy", np.array(er["onp"], np.int32))
    d.set("episode_id", np.array(er["ep_id"], np.int64))
    d.set("episode_pos", np.array(er["ep_pos"], np.int32))
    d.set_scalar("total", n)
    d.set_scalar("size", n)
    d.set_scalar("off_policy_count", ag.off_count)
    d.set_scalar("current_episode", ag.current_episode)
    d.set_scalar("experience_count", ag.experience_count)
