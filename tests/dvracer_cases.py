"""Shared pieces of the dVRACER tests: the reference's
examples/learning/reinforcement/cartpole/run-dvracer.py configuration, and
restatement agents (tests/dvracer_ref.py) whose replay memory is loaded into a
discrete device agent through the C-ABI's fields."""
import numpy as np

import dvracer_ref as D
from vracer_replay import load_replay as load_continuous_fields

f32 = np.float32


def cartpole_dvracer(max_generations=50, environments=1, kernel="CartPole"):
    """run-dvracer.py key for key with its defaults (--engine OneDNN, --optimizer
    Adam, learning rate 1e-3, 1 concurrent environment); the host `env` function
    replaced by the device CartPole kernel unless kernel is None."""
    import korali
    e = korali.Experiment()
    e["Problem"]["Type"] = "Reinforcement Learning / Discrete"
    e["Problem"]["Possible Actions"] = [[-10.0], [10.0]]
    if kernel is None:
        e["Problem"]["Environment Function"] = lambda s: None
    else:
        e["Problem"]["Environment Kernel"] = kernel
    e["Problem"]["Environment Count"] = 3
    e["Problem"]["Actions Between Policy Updates"] = 5
    for i, n in enumerate(["Cart Position", "Cart Velocity", "Pole Angle", "Pole Angular Velocity"]):
        e["Variables"][i]["Name"] = n
        e["Variables"][i]["Type"] = "State"
    e["Variables"][4]["Name"] = "Force"
    e["Variables"][4]["Type"] = "Action"
    e["Solver"]["Type"] = "Agent / Discrete / dVRACER"
    e["Solver"]["Mode"] = "Training"
    e["Solver"]["Episodes Per Generation"] = 10
    e["Solver"]["Experiences Between Policy Updates"] = 1
    e["Solver"]["Learning Rate"] = 1e-3
    e["Solver"]["Mini Batch"]["Size"] = 32
    e["Solver"]["Concurrent Environments"] = environments
    e["Solver"]["Experience Replay"]["Start Size"] = 4096
    e["Solver"]["Experience Replay"]["Maximum Size"] = 65536
    e["Solver"]["Experience Replay"]["Off Policy"]["Annealing Rate"] = 5.0e-8
    e["Solver"]["Experience Replay"]["Off Policy"]["Cutoff Scale"] = 5.0
    e["Solver"]["Experience Replay"]["Off Policy"]["REFER Beta"] = 0.3
    e["Solver"]["Experience Replay"]["Off Policy"]["Target"] = 0.1
    e["Solver"]["State Rescaling"]["Enabled"] = True
    e["Solver"]["Reward"]["Rescaling"]["Enabled"] = True
    e["Solver"]["Neural Network"]["Engine"] = "OneDNN"
    e["Solver"]["Neural Network"]["Optimizer"] = "Adam"
    for l in (0, 2):
        e["Solver"]["Neural Network"]["Hidden Layers"][l]["Type"] = "Layer/Linear"
        e["Solver"]["Neural Network"]["Hidden Layers"][l]["Output Channels"] = 32
        e["Solver"]["Neural Network"]["Hidden Layers"][l + 1]["Type"] = "Layer/Activation"
        e["Solver"]["Neural Network"]["Hidden Layers"][l + 1]["Function"] = "Elementwise/Tanh"
    e["Solver"]["Termination Criteria"]["Max Generations"] = max_generations
    e["File Output"]["Enabled"] = False
    e["Console Output"]["Verbosity"] = "Silent"
    e["Random Seed"] = 1337
    return e


def theta_for(S, H, L, K, seed, spread=0.15, q_spread=0.0):
    """initial hyperparameters plus a spread; q_spread widens the output
    layer's biases so that the action probabilities differ between rows"""
    n = D.hyperparameter_count(S, H, L, K)
    rng = np.random.default_rng(seed)
    th = D.initial_hyperparameters(S, H, L, K, rng.uniform(-1, 1, n))
    th = (th + spread * rng.standard_normal(n) / np.sqrt(H)).astype(f32)
    if q_spread:
        th[n - (K + 2):] += (q_spread * rng.standard_normal(K + 2)).astype(f32)
    return th


def actions_for(K, A):
    return (np.arange(K * A, dtype=f32).reshape(K, A) - f32(K * A / 2)) * f32(0.5)


def fill_synthetic(S, A, K, H, L, n_eps, seed, max_size=600, steps=(1, 30), **agent_kw):
    """A restatement agent's replay memory filled with synthetic episodes:
    states and rewards from a seeded generator, categorical actions from the
    agent's own policy, terminal and truncated endings alternating."""
    th = theta_for(S, H, L, K, seed, q_spread=1.0)
    ag = D.Agent(S, K, H, L, th, possible_actions=actions_for(K, A), max_size=max_size, **agent_kw)
    rng = np.random.default_rng(seed + 100)
    for ep in range(n_eps):
        T = int(rng.integers(steps[0], steps[1]))
        states = rng.uniform(-1, 1, (T, S)).astype(f32)
        out = ag.policy(states)
        pols, acts = [], []
        for t in range(T):
            p, q, invT = D.softmax_policy(out[t], K)
            idx = D.categorical(p, f32(rng.uniform()))
            pols.append(D.pack(q, invT, p, idx))
            acts.append(ag.actions[idx].copy())
        rewards = rng.normal(0, 1, T).astype(f32)
        term = D.TERMINAL if ep % 2 else D.TRUNCATED
        ag.process_episode(ep % 3, states, acts, rewards, pols, out[:, 0], term,
                           tstate=rng.uniform(-1, 1, S).astype(f32))
    return ag, th


def load_replay(d, ag):
    """the restatement's replay memory into the device agent's fields"""
    packed_exp, packed_cur = ag.er["exp_pol"], ag.er["cur_pol"]
    try:  # the shared fields take the K + 1 distribution parameters as the policy
        ag.er["exp_pol"] = list(ag.field("exp_policy"))
        ag.er["cur_pol"] = list(ag.field("cur_policy"))
        load_continuous_fields(d, ag)
    finally:
        ag.er["exp_pol"], ag.er["cur_pol"] = packed_exp, packed_cur
    d.set("action_index", ag.field("action_index"))
    d.set("exp_action_probabilities", ag.field("exp_action_probabilities"))
    d.set("cur_action_probabilities", ag.field("cur_action_probabilities"))
