"""Learner/DeepSupervisor through korali.Engine on the device: the reference's
sine-wave examples, the initial hyperparameters, continued and resumed runs."""
import os

import numpy as np
import pytest

import supervisor_ref as SR
import vracer_f64 as F

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64

TANH = {"Type": "Layer/Activation", "Function": "Elementwise/Tanh", "Alpha": 1.0, "Beta": 0.0}
LAYERS = [{"Type": "Layer/Linear", "Output Channels": 32}, TANH, {"Type": "Layer/Linear", "Output Channels": 32}, TANH,
          {"Type": "Layer/Linear", "Output Channels": 1}]


def sine(n, rs):
    x = rs.uniform(0, 2 * np.pi, n)
    return x, np.tanh(np.exp(np.sin(x))) * 5.0


def ffn(korali, x, y, generations, steps=200, lr=0.005, seed=0xC0FFEE, ni=100):
    """examples/learning/supervised/sineWave/run-ffn.py"""
    e = korali.Experiment()
    e["Problem"]["Type"] = "Supervised Learning"
    e["Problem"]["Max Timesteps"] = 1
    e["Problem"]["Training Batch Size"] = len(x)
    e["Problem"]["Inference Batch Size"] = ni
    e["Problem"]["Input"]["Data"] = [[[float(v)]] for v in x]
    e["Problem"]["Input"]["Size"] = 1
    e["Problem"]["Solution"]["Data"] = [[float(v)] for v in y]
    e["Problem"]["Solution"]["Size"] = 1
    e["Solver"]["Type"] = "Learner/DeepSupervisor"
    e["Solver"]["Loss Function"] = "Mean Squared Error"
    e["Solver"]["Steps Per Generation"] = steps
    e["Solver"]["Learning Rate"] = lr
    e["Solver"]["Neural Network"]["Engine"] = "OneDNN"
    e["Solver"]["Neural Network"]["Optimizer"] = "Adam"
    for i in (0, 2):
        e["Solver"]["Neural Network"]["Hidden Layers"][i]["Type"] = "Layer/Linear"
        e["Solver"]["Neural Network"]["Hidden Layers"][i]["Output Channels"] = 32
        e["Solver"]["Neural Network"]["Hidden Layers"][i + 1]["Type"] = "Layer/Activation"
        e["Solver"]["Neural Network"]["Hidden Layers"][i + 1]["Function"] = "Elementwise/Tanh"
    e["Console Output"]["Verbosity"] = "Silent"
    e["File Output"]["Enabled"] = False
    e["Random Seed"] = seed
    e["Solver"]["Termination Criteria"]["Max Generations"] = generations
    return e


def theta_of(e):
    return np.asarray(e["Solver"]["Hyperparameters"], f32)


def test_sine_wave_ffn_reaches_the_examples_threshold():
    import korali

    rs = np.random.RandomState(0xC0FFEE)
    x, y = sine(500, rs)
    e = ffn(korali, x, y, 10)
    korali.Engine().run(e)
    xt, yt = sine(100, rs)
    out = np.asarray(e.getEvaluation([[[float(v)]] for v in xt]))[:, 0]
    mse = np.mean((out - yt) ** 2)
    assert mse < 0.05, mse
    assert e["Current Generation"] == 10 and e["Solver"]["Current Loss"] < 0.05
    with pytest.raises(RuntimeError, match=r"Batch size \(7\) of input is not within the configured batch sizes"):
        e.getEvaluation([[[0.0]]] * 7)


def test_deep_supervisor_example_configuration():
    """examples/learning/supervised/sineWave/run-deep-supervisor.py: an output activation, an output
    scale and a Target Loss, Max Generations cut to 5"""
    import korali

    rs = np.random.RandomState(0xC0FFEE)
    x = rs.uniform(0, 2 * np.pi, 500)
    y = np.tanh(np.exp(np.sin(x))) * 5.0
    e = ffn(korali, x, y, 5, steps=200, lr=0.0001)
    e["Solver"]["Neural Network"]["Output Activation"] = "Elementwise/Tanh"
    e["Solver"]["Neural Network"]["Output Layer"]["Scale"] = [5.0]
    e["Solver"]["Termination Criteria"]["Target Loss"] = 1e-3
    korali.Engine().run(e)
    assert e["Current Generation"] == 5 and np.isfinite(e["Solver"]["Current Loss"])
    out = np.asarray(e.getEvaluation([[[float(v)]] for v in x[:100]]))
    assert out.shape == (100, 1) and np.all(np.abs(out) <= 5.0)


def test_initial_hyperparameters_are_the_restatements_draws():
    """Learning Rate 0: Adam leaves the hyperparameters where they were drawn.  The network's generator
    takes the experiment's seed counter: the Random Seed itself here (no other generator before it)."""
    import korali

    rs = np.random.RandomState(1)
    x, y = sine(16, rs)
    e = ffn(korali, x, y, 1, steps=1, lr=0.0, seed=4242, ni=16)
    e["Solver"]["Neural Network"]["Hidden Layers"][2]["Weight Scaling"] = 0.5
    e["Solver"]["Output Weights Scaling"] = 0.25
    korali.Engine().run(e)
    layers = [dict(l) for l in LAYERS]
    layers[2]["Weight Scaling"], layers[4]["Weight Scaling"] = 0.5, 0.25
    assert np.array_equal(theta_of(e), SR.initial_hyperparameters(1, layers, 4242))


def test_a_second_run_continues_the_first():
    import korali

    rs = np.random.RandomState(2)
    x, y = sine(64, rs)
    a = ffn(korali, x, y, 2, steps=5, ni=64)
    k = korali.Engine()
    k.run(a)
    first = theta_of(a)
    a["Solver"]["Termination Criteria"]["Max Generations"] = 5
    k.run(a)
    b = ffn(korali, x, y, 5, steps=5, ni=64)
    korali.Engine().run(b)
    assert a["Current Generation"] == 5 and not np.array_equal(first, theta_of(a))
    assert np.array_equal(theta_of(a), theta_of(b))
    assert a["Solver"]["Current Loss"] == b["Solver"]["Current Loss"]


def test_a_resumed_run_starts_a_fresh_optimizer(tmp_path):
    import korali

    rs = np.random.RandomState(3)
    x, y = sine(64, rs)
    a = ffn(korali, x, y, 2, steps=3, ni=64)
    a["File Output"]["Enabled"] = True
    a["File Output"]["Path"] = str(tmp_path)
    korali.Engine().run(a)
    theta = theta_of(a)
    r = korali.Experiment()
    assert r.loadState(os.path.join(str(tmp_path), "latest"))
    assert np.array_equal(theta_of(r), theta)
    r["Solver"]["Steps Per Generation"] = 1
    r["Solver"]["Termination Criteria"]["Max Generations"] = 3
    r["File Output"]["Enabled"] = False
    korali.Engine().run(r)
    got = theta_of(r)
    assert r["Current Generation"] == 3 and not np.array_equal(got, theta)
    # the same step on a learner of its own, loaded with the file's hyperparameters and zero moments,
    # where every stage can be read: forward, backward and the Adam step each lie within the bounds of
    # tests/vracer_f64.py's model of their float64 restatement (teacher-forced, as in
    # test_gpu_supervisor.py), and the resumed run's step is that step bit for bit
    from test_gpu_supervisor import assert_within, check_pass, device

    X, S = x[:, None].astype(f32), y[:, None].astype(f32)
    dev = device(1, LAYERS, 1, 64, NI=64, learning_rate=0.005)
    dev.set_training_data(X, S)
    vals, _ = check_pass(dev, 1, LAYERS, 1, 64, theta, X)
    G = (S - vals[-1]).astype(f32)  # one IEEE subtraction: the device's bits
    _, grad = check_pass(dev, 1, LAYERS, 1, 64, theta, X, G)
    dev.train(1)
    assert np.array_equal(dev.get("gradient"), grad)
    zero = np.zeros_like(theta)
    _, _, step = F.adam(theta, grad, zero, zero, f64(f32(0.005)), f32(0.9), f32(0.999), None)
    assert_within("the first step from zero moments", got, step)
    assert np.array_equal(got, dev.hyperparameters)
    dev.close()
    # the continued optimizer (moments of six steps) would have moved differently
    c = ffn(korali, x, y, 2, steps=3, ni=64)
    k = korali.Engine()
    k.run(c)
    c["Solver"]["Steps Per Generation"] = 1
    c["Solver"]["Termination Criteria"]["Max Generations"] = 3
    k.run(c)
    assert not np.array_equal(theta_of(c), got)
