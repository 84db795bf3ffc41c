"""Learner/DeepSupervisor through korali.Engine, the part that needs no GPU:
the configuration is parsed and checked before any device call, so every
configuration error is reported on a CPU-only machine, by message."""
import re

import pytest


def experiment(korali, n=4, ni=2, ic=1, oc=1, timesteps=1):
    e = korali.Experiment()
    e["Problem"]["Type"] = "Supervised Learning"
    if timesteps is not None:
        e["Problem"]["Max Timesteps"] = timesteps
    e["Problem"]["Training Batch Size"] = n
    e["Problem"]["Inference Batch Size"] = ni
    e["Problem"]["Input"]["Data"] = [[[0.1 * b + i for i in range(ic)]] for b in range(n)]
    e["Problem"]["Input"]["Size"] = ic
    e["Problem"]["Solution"]["Data"] = [[0.2 * b + i for i in range(oc)] for b in range(n)]
    e["Problem"]["Solution"]["Size"] = oc
    e["Solver"]["Type"] = "Learner/DeepSupervisor"
    e["Solver"]["Loss Function"] = "Mean Squared Error"
    e["Solver"]["Learning Rate"] = 0.01
    e["Solver"]["Neural Network"]["Engine"] = "OneDNN"
    e["Solver"]["Neural Network"]["Optimizer"] = "Adam"
    e["Solver"]["Neural Network"]["Hidden Layers"][0]["Type"] = "Layer/Linear"
    e["Solver"]["Neural Network"]["Hidden Layers"][0]["Output Channels"] = 3
    e["Solver"]["Neural Network"]["Hidden Layers"][1]["Type"] = "Layer/Activation"
    e["Solver"]["Neural Network"]["Hidden Layers"][1]["Function"] = "Elementwise/Tanh"
    e["Solver"]["Termination Criteria"]["Max Generations"] = 1
    e["File Output"]["Enabled"] = False
    e["Console Output"]["Verbosity"] = "Silent"
    e["Random Seed"] = 7
    return e


def fails(korali, e, message, k=None):
    with pytest.raises(RuntimeError, match=re.escape(message)):
        (k or korali.Engine()).run(e)


def set_path(e, path, value):
    node = e
    for k in path[:-1]:
        node = node[k]
    node[path[-1]] = value


H0 = ("Solver", "Neural Network", "Hidden Layers", 0)
H1 = ("Solver", "Neural Network", "Hidden Layers", 1)
OL = ("Solver", "Neural Network", "Output Layer")
CASES = [
    # SupervisedLearning::initialize and the shape the device path takes
    (("Problem", "Training Batch Size"), 0, "Empty input batch provided."),
    (("Problem", "Max Timesteps"), 0, "Incorrect max timesteps provided: 0."),
    (("Problem", "Input", "Size"), 0, "Empty input vector size provided."),
    (("Problem", "Solution", "Size"), 0, "Empty solution vector size provided."),
    (("Problem", "Max Timesteps"), 3, "recurrent networks are not provided"),
    (("Problem", "Inference Batch Size"), 0, "Batch size 1 is zero."),
    # SupervisedLearning::verifyData
    (("Problem", "Input", "Data"), [], "Empty input dataset provided."),
    (("Problem", "Solution", "Data"), [], "Empty solution dataset provided."),
    (("Problem", "Input", "Data"), [[[0.0]]] * 3, "Training Batch size 3  different than that of input data (4)."),
    (("Problem", "Input", "Data"), [[[0.0], [1.0]]] * 4,
     "More timesteps (2) provided in batch 0 than max specified in the configuration (1)."),
    (("Problem", "Input", "Data"), [[[0.0]], [[0.0, 1.0]], [[0.0]], [[0.0]]],
     "Vector size of timestep 1 input data 0 is inconsistent. Size: 2 - Expected: 1."),
    (("Problem", "Solution", "Data"), [[0.0]] * 5,
     "Training Batch size of solution data (5) is different than that of input data (4)."),
    (("Problem", "Solution", "Data"), [[0.0], [0.0], [0.0, 1.0], [0.0]],
     "Solution vector size of batch 2 is inconsistent. Size: 2 - Expected: 1."),
    # layers
    (H1 + ("Function",), "Elementwise/Clip", "'Elementwise/Clip' (layer 2) is not provided"),
    (H1 + ("Function",), "Elementwise/Swish", "Unrecognized value (Elementwise/Swish) provided for mandatory setting: ['Function']"),
    (H0 + ("Type",), "Layer/Convolution", "Layer type 'Layer/Convolution' (hidden layer 1) is not provided"),
    (H0 + ("Type",), "Layer/Deconvolution", "Layer type 'Layer/Deconvolution' (hidden layer 1) is not provided"),
    (H0 + ("Type",), "Layer/Pooling", "Layer type 'Layer/Pooling' (hidden layer 1) is not provided"),
    (H0 + ("Type",), "Layer/Recurrent/LSTM", "Layer type 'Layer/Recurrent/LSTM' (hidden layer 1) is not provided"),
    (H0 + ("Type",), "Layer/Recurrent/GRU", "Layer type 'Layer/Recurrent/GRU' (hidden layer 1) is not provided"),
    (H0 + ("Output Channels",), 0, "Node count for layer (1) should be larger than zero."),
    # the Output layer's sizes (output.cpp.base)
    (OL + ("Scale",), [1.0, 2.0], "Wrong number of output scaling factors passed to the neural network. Expected: 1, provided: 2."),
    (OL + ("Shift",), [1.0, 2.0], "Wrong number of output shift factors passed to the neural network. Expected: 1, provided: 2."),
    (OL + ("Transformation Mask",), ["Identity", "Tanh"], "Wrong size of transformation mask specified: 2, expected: 1."),
    (OL + ("Transformation Mask",), ["Cube"], "Wrong transformation mask specified: Cube for output variable 0."),
    # the solver's own settings
    (("Solver", "Neural Network", "Engine"), "TensorFlow", "Neural Network Engine 'TensorFlow' is not recognized"),
    (("Solver", "Neural Network", "Optimizer"), "SGD",
     "Unrecognized value (SGD) provided for mandatory setting: ['Neural Network']['Optimizer'] required by deepSupervisor."),
    (("Solver", "Loss Function"), "Cross Entropy",
     "Unrecognized value (Cross Entropy) provided for mandatory setting: ['Loss Function'] required by deepSupervisor."),
    (("Solver", "Hyperparameters"), [0.0] * 5, "'Hyperparameters' holds 5 values; the network has 10."),
    (("Solver", "Neural Network", "Output Activation"), "Elementwise/Clip", "'Elementwise/Clip'"),
    # unknown keys, at every level
    (("Solver", "Learning Rates"), 0.1, "Unrecognized settings for Korali module: deepSupervisor"),
    (("Solver", "Neural Network", "Optimiser"), "Adam", "Unrecognized settings for Korali module: deepSupervisor"),
    (("Solver", "L2 Regularization", "Weight"), 0.1, "Unrecognized settings for Korali module: deepSupervisor"),
    (("Solver", "Termination Criteria", "Target Lost"), 0.1, "Unrecognized settings for Korali module: deepSupervisor"),
    (H0 + ("Channels",), 3, "Unrecognized settings for Korali module: linear"),
    (H1 + ("Gamma",), 3, "Unrecognized settings for Korali module: activation"),
    (OL + ("Masks",), [], "Unrecognized settings for Korali module: output"),
    (("Problem", "Batch Size"), 3, "Unrecognized settings for Korali module: supervisedLearning"),
    (("Problem", "Input", "Sizes"), 3, "Unrecognized settings for Korali module: supervisedLearning"),
]


@pytest.mark.parametrize("path,value,message", CASES, ids=[f"{'/'.join(map(str, c[0]))}={c[1]}"[:60] for c in CASES])
def test_configuration_error(path, value, message):
    import korali

    e = experiment(korali)
    set_path(e, path, value)
    fails(korali, e, message)


@pytest.mark.parametrize("path,message", [
    (("Solver", "Neural Network", "Hidden Layers"), "['Neural Network']['Hidden Layers'] required by deepSupervisor."),
    (("Solver", "Neural Network", "Engine"), "['Neural Network']['Engine'] required by deepSupervisor."),
    (("Solver", "Neural Network", "Optimizer"), "['Neural Network']['Optimizer'] required by deepSupervisor."),
    (("Solver", "Loss Function"), "['Loss Function'] required by deepSupervisor."),
    (("Solver", "Learning Rate"), "['Learning Rate'] required by deepSupervisor."),
    (("Problem", "Training Batch Size"), "['Training Batch Size'] required by supervisedLearning."),
    (("Problem", "Inference Batch Size"), "['Inference Batch Size'] required by supervisedLearning."),
    (("Problem", "Input", "Size"), "['Input']['Size'] required by supervisedLearning."),
    (("Problem", "Solution", "Size"), "['Solution']['Size'] required by supervisedLearning."),
])
def test_mandatory_setting(path, message):
    import korali

    e = experiment(korali)
    set_path(e, path, None)
    fails(korali, e, " + No value provided for mandatory setting: " + message)


def test_distributed_conduit_is_not_provided(monkeypatch):
    import korali

    for v in ("RANK", "WORLD_SIZE"):
        monkeypatch.delenv(v, raising=False)
    k = korali.Engine()
    k["Conduit"]["Type"] = "Distributed"
    k["Conduit"]["Transport"] = "Host"  # one rank: no sockets
    fails(korali, experiment(korali), "Learner/DeepSupervisor does not shard across ranks", k)


def test_a_failed_first_run_leaves_no_learner_behind():
    """the corrected experiment starts afresh: it is not taken for a further run of a network built for
    other sizes (without a GPU the second run ends at device creation, with one it finishes)"""
    import korali

    e = experiment(korali)
    e["Problem"]["Training Batch Size"] = 5
    fails(korali, e, "Training Batch size 4  different than that of input data (5).")
    e["Problem"]["Training Batch Size"] = 4
    e["Solver"]["Neural Network"]["Hidden Layers"][0]["Output Channels"] = 6
    try:
        korali.Engine().run(e)
    except RuntimeError as err:
        msg = str(err)
        assert "changed between runs" not in msg, msg
        assert "hip" in msg.lower() or "device" in msg.lower() or "gpu" in msg.lower(), msg
    else:
        assert len(e["Solver"]["Hyperparameters"]) == 1 * 6 + 6 + 6 * 1 + 1


def test_other_problems_are_errors():
    import korali

    e = experiment(korali)
    e["Problem"]["Type"] = "Optimization"
    fails(korali, e, "Problems of type 'Optimization' are not supported by the Learner/DeepSupervisor solver")
    e = experiment(korali)
    e["Problem"]["Type"] = "Hierarchical/Psi"
    fails(korali, e, "are supported with the 'Sampler/TMCMC' solver")
    e = experiment(korali)
    e["Solver"]["Type"] = "Learner/GaussianProcess"
    fails(korali, e, "Agent/Discrete/dVRACER and Learner/DeepSupervisor)")


def test_defaults_are_written_back():
    """the module defaults of deepSupervisor.config and supervisedLearning.config, visible after the
    configuration was read (here: up to the data check, which fails last)"""
    import korali

    e = experiment(korali, timesteps=None)
    e["Problem"]["Solution"]["Data"] = []
    fails(korali, e, "Empty solution dataset provided.")
    sv = e["Solver"]
    assert sv["Steps Per Generation"] == 1
    assert sv["L2 Regularization"]["Enabled"] is False and sv["L2 Regularization"]["Importance"] == 1e-4
    assert sv["Neural Network"]["Output Activation"] == "Identity"
    assert sv["Termination Criteria"]["Target Loss"] == -1.0
    assert sv["Output Weights Scaling"] == 1.0
    assert len(sv["Hyperparameters"]) == 0
    assert e["Problem"]["Max Timesteps"] == 1


def test_get_evaluation_before_any_run():
    """Experiment::getEvaluation initializes the experiment first (experiment.cpp.base:221-222); a batch
    of neither configured size is refused with NeuralNetwork::getBatchSizeIdx's message before any
    device call"""
    import korali

    e = experiment(korali)
    with pytest.raises(RuntimeError, match=re.escape(
            "Batch size (3) of input is not within the configured batch sizes of the neural network..")):
        e.getEvaluation([[[0.0]]] * 3)
    bad = experiment(korali)
    bad["Solver"]["Loss Function"] = "Cross Entropy"
    with pytest.raises(RuntimeError, match="Unrecognized value \\(Cross Entropy\\)"):
        bad.getEvaluation([[[0.0]]] * 2)
    other = korali.Experiment()
    other["Solver"]["Type"] = "Optimizer/CMAES"
    with pytest.raises(RuntimeError, match="This solver does not support evaluation operations."):
        other.getEvaluation([[[0.0]]])
