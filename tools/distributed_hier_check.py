"""One rank of the Distributed conduit check for Hierarchical/Psi
(tests/test_gpu_hier.py launches it with torch.distributed.run): the Psi
experiment on the Distributed conduit (chains sharded, every rank evaluating
the likelihood of its pending chains on the device), then the same experiment
unsharded on the Sequential conduit, after 1 and after 3 generations; the
solver states go to <out>/rank<r>.json.

    distributed_hier_check.py <out dir> Host|RCCL
"""
import json
import os
import sys

import numpy as np

import korali

KEYS = ["Sample Database", "Sample LogLikelihood Database", "Sample LogPrior Database", "Annealing Exponent",
        "LogEvidence", "Chain Leaders", "Covariance Matrix", "Model Evaluation Count", "Accepted Samples Count"]


def sub_experiment(seed, rows):
    """A finished sampling experiment's result file, synthetic"""
    rng = np.random.default_rng(seed)
    return {"Is Finished": True, "Variables": [{"Name": "X0"}, {"Name": "X1"}],
            "Solver": {"Sample Database": np.stack([rng.normal(0.3 * seed, 1.2, rows),
                                                    np.exp(rng.normal(0.1, 0.5, rows))], axis=1).tolist(),
                       "Sample LogPrior Database": rng.uniform(-4.0, -1.0, rows).tolist(),
                       "Sample LogLikelihood Database": rng.uniform(-9.0, -1.0, rows).tolist()}}


def experiment(gens):
    e = korali.Experiment()
    e["Random Seed"] = 777
    e["File Output"]["Enabled"] = False
    e["Console Output"]["Verbosity"] = "Silent"
    e["Problem"]["Type"] = "Hierarchical/Psi"
    for i, rows in enumerate((70, 257, 33)):
        e["Problem"]["Sub Experiments"][i] = sub_experiment(i + 1, rows)
    e["Problem"]["Conditional Priors"] = ["Conditional 0", "Conditional 1"]
    bounds = [(-3.0, 3.0), (0.2, 4.0), (-2.0, 2.0), (0.2, 3.0)]
    for i, (lo, hi) in enumerate(bounds):
        e["Variables"][i]["Name"] = "Psi %d" % i
        e["Variables"][i]["Prior Distribution"] = "Uniform %d" % i
        e["Distributions"][i]["Name"] = "Uniform %d" % i
        e["Distributions"][i]["Type"] = "Univariate/Uniform"
        e["Distributions"][i]["Minimum"] = lo
        e["Distributions"][i]["Maximum"] = hi
    for c, (t, a, b) in enumerate((("Univariate/Normal", "Mean", "Standard Deviation"),
                                   ("Univariate/LogNormal", "Mu", "Sigma"))):
        e["Distributions"][4 + c]["Name"] = "Conditional %d" % c
        e["Distributions"][4 + c]["Type"] = t
        e["Distributions"][4 + c][a] = "Psi %d" % (2 * c)
        e["Distributions"][4 + c][b] = "Psi %d" % (2 * c + 1)
    e["Solver"]["Type"] = "Sampler/TMCMC"
    e["Solver"]["Population Size"] = 300
    e["Solver"]["Max Chain Length"] = 2
    e["Solver"]["Burn In"] = 1
    e["Solver"]["Termination Criteria"]["Max Generations"] = gens
    return e


def state(e):
    return {k: e["Solver"][k] for k in KEYS} | {"Current Generation": e["Current Generation"]}


def main():
    out, transport = sys.argv[1:3]
    rank = int(os.environ["RANK"])
    result = {}
    for gens in (1, 3):
        k = korali.Engine()
        k["Conduit"]["Type"] = "Distributed"
        k["Conduit"]["Transport"] = transport
        e = experiment(gens)
        k.run(e)
        u = experiment(gens)
        korali.Engine().run(u)
        result[str(gens)] = {"sharded": state(e), "unsharded": state(u)}
    with open(os.path.join(out, "rank%d.json" % rank), "w") as f:
        json.dump(result, f)
    print("DISTRIBUTED_HIER_CHECK rank %d done" % rank, flush=True)


if __name__ == "__main__":
    main()
