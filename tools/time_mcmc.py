#!/usr/bin/env python3
"""Time of one Sampler/MCMC chain step on the device, and the engine's rate.

  steps    N in {1, 8, 64}, Use Adaptive Sampling off and on (Non Adaption
           Period 200, so the chain covariance has full rank when its factor
           takes over), Rejection Levels 1, the gaussian kernel: wall-clock
           microseconds per generation when kg_mcmc_run is called with windows
           of 1 and of 4096 generations, and the HIP-event time of the stages
           "window" (the stream windows), "chain" (k_mcmc_chain) and "consume"
           per launch (kg_mcmc_profile)
  engine   the recorded run's configuration (N = 1, Burn In 500, 5000 samples,
           5500 generations) through korali.Engine, no files, nothing printed:
           generations per second

Every figure is the mean of --repeats runs (default 3) of --generations
generations each (default 8192; windows of 1: a quarter of that), after a
warm-up run; the JSON line says so.  Usage: python tools/time_mcmc.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from korali_amd.native import McmcDevice  # noqa: E402

STAGES = ("window", "chain", "consume")
WARM = 512


def step_times(N, adaptive, window, generations, repeats):
    sd = np.full(N, 1.0 / np.sqrt(N))
    walls, stages = [], {s: [] for s in STAGES}
    for r in range(repeats):
        dev = McmcDevice(N, np.zeros(N), sd, use_adaptive_sampling=adaptive, non_adaption_period=200,
                         max_samples=WARM + generations + 1, normal_seed=11 + r, uniform_seed=21 + r)
        dev.run(1, WARM)  # warm-up: code objects, the adaptive switch
        dev.synchronize()
        dev.profile(True)
        for s in STAGES:
            dev.profile_read(s)
        g, t0 = WARM + 1, time.perf_counter()
        while g <= WARM + generations:
            n = min(window, WARM + generations + 1 - g)
            dev.run(g, n)
            g += n
        dev.synchronize()
        walls.append(1e6 * (time.perf_counter() - t0) / generations)
        for s in STAGES:
            ms, n = dev.profile_read(s)
            stages[s].append(1e3 * ms / n if n else 0.0)
        dev.close()
    out = {"us_per_step_wall": float(np.mean(walls))}
    for s in STAGES:
        out[s + "_us_per_launch"] = float(np.mean(stages[s]))
    return out


def engine_rate(repeats):
    import korali
    rates = []
    for r in range(repeats + 1):  # the first run warms up
        e = korali.Experiment()
        e["Random Seed"] = 1000 + r
        e["Problem"]["Type"] = "Sampling"
        e["Problem"]["Probability Kernel"] = "Gaussian"
        e["Variables"][0]["Name"] = "X"
        e["Variables"][0]["Initial Mean"] = 0.0
        e["Variables"][0]["Initial Standard Deviation"] = 1.0
        e["Solver"]["Type"] = "Sampler/MCMC"
        e["Solver"]["Burn In"] = 500
        e["Solver"]["Termination Criteria"]["Max Samples"] = 5000
        e["File Output"]["Enabled"] = False
        e["Console Output"]["Verbosity"] = "Silent"
        t0 = time.perf_counter()
        korali.Engine().run(e)
        if r:
            rates.append(5500 / (time.perf_counter() - t0))
    return float(np.mean(rates))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    out = {"mean_of_runs": a.repeats, "generations_per_run": {"window_4096": a.generations, "window_1": a.generations // 4}}
    for N in (1, 8, 64):
        for adaptive in (False, True):
            key = "N%d_%s" % (N, "adaptive" if adaptive else "fixed")
            out[key] = {"window_1": step_times(N, adaptive, 1, a.generations // 4, a.repeats),
                        "window_4096": step_times(N, adaptive, 4096, a.generations, a.repeats)}
    out["engine_recorded_configuration_generations_per_s"] = engine_rate(a.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
