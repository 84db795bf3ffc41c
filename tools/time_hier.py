"""Device time of the Hierarchical/Psi likelihood at the reference example's
shape (examples/hierarchical.bayesian, phase 2): P = 2000 candidates, 5
sub-experiments of 1000 samples, two conditional priors (Normal, LogNormal),
synthetic databases.

  ms per kg_tmcmc_evaluate round  HIP events around the call (stage "evaluate":
                                  the log-prior kernel + the likelihood),
  ms of the likelihood kernels    stage "hier_loglik" (k_hier_group + k_hier_finish),
  ms per generation               host clock around kg_tmcmc_generation + synchronize.

And of the Hierarchical/Theta likelihood at the example's phase 3b shape: P =
1000 candidates, the phase-2 result's M = 2000 Psi samples, the phase-1
result's K = 1000 sub-experiment samples, the same two conditional priors:

  ms of the denominator set-up    stage "theta_denominators" of
                                  kg_tmcmc_set_hierarchical_theta (k_hier_group's
                                  denominator mode + k_hier_finish), one fresh
                                  handle per sample,
  ms of one evaluation round      stage "hier_loglik" of kg_tmcmc_evaluate
                                  (k_hier_group's Theta mode + k_hier_finish).

Warm-up first, then the median of at least 20 samples each.  tools/hier_cpu_loop
(tools/hier_cpu_loop.cpp) times the same sums on one CPU core with libm.

  python tools/time_hier.py [--json out.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, G, K = 2000, 5, 1000


def handle(seed):
    from korali_amd.native import TmcmcDevice
    rng = np.random.default_rng(1)
    groups = [np.stack([0.3 * g + 1.5 * rng.standard_normal(K), np.exp(0.2 + 0.6 * rng.standard_normal(K))], axis=1)
              for g in range(G)]
    lps = [rng.uniform(-6.0, -1.0, K) for _ in range(G)]
    dev = TmcmcDevice(4, P, prior_min=[-2.0, 0.2, -1.0, 0.2], prior_max=[2.0, 3.0, 1.0, 2.0],
                      prior_seeds=[seed, seed + 1, seed + 2, seed + 3], multinomial_seed=seed + 4,
                      multivariate_seed=seed + 5, uniform_seed=seed + 6)
    dev.set_hierarchical("psi", ["normal", "lognormal"], [[0, 1], [2, 3]], [[0.0, 0.0], [0.0, 0.0]], groups, lps)
    return dev


TP, TM, TK = 1000, 2000, 1000


def theta_handle(seed, profile):
    from korali_amd.native import TmcmcDevice
    rng = np.random.default_rng(2)
    psi = np.stack([rng.uniform(-2.0, 2.0, TM), rng.uniform(0.2, 3.0, TM), rng.uniform(-1.0, 1.0, TM),
                    rng.uniform(0.2, 2.0, TM)], axis=1)
    sub = np.stack([1.5 * rng.standard_normal(TK), np.exp(0.2 + 0.6 * rng.standard_normal(TK))], axis=1)
    dev = TmcmcDevice(2, TP, prior_min=[-4.0, 0.1], prior_max=[4.0, 5.0], prior_seeds=[seed, seed + 1],
                      multinomial_seed=seed + 4, multivariate_seed=seed + 5, uniform_seed=seed + 6)
    dev.profile(profile)
    dev.set_hierarchical_theta(["normal", "lognormal"], [[0, 1], [2, 3]], [[0.0, 0.0], [0.0, 0.0]], psi, sub,
                               rng.uniform(-6.0, -1.0, TK))
    return dev


def theta(samples):
    theta_handle(5, False).close()  # warm-up: the code object, the allocator's blocks
    den = []
    for i in range(samples):
        d = theta_handle(200 + 10 * i, True)
        ms, n = d.profile_read("theta_denominators")
        assert n == 1
        den.append(ms)
        if i + 1 < samples:
            d.close()
    d.profile(False)
    d.prepare(1)
    for _ in range(5):
        d.evaluate()
    d.synchronize()
    d.profile(True)
    hk = []
    for _ in range(samples):
        d.evaluate()
        d.synchronize()
        ms, n = d.profile_read("hier_loglik")
        assert n == 1
        hk.append(ms)
    d.close()
    out = {"theta_P": TP, "theta_psi_rows": TM, "theta_sub_rows": TK,
           "theta_denominators_ms_median": statistics.median(den), "theta_denominators_ms_min": min(den),
           "theta_denominators_ms_max": max(den), "theta_round_ms_median": statistics.median(hk),
           "theta_round_ms_min": min(hk), "theta_round_ms_max": max(hk)}
    exe = os.path.join(ROOT, "tools", "hier_cpu_loop")
    if os.path.exists(exe):
        out.update(json.loads(subprocess.check_output([exe, "theta", str(TP), str(TM), str(TK), "5"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--samples", type=int, default=25)
    a = ap.parse_args()
    dev = handle(10)
    dev.prepare(1)
    for _ in range(5):  # warm-up
        dev.evaluate()
    dev.synchronize()
    dev.profile(True)
    ev, hk = [], []
    for _ in range(a.samples):
        dev.evaluate()
        dev.synchronize()
        ms, n = dev.profile_read("evaluate")
        assert n == 1
        ev.append(ms)
        ms, n = dev.profile_read("hier_loglik")
        assert n == 1
        hk.append(ms)
    dev.profile(False)
    gens, seed = [], 100
    while len(gens) < a.samples:
        d = handle(seed)
        seed += 10
        for g in range(1, 40):
            t0 = time.perf_counter()
            d.generation(g)
            d.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            if g > 1:  # generation 1 carries the first-use costs
                gens.append(dt)
            if d["Previous Annealing Exponent"][0] >= 1.0:
                break
        d.close()
    out = {"P": P, "groups": G, "rows_per_group": K, "conditional_priors": 2,
           "evaluate_ms_median": statistics.median(ev), "evaluate_ms_min": min(ev), "evaluate_ms_max": max(ev),
           "hier_kernels_ms_median": statistics.median(hk), "hier_kernels_ms_min": min(hk),
           "hier_kernels_ms_max": max(hk), "generation_ms_median": statistics.median(gens),
           "generation_ms_min": min(gens), "generation_ms_max": max(gens), "samples": a.samples,
           "generation_samples": len(gens)}
    exe = os.path.join(ROOT, "tools", "hier_cpu_loop")
    if os.path.exists(exe):
        out.update(json.loads(subprocess.check_output([exe, str(P), str(G), str(K), "5"])))
    out.update(theta(a.samples))
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
