"""Per-stage device time of Optimizer/MOCMAES (kg_mocmaes_profile_read) at
N = 128 variables, P = 4096 offspring, mu = 2048 parents, K = 2 objectives,
with the builtin negative_rosenbrock_and_sphere kernel.

  draw        parent pick, the parents' factors, the normals and the draw chain
  evaluate    the objective kernel
  sort        rank peeling and the hypervolume order over the 2P merged values
  update      success rates, paths, covariances and step sizes (the stream over
              P N^2 doubles read from the parents and P N^2 written: its share
              of the HBM peak is printed beside it)
  parents     the gather of the mu selected rows
  statistics  best values, standard deviations, the non-dominated set and the
              archive merge

Warm-up generations first, then the median over the measured ones; stage
times are HIP events on the handle's stream (the host's waits inside a stage
count).

  python tools/time_mocmaes.py [--generations G] [--warmup W] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, P, MU, K = 128, 4096, 2048, 2
STAGES = ["draw", "evaluate", "sort", "update", "parents", "statistics"]
HBM_PEAK = 8.0e12  # bytes/s, the MI355X's HBM3E peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    from korali_amd.native import MocmaesDevice
    dev = MocmaesDevice(N, P, [-25.0] * N, [25.0] * N, mu=MU, num_objectives=K, initial_sdev=[3.0] * N,
                        multinormal_seed=1, uniform_seed=2)
    times = {s: [] for s in STAGES}
    for g in range(1, a.warmup + a.generations + 1):
        dev.profile(g > a.warmup)
        dev.generation(g, "negative_rosenbrock_and_sphere")
        dev.synchronize()
        if g > a.warmup:
            for s in STAGES:
                ms, n = dev.profile_read(s)
                if n:
                    times[s].append(ms)
    out = {"N": N, "P": P, "mu": MU, "K": K, "generations": a.generations,
           "median_ms": {s: statistics.median(v) for s, v in times.items() if v}}
    upd = out["median_ms"].get("update")
    if upd:
        out["update_bytes"] = 2 * P * N * N * 8
        out["update_hbm_share"] = out["update_bytes"] / (upd * 1e-3) / HBM_PEAK
    for s in STAGES:
        if s in out["median_ms"]:
            print("%-11s %9.3f ms" % (s, out["median_ms"][s]))
    if upd:
        print("update: %.2f GB algorithmic, %.1f %% of the %.1f TB/s HBM peak" %
              (out["update_bytes"] / 1e9, 100 * out["update_hbm_share"], HBM_PEAK / 1e12))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
