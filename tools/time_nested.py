#!/usr/bin/env python3
"""Device time of Sampler/Nested per stage, and its generation rate.

  stages   L = 4096, N = 32, B = 1024, Ellipse, the gaussian kernel: HIP-event
           time of "bounds", "draw", "evaluate" and "select" per call
           (kg_nested_profile), and the wall time of a generation
  rate     the defaults, L = 1500, B = 1 (N = 3): generations per second; a
           generation there is a handful of small launches and two host
           synchronisations, i.e. launch-bound

Prints one JSON line.  Usage: python tools/time_nested.py [--generations G]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from korali_amd.native import NestedDevice  # noqa: E402

STAGES = ("bounds", "draw", "evaluate", "select")


def stage_times(generations):
    dev = NestedDevice(32, 4096, -5.0, 5.0, batch_size=1024, method="Ellipse", proposal_update_frequency=4096,
                       uniform_seed=1, normal_seed=2)
    dev.first_generation()
    for g in range(2, 5):  # warm-up: the first bounds update, the window's growth
        dev.generation(g)
    dev.synchronize()
    dev.profile(True)
    for s in STAGES:
        dev.profile_read(s)
    t0 = time.perf_counter()
    for g in range(5, 5 + generations):
        dev.generation(g)
    dev.synchronize()
    wall = time.perf_counter() - t0
    out = {"generation_ms": 1e3 * wall / generations, "windows_last": dev.diagnostics()[0],
           "tries_last": dev.diagnostics()[1], "accepted": float(dev["Accepted Samples"][0])}
    for s in STAGES:
        ms, n = dev.profile_read(s)
        out[s + "_ms"] = ms / n if n else 0.0
        out[s + "_calls"] = n
    dev.close()
    return out


def default_rate(generations):
    dev = NestedDevice(3, 1500, -5.0, 5.0, uniform_seed=1, normal_seed=2)
    dev.first_generation()
    for g in range(2, 52):
        dev.generation(g)
    dev.synchronize()
    t0 = time.perf_counter()
    for g in range(52, 52 + generations):
        dev.generation(g)
    dev.synchronize()
    wall = time.perf_counter() - t0
    dev.close()
    return generations / wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=50)
    a = ap.parse_args()
    print(json.dumps({"stages_L4096_N32_B1024_ellipse": stage_times(a.generations),
                      "generations_per_s_defaults": default_rate(40 * a.generations)}))


if __name__ == "__main__":
    main()
