#!/usr/bin/env python3
"""Device times of the discrete agent (Agent / Discrete / dVRACER) at the C5
shape: 4096 concurrent CartPole environments, 2 x 256 tanh, mini-batch 256,
Experiences Between Policy Updates 1, Possible Actions [[-10], [10]] (K = 2).

The replay memory is filled to its start size, then `--steps` training steps
run with the stage timers on (kg_vracer_profile: HIP events on the handle's
stream).  Prints one JSON line: the time per policy update ("update") and per
environment step ("environment_step"), and the experiences per second of the
timed steps.  `--continuous` times the continuous agent the same way.

    python tools/time_dvracer.py [--steps 5] [--warmup 2] [--continuous]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C5 = dict(environments=4096, hidden_size=256, hidden_layers=2, mini_batch_size=256, replay_maximum_size=262144,
          replay_start_size=131072, experiences_between_policy_updates=1.0, max_episode_steps=500,
          environment_count=3, discount_factor=0.99, learning_rate=1e-4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--continuous", action="store_true")
    args = ap.parse_args()
    from korali_amd.vracer import VracerDevice
    kw = dict(initial_exploration_noise=1.0) if args.continuous else dict(possible_actions=[[-10.0], [10.0]])
    d = VracerDevice(seed=1337, **C5, **kw)
    while d.scalar("experience_count") < C5["replay_start_size"]:
        d.training_step()
    for _ in range(args.warmup):
        d.training_step()
    d.synchronize()
    d.profile(True)
    exps, ups = 0, 0
    t0 = time.perf_counter()
    for _ in range(args.steps):
        n, u = d.training_step()
        exps, ups = exps + n, ups + u
    d.synchronize()
    elapsed = time.perf_counter() - t0
    out = {"agent": "continuous (Normal)" if args.continuous else "discrete (K = 2)", "steps": args.steps,
           "experiences": exps, "updates": ups, "experiences_per_s": exps / elapsed}
    for stage in ("update", "environment_step"):
        ms, cnt = d.profile_read(stage)
        out[stage + "_us"] = ms / cnt * 1e3 if cnt else None
        out[stage + "_count"] = cnt
    d.profile(False)
    d.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
