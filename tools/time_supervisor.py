#!/usr/bin/env python3
"""Time the DeepSupervisor device path (needs a GPU).

Large shape: batch 4096, input 64, three Tanh layers of 1024, 16 outputs,
Adam: ms per training step (median of 7 windows of 300 steps after warm-up,
the device path and PyTorch taking turns window by window), ms per stage
(forward, data gradient, weight gradient, optimizer; HIP events through
kg_supervisor_profile) and the achieved TF/s of each product family, beside
the same step in PyTorch FP32 on the same GPU (torch.nn.functional.linear,
autograd, torch.optim.Adam): an independent implementation of the same
arithmetic.  Small shape: the sine-wave example's network (batch 500, two
Tanh layers of 32), in steps per second; it is launch-bound.

Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from korali_amd.supervisor import SupervisorDevice  # noqa: E402

TANH = {"Type": "Layer/Activation", "Function": "Elementwise/Tanh"}


def network(hidden, outputs):
    layers = []
    for h in hidden:
        layers += [{"Type": "Layer/Linear", "Output Channels": h}, TANH]
    return layers + [{"Type": "Layer/Linear", "Output Channels": outputs}]


class DeviceRun:
    def __init__(self, I, hidden, O, B):
        rng = np.random.default_rng(0)
        self.w, self.B = [I] + hidden + [O], B
        w = self.w
        n = sum(w[i] * w[i + 1] + w[i + 1] for i in range(len(w) - 1))
        self.dev = SupervisorDevice(I, O, network(hidden, O), B, learning_rate=1e-4,
                                    hyperparameters=(rng.uniform(-1, 1, n) * 0.03).astype(np.float32))
        self.dev.set_training_data(rng.standard_normal((B, I)), rng.standard_normal((B, O)))

    def run(self, steps):
        self.dev.train(steps)  # returns after the last step's loss has been read

    def stages(self, steps):
        """ms per step of each stage (HIP events) and the TF/s of its products"""
        w, B = self.w, self.B
        self.dev.profile(True)
        self.dev.train(steps)
        st = {s: self.dev.profile_read(s)[0] / steps
              for s in ("forward", "data_gradient", "weight_gradient", "optimizer", "other")}
        self.dev.profile(False)
        flops = sum(2.0 * B * w[i] * w[i + 1] for i in range(len(w) - 1))
        dflops = sum(2.0 * B * w[i] * w[i + 1] for i in range(1, len(w) - 1))
        tf = {"forward": flops / st["forward"] / 1e9, "weight_gradient": flops / st["weight_gradient"] / 1e9,
              "data_gradient": dflops / st["data_gradient"] / 1e9 if st["data_gradient"] else 0.0}
        return st, tf


class TorchRun:
    def __init__(self, I, hidden, O, B):
        import torch

        self.torch = torch
        torch.backends.cuda.matmul.allow_tf32 = False
        g = torch.Generator(device="cuda").manual_seed(0)
        w = [I] + hidden + [O]
        self.P = []
        for i in range(len(w) - 1):
            self.P += [(torch.rand(w[i + 1], w[i], device="cuda", generator=g) * 0.06 - 0.03).requires_grad_(),
                       torch.zeros(w[i + 1], device="cuda", requires_grad=True)]
        self.X = torch.randn(B, I, device="cuda", generator=g)
        self.S = torch.randn(B, O, device="cuda", generator=g)
        self.B = B
        self.opt = torch.optim.Adam(self.P, lr=1e-4)

    def run(self, steps):
        import torch.nn.functional as Fn

        torch, P = self.torch, self.P
        for _ in range(steps):
            x = self.X
            for i in range(0, len(P), 2):
                x = Fn.linear(x, P[i], P[i + 1])
                if i + 2 < len(P):
                    x = torch.tanh(x)
            loss = ((self.S - x) ** 2).sum() / (2 * self.B)
            self.opt.zero_grad(set_to_none=True)
            loss.backward()
            self.opt.step()
        torch.cuda.synchronize()


def alternate(runs, steps, repeats, warmup):
    """seconds per step of each runner: all warmed up first, then `repeats` rounds in which the runners
    take turns, one window of `steps` steps each, so that clock and machine state are shared"""
    for r in runs:
        r.run(warmup)
    ts = [[] for _ in runs]
    for _ in range(repeats):
        for r, t in zip(runs, ts):
            t0 = time.perf_counter()
            r.run(steps)
            t.append((time.perf_counter() - t0) / steps)
    return ts


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())}


def main():
    # windows of 300 steps: about 0.3 s for the device path and 0.2 s for PyTorch at the large shape
    big = (64, [1024, 1024, 1024], 16, 4096)
    d = DeviceRun(*big)
    runs = [d]
    try:
        runs.append(TorchRun(*big))
    except Exception as ex:  # PyTorch is the yardstick, not a dependency
        print("PyTorch run not available: %s" % ex, file=sys.stderr)
    ts = alternate(runs, steps=300, repeats=7, warmup=100)
    stages, tf = d.stages(100)
    out = {"large": {"device": spread(ts[0]), "stage_ms": stages, "product_tflops": tf}}
    if len(runs) == 2:
        out["large"]["pytorch"] = spread(ts[1])
    d.dev.close()
    s = DeviceRun(1, [32, 32], 1, 500)
    ts = alternate([s], steps=2000, repeats=7, warmup=500)
    out["small"] = {"steps_per_second": float(1.0 / np.median(ts[0])), "spread": spread(ts[0])}
    s.dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
