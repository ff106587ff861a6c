"""Times one SARL / OM-SARL optimisation step on the MI355X: a batch of 100 replay rows, D = 61, global state, at H = 5 and H = 19.

    python tools/sarl_train_time.py [--batch 100] [--humans 5 19] [--reps 200] [--out FILE]

Sides, all in this process on the same rows and weights:
  hip      SarlValueNetwork after enable_training(): sarl_value_train_f32 + sarl_value_backward_f32 behind autograd, recorded into
           a hipGraph the way VNRLTrainer records its step; `hip_step` IS the trainer's own captured imitation-learning step
           (forward, fused loss, backward, fused Adam, repack), replayed.
  torch    the same network composed from torch operators with torch autograd (tools/sarl_time.py's torch_value_network), eager and
           captured the same way; `*_step` adds the same fused capturable Adam.
The yardstick of the HIP path is the captured torch composition, never the HIP path itself.  Method of tools/sarl_time.py: every
side is warmed up for at least 40 ms, then five alternated runs of --reps steps each, timed per step with HIP events; a line
reports the median of the five medians and their spread (the smallest and the largest).  One JSON line per H."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from relationalgraphlearning_amd import SARL, VNRLTrainer, ReplayMemory  # noqa: E402
from relationalgraphlearning_amd.config import policy_config  # noqa: E402
from sarl_time import torch_value_network, timed  # noqa: E402


def captured(fn):
    """fn recorded into a hipGraph after three real runs on a side stream; returns the replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def warm(fn, seconds=0.04):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()


class _Writer(object):
    def add_scalar(self, *a, **k):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 19])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sarl_train_time.py measures on the MI355X; no device found")
    dev = torch.device("cuda:0")
    lines = []
    for H in args.humans:
        torch.manual_seed(0)
        pol = SARL()
        pol.configure(policy_config("sarl", sarl__with_om=True, sarl__with_global_state=True))
        pol.set_device(dev)
        pol.model.to(dev)
        D, S = pol.input_dim(), args.batch
        rng = np.random.RandomState(H)
        rows = torch.tensor(rng.uniform(-2, 2, (S, H, D)).astype(np.float32), device=dev)
        target = torch.tensor(rng.uniform(0, 1, (S, 1)).astype(np.float32), device=dev)

        def forward_backward(net, forward):
            def fn():
                for p in net.parameters():
                    p.grad = None
                out = forward(net)
                out.backward((2.0 / S) * (out.detach() - target))
            return fn

        def with_adam(net, forward):
            opt = torch.optim.Adam(net.parameters(), lr=1e-3, capturable=True, fused=True)
            fb = forward_backward(net, forward)

            def fn():
                fb()
                opt.step()
            return fn

        def hip_forward(net):
            return net(rows)

        def torch_forward(net):
            return torch_value_network(net, rows)[0].unsqueeze(1)

        hip_net = copy.deepcopy(pol.model).enable_training()
        torch_net, torch_net_adam = copy.deepcopy(pol.model), copy.deepcopy(pol.model)
        # (i) the trainer's own captured step: one batch of S items, imitation learning
        memory = ReplayMemory(S)
        for i in range(S):
            memory.push((rows[i], target[i], target[i], rows[i]))
        trainer = VNRLTrainer(copy.deepcopy(pol.model), memory, dev, pol, S, "Adam", _Writer())
        trainer.set_learning_rate(1e-3)
        trainer.optimize_epoch(2)                          # the first step captures, the second replays
        assert trainer._capturable and len(trainer._steps) == 1
        step = next(iter(trainer._steps.values()))
        with torch.enable_grad():
            sides = {"hip_fwd_bwd_captured": captured(forward_backward(hip_net, hip_forward)),
                     "hip_step_captured": step.graph.replay,
                     "torch_fwd_bwd_eager": forward_backward(torch_net, torch_forward),
                     "torch_fwd_bwd_captured": captured(forward_backward(copy.deepcopy(pol.model), torch_forward)),
                     "torch_step_eager": with_adam(torch_net_adam, torch_forward),
                     "torch_step_captured": captured(with_adam(copy.deepcopy(pol.model), torch_forward))}
            for fn in sides.values():
                warm(fn)
            medians = {k: [] for k in sides}
            for _ in range(5):                              # alternated: every side sees the same neighbours on the machine
                for k, fn in sides.items():
                    medians[k].append(timed(fn, args.reps)[0])
        line = {"batch": S, "H": H, "input_dim": D, "reps": args.reps}
        for k, m in medians.items():
            line[k + "_ms"] = float(np.median(m))
            line[k + "_ms_spread"] = [float(min(m)), float(max(m))]
        line["hip_over_torch_captured_fwd_bwd"] = line["hip_fwd_bwd_captured_ms"] / line["torch_fwd_bwd_captured_ms"]
        line["hip_over_torch_captured_step"] = line["hip_step_captured_ms"] / line["torch_step_captured_ms"]
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
