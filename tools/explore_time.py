#!/usr/bin/env python
"""What epsilon-greedy exploration costs a training run per lock-step step, on the host and on the device:
`VectorExplorer.run_k_episodes(k, "train", update_memory=True)` for k fresh train cases with `exploration="host"` (two numpy draws
of length B, two host-to-device copies, a `where` and a `table[idx]` gather per step) and `exploration="device"` (one
crowd_explore_select_f64 launch per step, one crowd_explore_seed_u32 launch per chunk), alternated in ONE process on one MI355X.
ORCA humans, device scene generator, DeviceReplayMemory, MPRL policy of depth 2 / width 2 with action clipping, epsilon 0.5.
Both modes run the same cases in every repetition (they explore differently, so the episodes and their step counts differ);
a warm-up run of both precedes the timed ones.  Wall time is the host clock from the call to a device synchronise after it.
usage: explore_time.py [--episodes 2048] [--humans 5] [--repeat 5]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relationalgraphlearning_amd as rga  # noqa: E402
from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig  # noqa: E402
from tests.helpers import make_mprl_policy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--humans", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--epsilon", type=float, default=0.5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda:0")
    k = args.episodes
    pol = make_mprl_policy("trained", D=2, w=2, clip=True, device=dev)
    pol.set_epsilon(args.epsilon)
    explorers = {}
    for mode in ("host", "device"):
        sim = BatchedCrowdSim(dev, SimConfig(human_num=args.humans, scene_generator="device"), human_policy="orca")
        explorers[mode] = rga.VectorExplorer(sim, pol, memory=rga.DeviceReplayMemory(100000), gamma=0.9, target_policy=pol,
                                             exploration=mode)
    print("run_k_episodes(%d, 'train', update_memory=True): MPRL depth 2 / width 2, epsilon %.2f, H = %d ORCA humans, device scene "
          "generator, DeviceReplayMemory; seconds, host clock to a device synchronise" % (k, args.epsilon, args.humans))
    print("%-4s %-7s %6s %9s %12s %8s" % ("rep", "mode", "steps", "seconds", "ms per step", "tuples"))
    per_step = {"host": [], "device": []}
    for rep in range(-1, args.repeat):                   # -1: the warm-up of both
        for mode in ("host", "device"):
            ex = explorers[mode]
            ex.case_counter["train"] = (rep + 1) * k     # the same fresh cases for both modes
            ex.memory.clear()
            np.random.seed(rep + 1)                      # the host mode's stream, for what it is worth
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ex.run_k_episodes(k, "train", update_memory=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            steps = max(ex.last_run["length"])
            if rep >= 0:
                per_step[mode].append(dt / steps * 1e3)
            print("%-4s %-7s %6d %9.4f %12.4f %8d" % ("warm" if rep < 0 else str(rep), mode, steps, dt, dt / steps * 1e3, len(ex.memory)))
    med = {m: float(np.median(v)) for m, v in per_step.items()}
    print("median ms per step: host %.4f, device %.4f (device - host = %+.4f ms, %+.1f%%)"
          % (med["host"], med["device"], med["device"] - med["host"], (med["device"] / med["host"] - 1) * 100))


if __name__ == "__main__":
    main()
