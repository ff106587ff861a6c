#!/usr/bin/env python
"""What filling the replay memory costs beside collecting the episodes: `VectorExplorer.run_k_episodes(k, "train", update_memory=True)`
with fresh device-generated scenes, once with `ReplayMemory` (the per-tuple `update_memory` loop) and once with `DeviceReplayMemory`
(`push_episodes`, one library call per chunk), in ONE process on one MI355X.  Per configuration three host-clock figures, each ending
in a device synchronise: the episodes (reset to the chunk's last read-back, statistics included), the fill (first fill call to the end
of the run) and the trainer's first `as_tensors()`; and the push's three launches alone, event-timed (median of --repeat calls on the
recorded chunk).  The episodes are the imitation-learning phase's (crowd_nav/train.py:143-155): the ORCA expert drives the robot
among ORCA humans, and the tuples are stored in the target policy's layout -- MPRL's six fields or path G's rotated rows -- for H = 5
and 19, k = 256 and 2 048.  A warm-up run of 64 episodes per configuration and memory precedes the timed one.
usage: replay_fill_time.py [--episodes 256 2048] [--humans 5 19] [--repeat 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relationalgraphlearning_amd as rga  # noqa: E402
from relationalgraphlearning_amd.orca import OrcaPolicy  # noqa: E402
from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig  # noqa: E402
from tests.helpers import make_gcn_policy, make_mprl_policy  # noqa: E402


class TimedExplorer(rga.VectorExplorer):
    """Marks the moment the first fill call of a run starts (the device is idle then: _run_chunk ends in read-backs) and keeps the
    recorded chunk."""

    def run_k_episodes(self, *args, **kwargs):
        self.fill_start, self.recorded = None, None
        return super().run_k_episodes(*args, **kwargs)

    def _mark(self):
        if self.fill_start is None:
            self.fill_start = time.perf_counter()

    def update_memory(self, *args, **kwargs):
        self._mark()
        return super().update_memory(*args, **kwargs)

    def _push_chunk(self, run, imitation_learning):
        self._mark()
        self.recorded = run
        return super()._push_chunk(run, imitation_learning)


def timed_run(ex, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ex.run_k_episodes(k, "train", update_memory=True, imitation_learning=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    start = ex.fill_start if ex.fill_start is not None else t1
    fields = ex.memory.as_tensors()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert fields is not None
    return start - t0, t1 - start, t2 - t1


def push_alone(ex, layout, kinematics, repeat):
    """The library call on the recorded chunk into a scratch memory: event-timed median, and the host time of the call."""
    run = ex.recorded
    robot, humans, rewards, info = run["recorded"]
    scratch = rga.DeviceReplayMemory(ex.memory.capacity)
    ms, host = [], []
    for _ in range(repeat + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h0 = time.perf_counter()
        e0.record()
        scratch.push_episodes(robot, humans, rewards, info, layout, kinematics, 0.9 ** 0.25, True, lengths=run["lengths"],
                              outcomes=run["outcome"])
        e1.record()
        host.append(time.perf_counter() - h0)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms[3:])), float(np.median(host[3:])) * 1e3, int(robot.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, nargs="+", default=[256, 2048])
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 19])
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=100000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda:0")
    print("run_k_episodes(k, 'train', update_memory=True, imitation_learning=True): ORCA expert, ORCA humans, device scene generator, "
          "capacity %d; seconds, host clock to a device synchronise" % args.capacity)
    print("%-5s %3s %5s  %-8s %8s  %9s %9s %11s  %9s" % ("path", "H", "k", "memory", "tuples", "episodes", "fill", "as_tensors",
                                                        "us/tuple"))
    for which in ("mprl", "gcn"):
        for H in args.humans:
            pol = make_mprl_policy("trained", 1, device=dev) if which == "mprl" else make_gcn_policy(device=dev)
            expert = OrcaPolicy(safety_space=0.15)
            explorers = {}
            for name, cls in (("host", rga.ReplayMemory), ("device", rga.DeviceReplayMemory)):
                cfg = SimConfig(human_num=H, scene_generator="device")
                cfg.scene_max_attempts *= 8          # one 19-human train case in a few thousand passes the default cap
                sim = BatchedCrowdSim(dev, cfg, human_policy="orca")
                explorers[name] = TimedExplorer(sim, expert, memory=cls(args.capacity), gamma=0.9, target_policy=pol)
                explorers[name].run_k_episodes(64, "train", update_memory=True, imitation_learning=True)      # warm-up
                explorers[name].memory.as_tensors()
            for k in args.episodes:
                fills = {}
                for name in ("host", "device"):
                    ex = explorers[name]
                    ex.memory.clear()
                    t_ep, t_fill, t_stack = timed_run(ex, k)
                    n = len(ex.memory)
                    fills[name] = t_fill + t_stack
                    print("%-5s %3d %5d  %-8s %8d  %9.4f %9.4f %11.4f  %9.2f" % (which, H, k, name, n, t_ep, t_fill, t_stack,
                                                                              (t_fill + t_stack) / max(n, 1) * 1e6))
                ms, host_ms, T = push_alone(explorers["device"], which, pol.kinematics or "holonomic", args.repeat)
                print("%-5s %3d %5d  push_episodes alone on the recorded chunk (T = %d): %.3f ms on the device (events), %.3f ms of host "
                      "time per call; fill + as_tensors host / device = %.0fx" % (which, H, k, T, ms, host_ms,
                                                                                 fills["host"] / max(fills["device"], 1e-9)))
            same = all(torch.equal(a, b) for a, b in zip(explorers["host"].memory.as_tensors(), explorers["device"].memory.as_tensors()))
            print("%-5s %3d        the two memories of the last run are %s" % (which, H, "bit-identical" if same else "DIFFERENT"))


if __name__ == "__main__":
    main()
