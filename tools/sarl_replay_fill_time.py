#!/usr/bin/env python
"""What filling the replay memory with SARL / OM-SARL rows costs beside collecting the episodes: tools/replay_fill_time.py's
measurement for a SARL target.  `VectorExplorer.run_k_episodes(k, "train", update_memory=True, imitation_learning=True)` with the
ORCA expert among ORCA humans and an OM-SARL target after enable_training() (D = 61: 13 relation features and 4 x 4 x 3 map slots),
once with `ReplayMemory` -- the host loop of `update_memory`: per episode one rotate and one occupancy-map launch, per tuple two
torch.tensor calls and a push of four tensors -- and once with `DeviceReplayMemory` (`push_sarl_episodes`: rgl_replay_push_sarl_f32,
three launches per chunk), in ONE process on one MI355X.  Per run three host-clock figures, each ending in a device synchronise: the
episodes (reset to the chunk's last read-back, statistics included), the fill (first fill call to the end of the run) and the
trainer's first `as_tensors()`.  The two memories take turns --repeat times on fresh cases after a 64-episode warm-up of each; the
table shows the medians.  The push's three launches alone are event-timed on the last recorded chunk (median of --calls calls).
usage: sarl_replay_fill_time.py [--episodes 2048] [--humans 5 19] [--repeat 5] [--calls 20] [--input-dim 61]"""
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
from tools.replay_fill_time import TimedExplorer, timed_run  # noqa: E402


def make_policy(dev, input_dim):
    from relationalgraphlearning_amd.config import policy_config
    channels = (input_dim - 13) // 16
    pol = rga.SARL()
    pol.configure(policy_config("sarl", sarl__with_om=channels > 0, om__om_channel_size=channels or 3))
    pol.set_phase("train")
    pol.set_device(dev)
    pol.time_step = 0.25
    pol.enable_training()
    assert pol.input_dim() == input_dim
    return pol


def push_alone(ex, pol, calls):
    """The library call on the recorded chunk into a scratch memory: event-timed median, and the host time of the call."""
    run = ex.recorded
    robot, humans, rewards, info = run["recorded"]
    scratch = rga.DeviceReplayMemory(ex.memory.capacity)
    om = (pol.cell_num, pol.cell_size, pol.om_channel_size) if pol.with_om else None
    ms, host = [], []
    for _ in range(calls + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h0 = time.perf_counter()
        e0.record()
        scratch.push_sarl_episodes(robot, humans, rewards, info, pol.kinematics, 0.9 ** 0.25, True, om=om, lengths=run["lengths"],
                                   outcomes=run["outcome"])
        e1.record()
        host.append(time.perf_counter() - h0)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms[3:])), float(np.median(host[3:])) * 1e3, int(robot.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, nargs="+", default=[2048])
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 19])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--input-dim", type=int, default=61, choices=[13, 29, 45, 61])
    ap.add_argument("--capacity", type=int, default=100000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda:0")
    print("run_k_episodes(k, 'train', update_memory=True, imitation_learning=True): ORCA expert, ORCA humans, device scene generator, "
          "SARL target with D = %d, capacity %d; seconds, host clock to a device synchronise, medians of %d alternated runs"
          % (args.input_dim, args.capacity, args.repeat))
    print("%3s %5s  %-8s %8s  %9s %9s %11s  %9s  %s" % ("H", "k", "memory", "tuples", "episodes", "fill", "as_tensors", "us/tuple",
                                                       "fill share of the collection"))
    for H in args.humans:
        pol = make_policy(dev, args.input_dim)
        expert = OrcaPolicy(safety_space=0.15)
        explorers = {}
        for name, cls in (("host", rga.ReplayMemory), ("device", rga.DeviceReplayMemory)):
            cfg = SimConfig(human_num=H, scene_generator="device")
            cfg.scene_max_attempts *= 8          # one 19-human train case in a few thousand passes the default cap
            sim = BatchedCrowdSim(dev, cfg, human_policy="orca")
            explorers[name] = TimedExplorer(sim, expert, memory=cls(args.capacity), gamma=0.9, target_policy=pol)
            explorers[name].run_k_episodes(64, "train", update_memory=True, imitation_learning=True)      # warm-up
            explorers[name].memory.as_tensors()
        assert explorers["device"].recorded is not None and explorers["host"].recorded is None
        for k in args.episodes:
            runs = {"host": [], "device": []}
            for _ in range(args.repeat):
                for name in ("host", "device"):
                    ex = explorers[name]
                    ex.memory.clear()
                    runs[name].append(timed_run(ex, k) + (len(ex.memory),))
            fills = {}
            for name in ("host", "device"):
                t_ep, t_fill, t_stack, n = (float(np.median(x)) for x in zip(*runs[name]))
                fills[name] = t_fill + t_stack
                print("%3d %5d  %-8s %8d  %9.4f %9.4f %11.4f  %9.2f  %.1f %%" % (H, k, name, n, t_ep, t_fill, t_stack,
                                                                              (t_fill + t_stack) / max(n, 1) * 1e6,
                                                                              100 * (t_fill + t_stack) / (t_ep + t_fill + t_stack)))
            ms, host_ms, T = push_alone(explorers["device"], pol, args.calls)
            print("%3d %5d  push_sarl_episodes alone on the recorded chunk (T = %d): %.3f ms on the device (events), %.3f ms of host "
                  "time per call; fill + as_tensors host / device = %.0fx" % (H, k, T, ms, host_ms,
                                                                             fills["host"] / max(fills["device"], 1e-9)))
        # both explorers have seen the same train cases in the same order: the memories of the last run hold the same tuples
        same = all(torch.equal(a, b) for a, b in zip(explorers["host"].memory.as_tensors(), explorers["device"].memory.as_tensors()))
        print("%3d        the two memories of the last run are %s" % (H, "bit-identical" if same else "DIFFERENT"))


if __name__ == "__main__":
    main()
