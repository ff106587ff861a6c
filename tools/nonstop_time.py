#!/usr/bin/env python
"""What nonstop humans cost the closed loop per lock-step step: `VectorExplorer.run_k_episodes(k, "test")` for k test cases with
H ORCA humans, the device scene generator and the MPRL policy of depth 2 / width 2 with action clipping (the setting of
profiles/explore_device.txt), with SimConfig.nonstop_human off or on.  One process measures ONE configuration (a warm-up run, then
--repeat timed runs of the same cases), so that two builds of the library can be alternated process by process with
RGL_HIP_LIBRARY; wall time is the host clock from the call to a device synchronise after it.  With --nonstop 1 an untimed run
afterwards counts the regenerations per episode and the share of (environment, step) pairs of live environments in which some human
arrived, that is, in which the wave brought the stream's words into LDS.
usage: nonstop_time.py [--nonstop 0|1] [--exploration host|device] [--episodes 2048] [--humans 5] [--repeat 1]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relationalgraphlearning_amd as rga  # noqa: E402
from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig  # noqa: E402
from tests.helpers import make_mprl_policy  # noqa: E402


class CountingSim(BatchedCrowdSim):
    """Adds up, on the device, the regenerations and the (live environment, step) pairs with an arrival."""

    def step(self, *args, **kw):
        live = self.done == 0
        out = BatchedCrowdSim.step(self, *args, **kw)
        hit = self.last_attempts > 0
        self.regenerations = getattr(self, "regenerations", 0) + hit.sum()
        self.touched = getattr(self, "touched", 0) + (hit.any(1) & live).sum()
        self.live_steps = getattr(self, "live_steps", 0) + live.sum()
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nonstop", type=int, default=0)
    ap.add_argument("--exploration", default="host")
    ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--humans", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda:0")
    k = args.episodes
    pol = make_mprl_policy("trained", D=2, w=2, clip=True, device=dev)
    over = {"nonstop_human": True} if args.nonstop else {}          # a build without the switch can still measure "off"
    cfg = SimConfig(human_num=args.humans, scene_generator="device", **over)
    ex = rga.VectorExplorer(BatchedCrowdSim(dev, cfg, human_policy="orca"), pol, gamma=0.9, exploration=args.exploration)
    label = args.label or ("nonstop %s, exploration %s" % ("on" if args.nonstop else "off", args.exploration))
    for rep in range(-1, args.repeat):
        ex.case_counter["test"] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ex.run_k_episodes(k, "test")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = max(ex.last_run["length"])
        print("%-40s %-4s %6d steps %9.4f s %10.4f ms per step" % (label, "warm" if rep < 0 else str(rep), steps, dt, dt / steps * 1e3))
    if args.nonstop:
        sim = CountingSim(dev, cfg, human_policy="orca")
        count = rga.VectorExplorer(sim, pol, gamma=0.9, exploration=args.exploration)
        count.run_k_episodes(k, "test")
        print("%-40s %.2f regenerations per episode; some human arrived in %.2f %% of %d (live environment, step) pairs"
              % (label, float(sim.regenerations) / k, 100.0 * float(sim.touched) / float(sim.live_steps), int(sim.live_steps)))


if __name__ == "__main__":
    main()
