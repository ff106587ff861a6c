"""Device time of ORCA: crowd_orca_humans_f64 alone for B = 4096 at H = 5 and H = 20, and one BatchedCrowdSim step with
human_policy="orca" against a "linear" step (B = 4096, H = 5).  HIP events around REPS back-to-back calls after WARM warm-up
calls; the median of 5 such windows is reported, per call, in microseconds.  One JSON line per measurement.

    python tools/orca_time.py [--reps 200] [--out profiles/orca_time.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relationalgraphlearning_amd.orca import orca_human_velocities  # noqa: E402
from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig  # noqa: E402


def timed(fn, reps, warm=20, windows=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / reps)
    return float(np.median(per)), float(min(per)), float(max(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = 4096
    rows = []
    for H in (5, 20):
        sim = BatchedCrowdSim(dev, SimConfig(human_num=H), human_policy="orca")
        sim.reset("test", list(range(B)))
        out = torch.empty(B, H, 2, dtype=torch.float64, device=dev)
        med, lo, hi = timed(lambda: orca_human_velocities(sim.robot, sim.humans, sim.human_goals, out=out), a.reps)
        rows.append(dict(what="crowd_orca_humans_f64", B=B, H=H, us_per_call=med, us_min=lo, us_max=hi, reps=a.reps))
    for policy in ("linear", "orca"):
        sim = BatchedCrowdSim(dev, SimConfig(time_limit=1e9), human_policy=policy)
        sim.reset("test", list(range(B)))
        act = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        med, lo, hi = timed(lambda: sim.step(act), a.reps)       # the robot stands still: every environment stays live
        rows.append(dict(what="BatchedCrowdSim.step", human_policy=policy, B=B, H=5, us_per_call=med, us_min=lo, us_max=hi,
                         reps=a.reps, note="host-side wrapper included (ctypes, output tensors, observe)"))
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
