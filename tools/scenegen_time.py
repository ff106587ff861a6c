#!/usr/bin/env python
"""Kernel time of the device scene generator for a batch of fresh train cases: as given, and sorted by draw count (the launch is
lock-step per case only, but a workgroup slot is held as long as its case runs), with the draws histogram.  Event-timed, median
of --repeat launches after a warm-up."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from relationalgraphlearning_amd.sim import SimConfig, _launch_scene_generator  # noqa: E402


def timed(cfg, cases, dev, repeat):
    ms = []
    for _ in range(repeat + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = _launch_scene_generator(cfg, "train", cases, dev)
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms[1:])), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2048)
    ap.add_argument("--first", type=int, default=100000)
    ap.add_argument("--humans", type=int, default=19)
    ap.add_argument("--scenario", default="circle_crossing")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-attempts", type=int, default=None)
    ap.add_argument("--tail", type=int, default=0, help="instead: the draws distribution of this many cases, in launches of --cases")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = SimConfig(human_num=args.humans, scenario=args.scenario)
    if args.max_attempts:
        cfg.scene_max_attempts = args.max_attempts
    if args.tail:
        draws, flagged = [], 0
        for lo in range(args.first, args.first + args.tail, args.cases):
            out = _launch_scene_generator(cfg, "train", list(range(lo, lo + args.cases)), dev)
            ok = out[4].cpu().numpy() == 0
            flagged += int((~ok).sum())
            draws.append(out[5].cpu().numpy()[ok])
        draws = np.concatenate(draws)
        print("%s H=%d, %d train cases from %d, cap %d attempts per human: %d flagged; draws of the others: median %d  p99 %d  "
              "p99.9 %d  p99.99 %d  max %d" % ((args.scenario, args.humans, args.tail, args.first, cfg.scene_max_attempts, flagged)
                                              + tuple(np.percentile(draws, [50, 99, 99.9, 99.99, 100]).astype(np.int64))))
        for x in (30000, 100000, 300000, 1000000, 3000000):
            print("  more than %7d draws: %d cases" % (x, int((draws > x).sum())))
        return
    cases = list(range(args.first, args.first + args.cases))
    ms, out = timed(cfg, cases, dev, args.repeat)
    draws = out[5].cpu().numpy()
    order = np.argsort(-draws, kind="stable")
    ms_sorted, _ = timed(cfg, [cases[i] for i in order], dev, args.repeat)
    print("%s H=%d, %d train cases from %d: launch %.3f ms as given, %.3f ms sorted by draws (longest first), %.0f cases/s"
          % (args.scenario, args.humans, args.cases, args.first, ms, ms_sorted, args.cases / ms * 1e3))
    q = np.percentile(draws, [0, 25, 50, 75, 90, 99, 100]).astype(int)
    print("draws per case: min %d  p25 %d  median %d  p75 %d  p90 %d  p99 %d  max %d  mean %.0f  total %d" % (tuple(q) + (draws.mean(), draws.sum())))
    edges = [0, 100, 300, 1000, 3000, 10000, 30000, 100000, 1 << 30]
    hist, _ = np.histogram(draws, edges)
    print("histogram: " + "  ".join("<%s: %d" % (("%d" % e) if e < (1 << 30) else "inf", n) for e, n in zip(edges[1:], hist)))


if __name__ == "__main__":
    main()
