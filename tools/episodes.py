#!/usr/bin/env python
"""Closed loop on device: N seeded episodes in lock-step, the model-predictive policy deciding for every live environment
per step (predict_batch) and the batched simulator advancing them.  Reports episodes/s and decisions/s, and what scene
generation costs: `--phase train` takes fresh cases for every run (the explorer's training counter never repeats, so the
simulator's scene memo cannot help there), `--generator host|device|both` picks who generates them."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig, run_episodes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--humans", type=int, default=5)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--width", type=int, default=2)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--phase", choices=("train", "val", "test"), default="test")
    ap.add_argument("--generator", choices=("host", "device", "both"), default="host")
    ap.add_argument("--human-policy", choices=("linear", "orca"), default="linear")
    ap.add_argument("--scenario", choices=("circle_crossing", "square_crossing"), default="circle_crossing")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pol = bench.make_policy(args, dev)
    counter = [0]

    def next_cases(n):                                        # train: never the same case twice in this process
        if args.phase != "train":
            return [k % 1000 for k in range(n)]
        counter[0] += n
        return list(range(counter[0] - n, counter[0]))
    for gen in (("host", "device") if args.generator == "both" else (args.generator,)):
        env = BatchedCrowdSim(dev, SimConfig(human_num=args.humans, scenario=args.scenario, scene_generator=gen),
                              human_policy=args.human_policy)
        run_episodes(env, pol, args.phase, next_cases(64))    # warm-up
        torch.cuda.synchronize()
        cases = next_cases(args.episodes)
        t0 = time.perf_counter()
        env.reset(args.phase, cases)                          # host: sequential seeded rejection sampling (memoised afterwards)
        torch.cuda.synchronize()
        t_gen = time.perf_counter() - t0
        if args.phase == "train":
            cases = next_cases(args.episodes)                 # the timed run generates its own scenes, as training does
        t0 = time.perf_counter()
        st = run_episodes(env, pol, args.phase, cases)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = int(st["time"].max() / env.cfg.time_step)
        decisions = float((st["time"] / env.cfg.time_step).sum())
        print("scene generation on %s: %.4f s for %d distinct %s cases (%.0f cases/s)"
              % (gen, t_gen, len(set(cases)), args.phase, len(set(cases)) / t_gen))
        print("episodes %d  H=%d D=%d w=%d %s humans, %s scenes%s | wall %.2f s | %.0f episodes/s | %.3e decisions/s | %d lock-step "
              "steps | success %.2f collision %.2f timeout %.2f (random-init weights: rates are not a quality claim)"
              % (args.episodes, args.humans, args.depth, args.width, args.human_policy, gen,
                 " generated inside the run" if args.phase == "train" else " memoised before it", dt, args.episodes / dt,
                 decisions / dt, steps, st["success_rate"], st["collision_rate"], st["timeout_rate"]))


if __name__ == "__main__":
    main()
