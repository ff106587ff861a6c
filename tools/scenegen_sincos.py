#!/usr/bin/env python
"""The device's float64 sin / cos against numpy's (the host libm) on the accepted angles of the scene-generator tests' circle
cases: the measurement the tolerance K of tests/test_scenegen_gpu.py rests on.  Prints the largest deviation in units of 2**-52.
--angles FILE.npy reads the angles instead of regenerating them (a minute of host work), --save FILE.npy writes them (no GPU)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--angles")
    ap.add_argument("--save")
    args = ap.parse_args()
    if args.angles:
        angles = np.load(args.angles)
    else:
        from tests import scenegen_cpu as sg
        angles = np.array([a for _, cfg in sg.configurations() if cfg.scenario == "circle_crossing"
                           for phase, k in sg.cases_of(cfg) for a in sg.generate_scene_restated(cfg, phase, k)[4]["angles"]])
    if args.save:
        np.save(args.save, angles)
        print("%d angles saved" % angles.size)
        return
    import torch
    a = torch.as_tensor(angles, dtype=torch.float64, device="cuda:0")
    unit = 2.0 ** -52
    d_sin = np.abs(torch.sin(a).cpu().numpy() - np.sin(angles)) / unit
    d_cos = np.abs(torch.cos(a).cpu().numpy() - np.cos(angles)) / unit
    print("%d angles in [%.3g, %.3g]: |device - numpy| in units of 2**-52: sin max %.3f (%d differ), cos max %.3f (%d differ)"
          % (angles.size, angles.min(), angles.max(), d_sin.max(), int((d_sin > 0).sum()), d_cos.max(), int((d_cos > 0).sum())))


if __name__ == "__main__":
    main()
