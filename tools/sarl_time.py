"""Times the SARL / OM-SARL one-step search on the MI355X: 2 048 roots x 81 actions at H = 5 and H = 19 (--dense: 30, 50 and 127),
per launch of sarl_predict_f32 (prepare, maps, weight layout, value network, selection), HIP events after a warm-up of every timed
shape.

    python tools/sarl_time.py [--roots 2048] [--humans 5 19 | --dense] [--no-om] [--reps 200] [--out FILE]
                              [--no-torch] [--no-value-forward] [--maps-only]

--no-om times SARL without occupancy maps (13-wide rows); --maps-only times sarl_occupancy_maps_f32 alone (three channels), which an
older build of the library (RGL_HIP_LIBRARY) can be asked for at any H; --no-torch / --no-value-forward leave out the comparison
lines (an older build has no sarl_value_workspace_bytes_for for the module's forward).

Reports per launch: time, the FLOPs the value kernel executes (its padded 16-wide tiles, counted from the shapes below), that rate
as a fraction of the f32 MFMA peak (157.3 TFLOP/s), and the FLOPs the network needs unpadded.  The comparison line is the same
module composed from torch operators on the same device and tensors (the value network of sarl.py:28-73 on the rows the search's
own first steps wrote, plus the selection) -- the parent commit has no SARL to compare with.  One JSON line per H."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from relationalgraphlearning_amd import SARL  # noqa: E402
from relationalgraphlearning_amd.config import policy_config  # noqa: E402
from relationalgraphlearning_amd.rollout import prepare_scenes, occupancy_maps  # noqa: E402

PEAK_F32_MFMA = 157.3e12
DT = 0.25


DENSE = [30, 50, 127]


def flops_per_scene(H, input_dim=61, with_global_state=True, padded=False):
    """2 x multiply-adds of one scene; padded: widths rounded up to the kernel's 16-feature tiles."""
    def up(n):
        return -(-n // 16) * 16 if padded else n
    att_in = (2 if with_global_state else 1) * up(100)
    per_human = (up(input_dim) * up(150) + up(150) * up(100) + up(100) * up(100) + up(100) * up(50)
                 + att_in * up(100) + up(100) * up(100) + up(100) * (16 if padded else 1))
    joint = (16 + up(50)) if padded else 56
    head = joint * up(150) + up(150) * up(100) + up(100) * up(100) + up(100) * (16 if padded else 1)
    return 2 * (H * per_human + head)


def scenes(B, H, seed=0):
    rng = np.random.RandomState(seed)
    robot = np.zeros((B, 9))
    robot[:, :2] = rng.uniform(-4, 4, (B, 2))
    robot[:, 2:4] = rng.uniform(-0.5, 0.5, (B, 2))
    robot[:, 4], robot[:, 7] = 0.3, 1.0
    robot[:, 5:7] = -robot[:, :2]
    humans = np.zeros((B, H, 5))
    humans[:, :, :2] = robot[:, None, :2] * 0.5 + rng.uniform(-3, 3, (B, H, 2))
    humans[:, :, 2:4] = rng.uniform(-1, 1, (B, H, 2))
    humans[:, :, 4] = 0.3
    return robot, humans


def torch_value_network(model, rows):
    """sarl.py:28-73 from torch operators on the device."""
    S, H, D = rows.shape
    y = model.mlp1(rows.reshape(S * H, D))
    feat = model.mlp2(y).reshape(S, H, -1)
    if model.with_global_state:
        mean = y.reshape(S, H, -1).mean(dim=1, keepdim=True).expand(S, H, y.shape[1]).reshape(S * H, -1)
        att_in = torch.cat([y, mean], dim=1)
    else:
        att_in = y
    scores = model.attention(att_in).reshape(S, H)
    w = torch.softmax(scores, dim=1)
    joint = torch.cat([rows[:, 0, :6], (w.unsqueeze(2) * feat).sum(dim=1)], dim=1)
    return model.mlp3(joint)[:, 0], w


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=2048)
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 19])
    ap.add_argument("--reps", type=int, default=200)     # a timed window of 0.4 s (our value forward at H = 5) to 4 s
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dense", action="store_true", help="H = 30, 50, 127 instead of --humans")
    ap.add_argument("--no-om", action="store_true", help="SARL without occupancy maps")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-value-forward", action="store_true")
    ap.add_argument("--maps-only", action="store_true")
    args = ap.parse_args()
    if args.dense:
        args.humans = DENSE
    if not torch.cuda.is_available():
        raise SystemExit("sarl_time.py measures on the MI355X; no device found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pol = SARL()
    pol.configure(policy_config("sarl", sarl__with_om=not args.no_om))
    D = pol.input_dim()
    pol.set_phase("test")
    pol.set_device(dev)
    pol.time_step = DT
    pol.build_action_space(1.0)
    search = pol.gcn_search()
    A = len(pol.action_space)
    lines = []
    for H in args.humans:
        robot, humans = scenes(args.roots, H)
        r64, h64 = torch.tensor(robot, device=dev), torch.tensor(humans, device=dev)
        r32, h32 = r64.float(), h64.float()
        S = args.roots * A

        def maps_alone():
            occupancy_maps(h64, 4, 1.0, 3, time_step=DT)

        for _ in range(args.warmup):
            maps_alone()
        torch.cuda.synchronize()
        t_maps = [timed(maps_alone, args.reps) for _ in range(3)]
        maps_ms = float(np.median([x[0] for x in t_maps]))
        if args.maps_only:
            line = {"roots": args.roots, "H": H, "maps_ms": maps_ms, "maps_ms_min_max": [min(x[1] for x in t_maps), max(x[2] for x in t_maps)]}
            print(json.dumps(line), flush=True)
            lines.append(line)
            continue
        with torch.no_grad():
            self6, hum7, reward = prepare_scenes(r32, h32, search.actions_np, "holonomic", DT, roots64=(r64, h64))
            parts = [self6[:, None, :].expand(S, H, 6), hum7]
            if D > 13:
                maps = occupancy_maps(h64, 4, 1.0, 3, time_step=DT)
                parts.append(maps[:, None].expand(args.roots, A, H, 48).reshape(S, H, 48))
            rows = torch.cat(parts, dim=2).contiguous()
            del parts
            disc = 0.9 ** (DT * 1.0)

            def ours():
                search.search(r32, h32, roots64=(r64, h64))

            def ours_value_only():
                pol.model(rows)

            def composed():
                v, w = torch_value_network(pol.model, rows)
                vals = reward.reshape(args.roots, A).double() + disc * v.reshape(args.roots, A).double()
                best = vals.argmax(dim=1)
                return vals, best, w.reshape(args.roots, A, H)[torch.arange(args.roots, device=dev), best]

            fns = [ours] + ([] if args.no_value_forward else [ours_value_only]) + ([] if args.no_torch else [composed])
            for fn in fns:
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            # alternate them so that all see the same neighbours on the machine
            times = {fn: [] for fn in fns}
            for _ in range(3):
                for fn in fns:
                    times[fn].append(timed(fn, args.reps))
            t_ours, t_val, t_torch = times[ours], times.get(ours_value_only), times.get(composed)
            vals, best = search.search(r32, h32, roots64=(r64, h64))
            if t_torch:
                tv, tb, _ = composed()
                agree = float((best.long() == tb).float().mean())
                dv = float((vals.double() - tv).abs().max())
        med = lambda t: float(np.median([x[0] for x in t]))      # noqa: E731
        executed, needed = flops_per_scene(H, D, padded=True) * S, flops_per_scene(H, D) * S
        line = {"roots": args.roots, "actions": A, "H": H, "input_dim": D, "scenes": S,
                "search_ms": med(t_ours), "search_ms_min_max": [min(x[1] for x in t_ours), max(x[2] for x in t_ours)],
                "maps_ms": maps_ms, "executed_gflop": executed / 1e9, "needed_gflop": needed / 1e9,
                "search_fraction_of_f32_mfma_peak": executed / (med(t_ours) * 1e-3) / PEAK_F32_MFMA}
        if t_val:
            line.update({"value_forward_ms": med(t_val),
                         "value_forward_fraction_of_f32_mfma_peak": executed / (med(t_val) * 1e-3) / PEAK_F32_MFMA})
        if t_torch:
            line.update({"torch_composed_ms": med(t_torch),
                         "torch_ms_min_max": [min(x[1] for x in t_torch), max(x[2] for x in t_torch)],
                         "speedup_over_torch": med(t_torch) / med(t_ours), "same_action_fraction": agree, "max_value_difference": dv})
        del rows
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
