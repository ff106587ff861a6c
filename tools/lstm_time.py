"""Times the LSTM-RL one-step search on the MI355X: 2 048 roots x 81 actions, with and without the interaction module, at H = 5 and
H = 19, per launch of lstm_predict_f32 (sort, prepare, maps, weight layout, value network, selection), HIP events after a warm-up
of every timed shape.

    python tools/lstm_time.py [--roots 2048] [--humans 5 19] [--om] [--reps 50] [--out FILE] [--no-torch]

--om times OM-LSTM-RL (61-wide rows with three-channel maps) instead of the shipped default without maps (13-wide rows).

Reports per launch: time, the FLOPs the value kernel executes (its padded 16-row tiles and 4-wide k-steps, counted from the shapes
below), that rate as a fraction of the f32 MFMA peak (157.3 TFLOP/s) for the whole search and for the module's forward alone
(lstm_value_f32 on the same rows), and the FLOPs the network needs unpadded.  The yardstick is the same network composed from torch
operators on the same device and rows -- mlp1, nn.LSTM (the device's own recurrent kernels), the head -- plus the selection; the
parent commit has no LSTM-RL to compare with.  Medians of three alternated rounds.  One JSON line per (network, H)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from relationalgraphlearning_amd import LstmRL  # noqa: E402
from relationalgraphlearning_amd.config import policy_config  # noqa: E402
from relationalgraphlearning_amd.rollout import prepare_scenes, occupancy_maps  # noqa: E402
from tools.sarl_time import scenes, timed  # noqa: E402

PEAK_F32_MFMA = 157.3e12
DT = 0.25


def flops_per_scene(H, input_dim, interact, padded=False):
    """2 x multiply-adds of one sequence of H rows; padded: what the kernel's tiles execute (16-feature input tiles, 13 gate tiles of
    16 rows, h as 13 k-steps of 4, no recurrent product at the first step)."""
    def up(n):
        return -(-n // 16) * 16 if padded else n
    gates = 208 if padded else 200
    x = 50 if interact else input_dim
    step = up(x) * gates
    if interact:
        step += up(input_dim) * up(150) + up(150) * up(100) + up(100) * up(100) + up(100) * up(50)
    rec = (52 if padded else 50) * gates
    joint = (16 + 52) if padded else 56
    head = joint * up(150) + up(150) * up(100) + up(100) * up(100) + up(100) * (16 if padded else 1)
    return 2 * (H * step + (H - 1 if padded else H) * rec + head)


def torch_value_network(model, rows):
    """lstm_rl.py:9-69 from torch operators on the device (all sequences of full length)."""
    S, H, D = rows.shape
    x = model.mlp1(rows.reshape(S * H, D)).reshape(S, H, -1) if model.with_interaction_module else rows
    _, (hn, _) = model.lstm(x)
    return model.mlp(torch.cat([rows[:, 0, :6], hn[0]], dim=1))[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=2048)
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 19])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--om", action="store_true", help="OM-LSTM-RL: rows with occupancy maps")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstm_time.py measures on the MI355X; no device found")
    dev = torch.device("cuda:0")
    lines = []
    for interact in (True, False):
        torch.manual_seed(0)
        pol = LstmRL()
        pol.configure(policy_config("lstm_rl", lstm_rl__with_om=args.om, lstm_rl__with_interaction_module=interact))
        D = pol.input_dim()
        pol.set_phase("test")
        pol.set_device(dev)
        pol.time_step = DT
        pol.build_action_space(1.0)
        search = pol.gcn_search()
        A = len(pol.action_space)
        for H in args.humans:
            robot, humans = scenes(args.roots, H)
            r64, h64 = torch.tensor(robot, device=dev), torch.tensor(humans, device=dev)
            r32, h32 = r64.float(), h64.float()
            S = args.roots * A
            with torch.no_grad():
                search.search(r32, h32, roots64=(r64, h64))
                order = search.last_order.long()
                s64 = torch.gather(h64, 1, order[:, :, None].expand(-1, -1, 5)).contiguous()      # the humans as the search sorts them
                self6, hum7, reward = prepare_scenes(r32, s64.float(), search.actions_np, "holonomic", DT, roots64=(r64, s64))
                parts = [self6[:, None, :].expand(S, H, 6), hum7]
                if D > 13:
                    maps = occupancy_maps(s64, 4, 1.0, 3, time_step=DT)
                    parts.append(maps[:, None].expand(args.roots, A, H, 48).reshape(S, H, 48))
                rows = torch.cat(parts, dim=2).contiguous()
                del parts
                disc = 0.9 ** (DT * 1.0)

                def ours():
                    search.search(r32, h32, roots64=(r64, h64))

                def ours_value_only():
                    pol.model(rows)

                def composed():
                    v = torch_value_network(pol.model, rows)
                    vals = reward.reshape(args.roots, A).double() + disc * v.reshape(args.roots, A).double()
                    return vals, vals.argmax(dim=1)

                fns = [ours, ours_value_only] + ([] if args.no_torch else [composed])
                for fn in fns:
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                times = {fn: [] for fn in fns}      # alternated, so that all see the same neighbours on the machine
                for _ in range(3):
                    for fn in fns:
                        times[fn].append(timed(fn, args.reps))
                vals, best = search.search(r32, h32, roots64=(r64, h64))
                if not args.no_torch:
                    tv, tb = composed()
                    agree = float((best.long() == tb).float().mean())
                    dv = float((vals.double() - tv).abs().max())
            med = lambda t: float(np.median([x[0] for x in t]))      # noqa: E731
            t_ours, t_val, t_torch = times[ours], times[ours_value_only], times.get(composed)
            executed, needed = flops_per_scene(H, D, interact, padded=True) * S, flops_per_scene(H, D, interact) * S
            line = {"interaction_module": interact, "roots": args.roots, "actions": A, "H": H, "input_dim": D, "scenes": S,
                    "search_ms": med(t_ours), "search_ms_min_max": [min(x[1] for x in t_ours), max(x[2] for x in t_ours)],
                    "value_forward_ms": med(t_val), "executed_gflop": executed / 1e9, "needed_gflop": needed / 1e9,
                    "search_fraction_of_f32_mfma_peak": executed / (med(t_ours) * 1e-3) / PEAK_F32_MFMA,
                    "value_forward_fraction_of_f32_mfma_peak": executed / (med(t_val) * 1e-3) / PEAK_F32_MFMA}
            if t_torch:
                line.update({"torch_composed_ms": med(t_torch),
                             "torch_ms_min_max": [min(x[1] for x in t_torch), max(x[2] for x in t_torch)],
                             "speedup_over_torch": med(t_torch) / med(t_ours), "same_action_fraction": agree,
                             "max_value_difference": dv})
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
