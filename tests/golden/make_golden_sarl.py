"""Fixture generator for SARL / OM-SARL (build container only: imports the upstream reference through ref_loader).

Writes tests/golden/sarl.npz: one default-initialised weight set at the shipped widths (stored once), the scaling of attention.4 that
makes the attention sharp, and per case what UPSTREAM computes: the occupancy maps of the next human states, the rows of
`transform`, `action_values`, the chosen action and `get_attention_weights()`.  The variants (input_dim 13 / 29 / 45, no global state)
load column slices of mlp1.0.weight / attention.0.weight into upstream's network.  Arrays and short tag strings only.

    python tests/golden/make_golden_sarl.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_loader  # noqa: E402

policy_factory = ref_loader.load_reference()

from crowd_nav.configs.icra_benchmark.sarl import PolicyConfig  # noqa: E402
from crowd_sim.envs.utils.state import FullState, ObservableState, JointState  # noqa: E402
from crowd_sim.envs.utils.action import ActionXY  # noqa: E402

from tests import sarl_cpu as cpu  # noqa: E402  (scene generator, action table and layer names only)

WEIGHT_SEED = 20
SHARP_SCALE = 256.0


def make_policy(kinematics, input_dim, with_global_state):
    pc = PolicyConfig()
    pc.action_space.kinematics = kinematics
    pc.action_space.query_env = False
    pc.sarl.with_om = input_dim != 13
    pc.sarl.with_global_state = with_global_state
    pc.om.cell_num, pc.om.cell_size, pc.om.om_channel_size = 4, 1, max(1, (input_dim - 13) // 16)
    pol = policy_factory["sarl"]()
    pol.configure(pc)
    pol.set_phase("test")
    pol.set_device(torch.device("cpu"))
    pol.time_step = cpu.DT
    return pol


def joint_state(robot, humans):
    return JointState(FullState(*[float(x) for x in robot]), [ObservableState(*[float(x) for x in h]) for h in humans])


def special_scene(tag):
    robot, humans = cpu.scenes(77, 1, 5)
    robot, humans = robot[0], humans[0]
    if tag == "resting":
        humans[1, 2:4] = 0.0                        # arctan2(0, 0) = 0: its frame is the world's
    elif tag == "shared":                           # humans 1 and 2 in one cell of human 0's grid, all three moving alike
        humans[0, 2:4] = humans[1, 2:4] = humans[2, 2:4] = (0.5, 0.0)
        humans[1, :2] = humans[0, :2] + (0.2, 0.6)
        humans[2, :2] = humans[0, :2] + (0.9, 0.1)
    elif tag == "outside":                          # humans 3 and 4 beyond everybody's 4 m grid
        humans[3, :2] = (9.0, 9.5)
        humans[4, :2] = (-9.5, 8.0)
    return robot, humans


def main():
    torch.manual_seed(WEIGHT_SEED)
    master = make_policy("holonomic", 61, True)
    msd = {k: v.detach().clone() for k, v in master.model.state_dict().items()}
    out = {"weights." + k: v.numpy().astype(np.float32) for k, v in msd.items()}
    out["sharp_scale"] = np.float64(SHARP_SCALE)

    def variant_sd(input_dim, gs, wset):
        sd = {k: v.clone() for k, v in msd.items()}
        sd["mlp1.0.weight"] = sd["mlp1.0.weight"][:, :input_dim].contiguous()
        if not gs:
            sd["attention.0.weight"] = sd["attention.0.weight"][:, :100].contiguous()
        if wset == "sharp":
            sd["attention.4.weight"] = sd["attention.4.weight"] * SHARP_SCALE
            sd["attention.4.bias"] = sd["attention.4.bias"] * SHARP_SCALE
        return sd

    cases = []
    for H in (2, 5, 7, 20):
        for kin in ("holonomic", "unicycle"):
            cases.append(("h%d_%s" % (H, kin[:4]), kin, H, 61, True, "plain", 100 + H))
    for D, gs in ((13, True), (29, True), (45, True), (61, False), (13, False)):
        cases.append(("d%d_g%d" % (D, gs), "holonomic", 5, D, gs, "plain", 200 + D))
    for H in (5, 7, 20):
        cases.append(("sharp_h%d" % H, "holonomic", H, 61, True, "sharp", 300 + H))
    cases.append(("sharp_noglobal", "unicycle", 5, 61, False, "sharp", 310))
    for tag in ("resting", "shared", "outside"):
        cases.append((tag, "holonomic", 5, 61, True, "plain", None))
        cases.append((tag + "_c2", "holonomic", 5, 45, True, "plain", None))

    lines = []
    for ci, (tag, kin, H, D, gs, wset, seed) in enumerate(cases):
        pol = make_policy(kin, D, gs)
        pol.model.load_state_dict(variant_sd(D, gs, wset))
        if seed is None:
            robot, humans = special_scene(tag.split("_")[0])
        else:
            robot, humans = cpu.scenes(seed, 1, H, kin)
            robot, humans = robot[0], humans[0]
        js = joint_state(robot, humans)
        pol.action_space = None
        action = pol.predict(js)
        table = np.asarray([[float(a[0]), float(a[1])] for a in pol.action_space])
        assert np.array_equal(table, cpu.action_table(kin, float(robot[7]))), "action tables differ"
        chosen = [i for i, a in enumerate(pol.action_space) if a == action][0]
        pre = "case%d." % ci
        out[pre + "robot"] = np.asarray(robot, np.float64)
        out[pre + "humans"] = np.asarray(humans, np.float64)
        out[pre + "action_values"] = np.asarray(pol.action_values, np.float64)
        out[pre + "chosen"] = np.int64(chosen)
        out[pre + "attention"] = np.asarray(pol.get_attention_weights(), np.float32)
        out[pre + "transform"] = pol.transform(js).numpy().astype(np.float32)
        if D != 13:
            nxt = [pol.propagate(h, ActionXY(h.vx, h.vy)) for h in js.human_states]
            out[pre + "maps_next"] = pol.build_occupancy_maps(nxt).numpy().astype(np.float32)
        lines.append("%s|%s|%d|%d|%d|%s" % (tag, kin, H, D, int(gs), wset))
        att = out[pre + "attention"]
        print("%-16s H=%2d D=%d chosen=%2d |V|max=%.3f att max %.3f min %.4f" % (tag, H, D, chosen, np.abs(out[pre + "action_values"]).max(),
                                                                                 att.max(), att.min()))
    out["cases"] = np.asarray(lines)

    # the H = 1 refusal with maps: what upstream raises
    pol = make_policy("holonomic", 61, True)
    robot, humans = cpu.scenes(5, 1, 1)
    try:
        pol.predict(joint_state(robot[0], humans[0]))
        raised = "none"
    except Exception as e:      # noqa: BLE001
        raised = type(e).__name__
    out["single_human_error"] = np.asarray(raised)
    print("H = 1 with maps raises", raised)
    np.savez_compressed(os.path.join(HERE, "sarl.npz"), **out)
    print("wrote sarl.npz, %d bytes" % os.path.getsize(os.path.join(HERE, "sarl.npz")))


if __name__ == "__main__":
    main()
