"""Fixture generator for LSTM-RL / OM-LSTM-RL (build container only: imports the upstream reference through ref_loader).

Writes tests/golden/lstm.npz: one default-initialised weight set per network at input_dim 61 (`vn2.`: ValueNetwork2's mlp1, lstm and
mlp; `vn1.`: ValueNetwork1's lstm -- its head is vn2's mlp, loaded into it), the scale of the "saturated" LSTM tensors, and per case
what UPSTREAM computes ("saturated": weight_ih and the biases times 512, weight_hh times 8):
  network cases  ValueNetwork1 / ValueNetwork2 forward on recorded rows, without `lengths` (a batch of one), with strictly decreasing
                 lengths H..1 (a batch of H) and with all lengths equal;
  search cases   the humans sorted by decreasing distance to the robot HERE (LstmRL.predict reads `state.self_state`, a field
                 JointState does not have: the sort is its lines 103-107 with `robot_state` for that name), then upstream's
                 MultiHumanRL.predict on the sorted state: the order, `action_values`, the chosen action and `transform`'s rows.
  bulk cases     search cases on the first 16 roots of the scenes tests/test_lstm_gpu.py searches at B = 40 (H = 5 and 20, input_dim 13,
                 both networks, both weight sets), stored as the seed with the orders, `action_values` and the chosen actions: the
                 error of upstream's float32 has a long tail -- a gate whose pre-activation cancels to the linear range from terms
                 of several hundred -- and a bound measured on a few dozen roots understates what thousands of scenes reach.
The variants (input_dim 13 / 29 / 45) load column slices of the matrix that reads the rows.  Arrays and short tag strings only.

The distances a sort case compares are either far apart (asserted below) or equal by construction -- two humans at (x, y) and
(-x, y) from the robot, every coordinate a small dyadic number, so that dx dx + dy dy is the same double however the two products
and the sum are rounded.

    python tests/golden/make_golden_lstm.py
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

from crowd_nav.configs.icra_benchmark.config import BasePolicyConfig  # noqa: E402
from crowd_nav.policy.multi_human_rl import MultiHumanRL  # noqa: E402
from crowd_sim.envs.utils.state import FullState, ObservableState, JointState  # noqa: E402

from tests import sarl_cpu as cpu  # noqa: E402  (scene generator and action table only)
from tests.lstm_cpu import gpu_seed, BULK_B, BULK_ROOTS  # noqa: E402  (which scenes the GPU test searches)

WEIGHT_SEED = 21
SATURATED_SCALE = 512.0            # weight_ih and the two biases: pre-activations beyond 100
SATURATED_RECURRENT_SCALE = 8.0    # weight_hh: a common factor of 256 on it makes the recurrence chaotic -- upstream's own float32
                                   # forward then stands 4e-2 from float64 at H = 20 (|V| < 0.1), and a bound built on that is none
CELL = ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0"]


def make_policy(kinematics, input_dim, interact):
    pc = BasePolicyConfig()
    pc.action_space.kinematics = kinematics
    pc.action_space.query_env = False
    pc.lstm_rl.with_om = input_dim != 13
    pc.lstm_rl.with_interaction_module = interact
    pc.om.cell_num, pc.om.cell_size, pc.om.om_channel_size = 4, 1, max(1, (input_dim - 13) // 16)
    pol = policy_factory["lstm_rl"]()
    pol.configure(pc)
    pol.set_phase("test")
    pol.set_device(torch.device("cpu"))
    pol.time_step = cpu.DT
    return pol


def joint_state(robot, humans):
    return JointState(FullState(*[float(x) for x in robot]), [ObservableState(*[float(x) for x in h]) for h in humans])


def upstream_sort(js):
    """lstm_rl.py:103-107 with `robot_state` for `self_state`; returns the order as indices into the given list."""
    def dist(human):
        return np.linalg.norm(np.array(human.position) - np.array(js.robot_state.position))
    given = list(js.human_states)
    js.human_states = sorted(js.human_states, key=dist, reverse=True)
    return [[i for i, g in enumerate(given) if g is h][0] for h in js.human_states], [dist(h) for h in given]


def tie_scene():
    """Five humans; humans 1 and 3 mirror each other across the robot's vertical: the same distance, exactly."""
    robot, humans = cpu.scenes(78, 1, 5)
    robot, humans = robot[0], humans[0]
    robot[0], robot[1] = 1.5, -2.25
    robot[5], robot[6] = -1.5, 2.25
    humans[1, :2] = (1.5 + 1.75, -2.25 + 0.5)
    humans[3, :2] = (1.5 - 1.75, -2.25 + 0.5)
    humans[0, :2] = (1.5 + 0.25, -2.25 + 3.0)       # farther than the pair
    humans[2, :2] = (1.5 - 1.0, -2.25 - 0.75)       # nearer
    humans[4, :2] = (1.5 + 2.5, -2.25 - 2.0)        # the farthest
    return robot, humans


def main():
    torch.manual_seed(WEIGHT_SEED)
    sd2 = {k: v.detach().clone() for k, v in make_policy("holonomic", 61, True).model.state_dict().items()}
    sd1 = {k: v.detach().clone() for k, v in make_policy("holonomic", 61, False).model.state_dict().items()}
    out = {"vn2." + k: v.numpy().astype(np.float32) for k, v in sd2.items()}
    out.update({"vn1." + k: sd1[k].numpy().astype(np.float32) for k in CELL})
    out["saturated_scale"] = np.float64(SATURATED_SCALE)
    out["saturated_recurrent_scale"] = np.float64(SATURATED_RECURRENT_SCALE)

    def variant_sd(input_dim, interact, wset):
        if interact:
            sd = {k: v.clone() for k, v in sd2.items()}
            sd["mlp1.0.weight"] = sd["mlp1.0.weight"][:, :input_dim].contiguous()
        else:
            sd = {k: sd1[k].clone() for k in CELL}
            sd.update({k: v.clone() for k, v in sd2.items() if k.startswith("mlp.")})
            sd["lstm.weight_ih_l0"] = sd["lstm.weight_ih_l0"][:, :input_dim].contiguous()
        if wset == "saturated":
            for k in CELL:
                sd[k] = sd[k] * (SATURATED_RECURRENT_SCALE if k == "lstm.weight_hh_l0" else SATURATED_SCALE)
        return sd

    # (tag, kind, kinematics, H, D, interact, weights, seed)
    cases = []
    for H in (2, 5, 20):
        for kin in ("holonomic", "unicycle"):
            cases.append(("h%d_%s" % (H, kin[:4]), "search", kin, H, 61, True, "plain", 400 + H))
    for im in (True, False):
        cases.append(("h1_im%d" % im, "search", "holonomic", 1, 13, im, "plain", 410 + im))
    for D, im in ((13, True), (29, True), (45, True), (13, False), (29, False), (45, False), (61, False)):
        cases.append(("d%d_im%d" % (D, im), "search", "holonomic", 5, D, im, "plain", 420 + D + im))
    cases.append(("tie", "search", "holonomic", 5, 61, True, "plain", None))
    cases.append(("tie_vn1", "search", "holonomic", 5, 13, False, "plain", None))
    for H in (2, 5, 20):
        for D, im in ((61, True), (61, False), (13, True), (13, False)):
            for rep in (0, 1):
                cases.append(("sat%d_h%d_d%d_im%d" % (rep, H, D, im), "search", "unicycle" if (H, D) == (5, 61) else "holonomic", H, D,
                              im, "saturated", 500 + 10 * H + D + im + 1000 * rep))
    for wset in ("plain", "saturated"):
        for im in (True, False):
            for form in ("nolen", "dec", "eq"):
                cases.append(("net_%s_im%d_%s" % (form, im, wset[:3]), "net", "holonomic", 5, 61, im, wset, 600 + im))
            cases.append(("net_dec20_im%d_%s" % (im, wset[:3]), "net", "holonomic", 20, 13, im, wset, 620 + im))

    for wset in ("plain", "saturated"):
        for H in (5, 20):
            for im in (True, False):
                cases.append(("bulk_h%d_im%d_%s" % (H, im, wset[:3]), "bulk", "holonomic", H, 13, im, wset, gpu_seed(H, BULK_B)))

    lines = []
    for ci, (tag, kind, kin, H, D, im, wset, seed) in enumerate(cases):
        pol = make_policy(kin, D, im)
        pol.model.load_state_dict(variant_sd(D, im, wset))
        pre = "case%d." % ci
        if kind == "bulk":
            robots, crowds = cpu.scenes(seed, BULK_B, H, kin)
            orders, values, chosens = [], [], []
            for root in range(BULK_ROOTS):
                js = joint_state(robots[root], crowds[root])
                order, dists = upstream_sort(js)
                assert np.diff(np.sort(dists)).min() > 1e-6, "distances too close for a sort case"
                pol.action_space = None
                with torch.no_grad():
                    action = MultiHumanRL.predict(pol, js)
                orders.append(order)
                values.append(pol.action_values)
                chosens.append([i for i, a in enumerate(pol.action_space) if a == action][0])
            out[pre + "seed"] = np.int64(seed)                      # the scenes are sarl_cpu.scenes(seed, 40, H)[:16]
            out[pre + "order"] = np.asarray(orders, np.int16)
            out[pre + "action_values"] = np.asarray(values, np.float64)
            out[pre + "chosen"] = np.asarray(chosens, np.int16)
            print("%-22s H=%2d D=%d im=%d %d roots |V|max=%.3f" % (tag, H, D, im, BULK_ROOTS, np.abs(out[pre + "action_values"]).max()))
        elif kind == "search":
            if seed is None:
                robot, humans = tie_scene()
            else:
                robot, humans = cpu.scenes(seed, 1, H, kin)
                robot, humans = robot[0], humans[0]
            js = joint_state(robot, humans)
            order, dists = upstream_sort(js)
            gaps = np.diff(np.sort(dists))
            if seed is None:
                assert dists[1] == dists[3] and order.index(1) + 1 == order.index(3), (dists, order)
                gaps = gaps[gaps != 0]
            assert gaps.size == 0 or gaps.min() > 1e-6, "distances too close for a sort case"
            pol.action_space = None
            with torch.no_grad():
                action = MultiHumanRL.predict(pol, js)
            table = np.asarray([[float(a[0]), float(a[1])] for a in pol.action_space])
            assert np.array_equal(table, cpu.action_table(kin, float(robot[7]))), "action tables differ"
            chosen = [i for i, a in enumerate(pol.action_space) if a == action][0]
            out[pre + "robot"] = np.asarray(robot, np.float64)
            out[pre + "humans"] = np.asarray(humans, np.float64)        # in the GIVEN order
            out[pre + "order"] = np.asarray(order, np.int64)
            out[pre + "action_values"] = np.asarray(pol.action_values, np.float64)
            out[pre + "chosen"] = np.int64(chosen)
            out[pre + "transform"] = pol.transform(js).numpy().astype(np.float32)
            print("%-22s H=%2d D=%d im=%d chosen=%2d |V|max=%.3f order %s" % (tag, H, D, im, chosen, np.abs(out[pre + "action_values"]).max(),
                                                                            order if H <= 5 else "..."))
        else:
            form = tag.split("_")[1]
            S = {"nolen": 1, "dec": H, "eq": 3, "dec20": H}[form]
            robot, humans = cpu.scenes(seed, S, H, kin)
            rows = []
            for b in range(S):
                js = joint_state(robot[b], humans[b])
                upstream_sort(js)
                rows.append(pol.transform(js))
            rows = torch.stack(rows)
            lengths = None if form == "nolen" else (list(range(H, 0, -1)) if form.startswith("dec") else [H] * S)
            with torch.no_grad():
                value = pol.model(rows if lengths is None else (rows, torch.IntTensor(lengths)))
            out[pre + "rows"] = rows.numpy().astype(np.float32)
            if lengths is not None:
                out[pre + "lengths"] = np.asarray(lengths, np.int64)
            out[pre + "value"] = value.numpy()[:, 0].astype(np.float32)
            print("%-22s S=%2d H=%2d D=%d im=%d |V|max=%.3f" % (tag, S, H, D, im, np.abs(out[pre + "value"]).max()))
        lines.append("%s|%s|%s|%d|%d|%d|%s" % (tag, kind, kin, H, D, int(im), wset))
    out["cases"] = np.asarray(lines)
    np.savez_compressed(os.path.join(HERE, "lstm.npz"), **out)
    print("wrote lstm.npz, %d bytes" % os.path.getsize(os.path.join(HERE, "lstm.npz")))


if __name__ == "__main__":
    main()
