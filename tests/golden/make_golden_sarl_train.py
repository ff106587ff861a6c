"""Fixture generator for SARL / OM-SARL training (build container only: imports the upstream reference through ref_loader).

Writes tests/golden/sarl_train.npz: per gradient case of tests/sarl_train.gradient_cases() what UPSTREAM's sarl.ValueNetwork gives on
the CPU in float32 for an MSE loss against seeded targets -- max |g| of every parameter tensor and its distance from the float64
restatement -- the float64 max |g|, the seed the case settled on and its ReLU margin; upstream's full gradients for one case; and two
runs of upstream's VNRLTrainer on upstream's network (final parameters and reported losses).  Arrays and short tag strings only.

    python tests/golden/make_golden_sarl_train.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_loader  # noqa: E402

ref_loader.load_reference()

from crowd_nav.policy.sarl import ValueNetwork  # noqa: E402
from crowd_nav.utils.trainer import VNRLTrainer, pad_batch  # noqa: E402
from crowd_nav.utils.memory import ReplayMemory  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from tests import sarl_cpu as cpu  # noqa: E402
from tests import sarl_train as st  # noqa: E402

MAX_SEEDS = 4000


def upstream_network(input_dim, with_global_state, sd):
    net = ValueNetwork(input_dim, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], with_global_state, 1.0, 4)
    net.load_state_dict({k: v.clone() for k, v in sd.items()})
    return net


def upstream_gradients(rows, targets, sd, input_dim, with_global_state):
    net = upstream_network(input_dim, with_global_state, sd)
    loss = torch.nn.MSELoss()(net(rows), targets)
    loss.backward()
    named = dict(net.named_parameters())
    return {k: named[k].grad.detach().clone() for k in st.PARAMS}


def settle_seed(case, index):
    """The first seed of the case's sequence whose float64 pass keeps every ReLU pre-activation RELU_MARGIN away from zero: a
    flipped ReLU is not rounding."""
    S, H, D, gs, w = case
    sd = cpu.weight_set(w, D, gs)
    for k in range(MAX_SEEDS):
        seed = 1000 * (index + 1) + k
        rows = st.case_rows(S, H, D, seed)
        margin = st.relu_margin(rows, sd, gs)
        if margin >= st.RELU_MARGIN:
            return seed, margin
    raise RuntimeError("no seed of %d keeps the ReLUs of %s %g away from zero" % (MAX_SEEDS, st.case_tag(case), st.RELU_MARGIN))


class Writer(object):
    def add_scalar(self, *a, **k):
        pass


def upstream_trainer_run(case, data, spec=None):
    spec = st.TRAINER_CASES[case] if spec is None else spec
    states, values, rewards, next_states = data
    net = upstream_network(st.TRAINER_D, True, cpu.weight_set(spec["weights"], st.TRAINER_D, True))
    memory = ReplayMemory(1000)
    for i in range(states.shape[0]):
        memory.push((states[i], values[i], rewards[i], next_states[i]))
    tr = VNRLTrainer(net, memory, torch.device("cpu"), None, st.TRAINER_BATCH, spec["optimizer"], Writer())
    tr.set_learning_rate(1e-3)
    tr.update_target_model(net)
    tr.data_loader = DataLoader(memory, st.TRAINER_BATCH, shuffle=False, collate_fn=pad_batch)
    losses = []
    with torch.enable_grad():
        if spec["epochs"]:
            losses.append(float(tr.optimize_epoch(spec["epochs"])))
        losses.append(float(tr.optimize_batch(spec["batches"], 0)))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}, losses


def main():
    out, tags, seeds, margins = {}, [], [], []
    for index, case in enumerate(st.gradient_cases()):
        S, H, D, gs, w = case
        seed, margin = settle_seed(case, index // 2)         # the two weight sets of a shape start from the same sequence
        rows, targets, sd = st.case_rows(S, H, D, seed), st.case_targets(S, seed), cpu.weight_set(w, D, gs)
        ref = st.reference_gradients(rows, targets, sd, gs)
        up = upstream_gradients(rows, targets, sd, D, gs)
        tag = st.case_tag(case)
        out["grad.%s.max" % tag] = st.max_abs(up)
        out["grad.%s.dist" % tag] = st.distances(up, ref)
        out["grad.%s.max64" % tag] = st.max_abs(ref)
        if case == st.FULL_CASE:
            for k in st.PARAMS:
                out["full.%s" % k] = up[k].numpy().astype(np.float32)
        tags.append(tag)
        seeds.append(seed)
        margins.append(margin)
        rel = np.where(out["grad.%s.max64" % tag] > 0, out["grad.%s.dist" % tag] / np.maximum(out["grad.%s.max64" % tag], 1e-300), 0)
        print("%-28s seed %6d margin %.2e  upstream rel. distance %.1e .. %.1e" % (tag, seed, margin, rel[rel > 0].min(), rel.max()))
    out["cases"], out["seeds"], out["margins"] = np.asarray(tags), np.asarray(seeds, np.int64), np.asarray(margins, np.float64)

    # the trainer: tests/sarl_train.trainer_data()'s 48 seeded transitions (made from seeds, not stored)
    data = st.trainer_data()
    for case in sorted(st.TRAINER_CASES):
        sd, losses = upstream_trainer_run(case, data)
        sd64, losses64 = st.trainer_loop(case, torch.float64)
        gap = max(float((sd[k].double() - sd64[k]).abs().max()) for k in st.PARAMS)
        print("trainer case %s: losses %s (float64 %s), float64 loop ends %.2e from upstream" % (case, losses, losses64, gap))
        if not gap <= st.PARAMETER_BOUND / 4:
            raise RuntimeError("trainer case %s: float32 and float64 end %.2e apart, more than a quarter of the bound" % (case, gap))
        for k in st.PARAMS:
            out["tr.%s.model.%s" % (case, k)] = sd[k].numpy().astype(np.float32)
        out["tr.%s.losses" % case] = np.asarray(losses, np.float64)
    path = os.path.join(HERE, "sarl_train.npz")
    np.savez_compressed(path, **out)
    print("wrote sarl_train.npz, %d bytes" % os.path.getsize(path))
    st._fixture.clear()
    for w in ("plain", "sharp"):                 # what tests/sarl_train.REFERENCE_GRADIENT_DEVIATION pins
        print('    "%s": [%s],' % (w, ", ".join("%.3g" % x for x in st.relative_figures(w))))


if __name__ == "__main__":
    main()
