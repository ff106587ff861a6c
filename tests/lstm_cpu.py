"""LSTM-RL / OM-LSTM-RL on the CPU, restated for the tests: the two recurrent value networks, the distance sort and the one-step
search behind it.

Written from upstream's arithmetic (crowd_nav/policy/lstm_rl.py:9-108 over multi_human_rl.py:12-171; torch's LSTM cell) in this
project's words.  The scenes, the action table, the rows, the maps, `decide` and `gap` are tests/sarl_cpu.py's.  The network runs in
the dtype it is asked for (float64: the yardstick of the device kernel; float32: the same sums in another order than upstream's).
Nothing here imports the package's kernels.
"""
import os

import numpy as np
import torch

from tests import sarl_cpu as cpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lstm.npz")
DT, GAMMA = cpu.DT, cpu.GAMMA
HID = 50
MLP1 = ["mlp1.0", "mlp1.2", "mlp1.4", "mlp1.6"]
HEAD = ["mlp.0", "mlp.2", "mlp.4", "mlp.6"]
CELL = ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0"]
_fixture = {}
_bulk_scenes = {}
BULK_B, BULK_ROOTS = 40, 16     # the fixture's bulk cases: the first 16 roots of the scenes the GPU test searches at B = 40

scenes, action_table, decide, gap, om_of = cpu.scenes, cpu.action_table, cpu.decide, cpu.gap, cpu.om_of


def fixture():
    if not _fixture:
        _fixture.update(np.load(GOLDEN, allow_pickle=False))
    return _fixture


def state_dict_keys(interact):
    return ([k + p for k in MLP1 for p in (".weight", ".bias")] if interact else []) + CELL + [k + p for k in HEAD for p in (".weight", ".bias")]


# ---- weights ---------------------------------------------------------------------------------------------------------------
def weight_set(name="plain", input_dim=61, interact=True):
    """State dict (float32 tensors) of one variant.  The fixture holds one default-initialised set per network at input_dim 61:
    `vn2.` (mlp1, lstm, mlp) and `vn1.` (its lstm; the head is vn2's).  A narrower input takes the first `input_dim` columns of the
    matrix that reads the rows (mlp1.0.weight, or lstm.weight_ih_l0 without the interaction module).  "saturated": the LSTM tensors
    times the recorded scales -- weight_ih and the two biases by one (512: pre-activations of several hundred), weight_hh by a
    smaller one (8), which keeps the recurrence from turning chaotic."""
    fx = fixture()
    sd = {}
    for k in state_dict_keys(interact):
        src = "vn2." if interact or k.startswith("mlp.") else "vn1."
        sd[k] = torch.tensor(fx[src + k])
    first = "mlp1.0.weight" if interact else "lstm.weight_ih_l0"
    sd[first] = sd[first][:, :input_dim].contiguous()
    if name == "saturated":
        for k in CELL:
            sd[k] = sd[k] * float(fx["saturated_recurrent_scale" if k == "lstm.weight_hh_l0" else "saturated_scale"])
    elif name != "plain":
        raise KeyError(name)
    return sd


# ---- the value networks (lstm_rl.py:9-69) --------------------------------------------------------------------------------------
def _mlp(x, sd, name, n):
    for k in range(n):
        x = x @ sd["%s.%d.weight" % (name, 2 * k)].t() + sd["%s.%d.bias" % (name, 2 * k)]
        if k + 1 < n:
            x = torch.relu(x)
    return x


def value_network(rows, sd, interact, lengths=None, dtype=torch.float64, extremes=None):
    """rows (S,H,D) -> value (S,) in `dtype`.  The LSTM over the rows of a sequence in row order from h = c = 0, torch's cell: gates
    W_ih x + b_ih + W_hh h + b_hh in the order i, f, g, o; c <- s(f) c + s(i) tanh(g); h <- s(o) tanh(c).  Sequence s stops
    updating after lengths[s] steps (pack_padded_sequence's hn).  `extremes` (a dict) receives the largest and the smallest
    magnitude of the gate pre-activations of the steps that count."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    rows = torch.as_tensor(rows).to(dtype)
    S, H, D = rows.shape
    x = _mlp(rows.reshape(S * H, D), sd, "mlp1", 4).reshape(S, H, -1) if interact else rows
    h = torch.zeros(S, HID, dtype=dtype)
    c = torch.zeros(S, HID, dtype=dtype)
    lens = torch.full((S,), H, dtype=torch.long) if lengths is None else torch.as_tensor(lengths, dtype=torch.long)
    for t in range(H):
        z = x[:, t] @ sd["lstm.weight_ih_l0"].t() + sd["lstm.bias_ih_l0"] + h @ sd["lstm.weight_hh_l0"].t() + sd["lstm.bias_hh_l0"]
        zi, zf, zg, zo = z.split(HID, dim=1)
        cn = torch.sigmoid(zf) * c + torch.sigmoid(zi) * torch.tanh(zg)
        hn = torch.sigmoid(zo) * torch.tanh(cn)
        on = (t < lens)[:, None]
        c, h = torch.where(on, cn, c), torch.where(on, hn, h)
        if extremes is not None and bool(on.any()):
            mag = z[on[:, 0]].abs()
            extremes["max"] = max(extremes.get("max", 0.0), float(mag.max()))
            extremes["min"] = min(extremes.get("min", float("inf")), float(mag.min()))
    return _mlp(torch.cat([rows[:, 0, :6], h], dim=1), sd, "mlp", 4)[:, 0]


# ---- the sort (lstm_rl.py:103-107) and the search behind it --------------------------------------------------------------------
def distances(robot, humans):
    humans = np.asarray(humans, np.float64)
    dx, dy = humans[:, 0] - float(robot[0]), humans[:, 1] - float(robot[1])
    return np.sqrt(dx * dx + dy * dy)


def sort_order(robot, humans):
    """Indices of the humans by decreasing distance to the robot, ties in their given order (python's sort is stable, also with
    reverse=True)."""
    d = distances(robot, humans)
    return sorted(range(len(d)), key=lambda h: d[h], reverse=True)


def search(robot, humans, kinematics, sd, interact, om, dtype=torch.float64, extremes=None):
    order = sort_order(robot, humans)
    humans = np.asarray(humans, np.float64)[order]
    rows, reward, maps = cpu.search_rows(robot, humans, kinematics, om)
    value = value_network(rows, sd, interact, None, dtype, extremes).double().numpy()
    vals, idx = decide(reward, value, robot[7])
    return dict(order=np.asarray(order), humans=humans, rows=rows, reward=reward, maps=maps, value=value, action_values=vals, best=idx)


# ---- the fixture's cases -------------------------------------------------------------------------------------------------------
def fixture_cases(kind=None):
    out = []
    for ci, line in enumerate(fixture()["cases"]):
        tag, knd, kin, H, D, im, wset = str(line).split("|")
        if kind is None or knd == kind:
            out.append(dict(idx=ci, tag=tag, kind=knd, kinematics=kin, H=int(H), input_dim=int(D), interact=bool(int(im)), weights=wset))
    return out


def case_arrays(ci):
    pre = "case%d." % ci
    return {k[len(pre):]: v for k, v in fixture().items() if k.startswith(pre)}


def bulk_roots(c):
    """A bulk case as BULK_ROOTS search cases: it names its scenes (the first roots of scenes(seed, BULK_B, H)) instead of holding
    them."""
    a = case_arrays(c["idx"])
    key = (int(a["seed"]), c["H"])
    if key not in _bulk_scenes:
        _bulk_scenes[key] = scenes(key[0], BULK_B, c["H"], c["kinematics"])
    robot, humans = _bulk_scenes[key]
    return [dict(robot=robot[r], humans=humans[r], order=a["order"][r], action_values=a["action_values"][r], chosen=a["chosen"][r])
            for r in range(BULK_ROOTS)]


def case_lengths(a):
    return a["lengths"].tolist() if "lengths" in a else None


# ---- the bounds ------------------------------------------------------------------------------------------------------------------
def measured_deviation(weights):
    """The largest distance of what UPSTREAM computed in float32 (the fixture: the action values of its search cases, the values of
    its network cases) from this module's float64, over the fixture cases of one weight set."""
    worst = 0.0
    for c in fixture_cases():
        if c["weights"] != weights:
            continue
        sd = weight_set(weights, c["input_dim"], c["interact"])
        a = case_arrays(c["idx"])
        if c["kind"] != "net":
            for a in bulk_roots(c) if c["kind"] == "bulk" else [a]:
                r = search(a["robot"], a["humans"], c["kinematics"], sd, c["interact"], om_of(c["input_dim"]))
                worst = max(worst, float(np.abs(r["action_values"] - a["action_values"]).max()))
        else:
            v = value_network(a["rows"], sd, c["interact"], case_lengths(a)).numpy()
            worst = max(worst, float(np.abs(v - a["value"].astype(np.float64)).max()))
    return worst


# measured_deviation() as tests/test_lstm_cpu.py pins it; the device is allowed four times upstream's own distance from float64
REFERENCE_DEVIATION = {"plain": 3.13e-8, "saturated": 2.96e-7}


def value_bound(weights):
    return 4 * REFERENCE_DEVIATION[weights]


# ---- what the GPU test runs --------------------------------------------------------------------------------------------------------
GPU_H = [1, 2, 5, 20]
GPU_B = [1, 3, 40, 3]           # through ONE search object: the second 3 reuses the workspace of the 40


def gpu_variants(H):
    """(input_dim, interact) the GPU test runs at H humans: every row width, both networks; maps need two humans."""
    return [(D, im) for D in (13, 29, 45, 61) for im in (True, False) if D == 13 or H >= 2]


def gpu_kinematics(H, input_dim, interact):
    return "unicycle" if (H, input_dim, interact) == (5, 61, True) else "holonomic"      # the one unicycle case


def gpu_seed(H, B):
    return 1000 * H + B


_batches = {}


def root_batch(seed, B, H, kinematics):
    """The B seeded roots of a GPU search as the restatement prepares them, computed once and shared (read-only): the sort, the
    sorted humans, the 13 relation features (B,A,H,13) float32 and the rewards (B,A) float64 of every action."""
    key = (seed, B, H, kinematics)
    if key not in _batches:
        robot, humans = scenes(seed, B, H, kinematics)
        order = np.stack([sort_order(robot[b], humans[b]) for b in range(B)])
        humans_sorted = np.stack([humans[b][order[b]] for b in range(B)])
        rows, reward = [], []
        for b in range(B):
            r, w, _ = cpu.search_rows(robot[b], humans_sorted[b], kinematics, None)
            rows.append(r)
            reward.append(w)
        _batches[key] = dict(robot=robot, humans=humans, order=order, humans_sorted=humans_sorted, rows13=torch.stack(rows),
                             reward=np.stack(reward), maps={})
    return _batches[key]


def batch_rows(batch, input_dim):
    """(B A, H, input_dim) float32 rows of a root batch: the maps of the sorted next human states behind the relation features."""
    rows13 = batch["rows13"]
    B, A, H = rows13.shape[:3]
    om = om_of(input_dim)
    if om is None:
        return rows13.reshape(B * A, H, 13)
    if input_dim not in batch["maps"]:
        batch["maps"][input_dim] = torch.tensor(np.stack([cpu.occupancy_maps(cpu.propagate_humans(h), *om) for h in batch["humans_sorted"]]))
    maps = batch["maps"][input_dim]
    return torch.cat([rows13, maps[:, None].expand(B, A, H, maps.shape[2])], dim=3).reshape(B * A, H, input_dim)


def batch_search(batch, input_dim, interact, weights, extremes=None):
    """float64 action values (B,A) and decisions (B,) of a root batch."""
    value = value_network(batch_rows(batch, input_dim), weight_set(weights, input_dim, interact), interact, extremes=extremes).numpy()
    B, A = batch["reward"].shape
    decided = [decide(batch["reward"][b], value[b * A:(b + 1) * A], batch["robot"][b, 7]) for b in range(B)]
    return np.stack([d[0] for d in decided]), np.asarray([d[1] for d in decided])
