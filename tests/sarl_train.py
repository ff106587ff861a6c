"""SARL / OM-SARL training on the CPU, restated for the tests: seeded replay rows, the float64 gradient of the value network, its
ReLU margins, the two deliberately wrong gradients the bounds must catch, and the trainer loop.

The gradient reference is float64 torch autograd through tests/sarl_cpu.value_network.  `network` below is that function with
switches (detached softmax weights, detached mean, recorded pre-activations); with every switch off it returns value_network's bits
(tests/test_sarl_train_cpu.py).  Nothing here imports the package's kernels.
"""
import os

import numpy as np
import torch

from tests import sarl_cpu as cpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sarl_train.npz")
PARAMS = ["%s.%s" % (layer, part) for layer in cpu.LAYERS for part in ("weight", "bias")]
VARIANTS = [(61, True), (45, True), (29, True), (13, True), (61, False), (45, False), (29, False), (13, False)]
RELU_MARGIN = 1e-5
MARGIN_FACTOR = 4            # the device sums in MFMA order, upstream in BLAS order; neither order is the reference
_fixture = {}


def fixture():
    if not _fixture:
        _fixture.update(np.load(GOLDEN, allow_pickle=False))
    return _fixture


# ---- gradient cases ------------------------------------------------------------------------------------------------------------
# (S, H, D, with_global_state): S = one scene, one full tile of sixteen, a partial second tile, a third; H = 1 (without maps only),
# 2, 5 and 21, the first crowd past the forward's LDS parking; every variant of the row width and the global state.  The flagship
# variant takes every S at H = 2 and 5; the crowd of 21 comes with the scene counts whose ReLU margin a seed can satisfy
# (make_golden_sarl_train.py: a pre-activation within 1e-5 of zero is a matter of seeds up to a few thousand rows' units, not beyond).
SHAPES = [(S, H, 61, True) for S in (1, 16, 17, 33) for H in (2, 5)] + \
         [(1, 21, 61, True), (2, 21, 61, True), (1, 21, 61, False), (1, 21, 13, True), (1, 1, 13, True), (17, 1, 13, True),
          (33, 1, 13, False)] + \
         [(17, 5, D, gs) for D, gs in VARIANTS[1:]] + [(33, 2, D, gs) for D, gs in VARIANTS[1:]]
FULL_CASE = (17, 5, 61, True, "sharp")          # the one case whose upstream gradients are stored in full


def gradient_cases():
    """[(S, H, D, with_global_state, weights)] in fixture order."""
    return [shape + (w,) for shape in SHAPES for w in ("plain", "sharp")]


def case_tag(case):
    S, H, D, gs, w = case
    return "s%d_h%d_d%d_g%d_%s" % (S, H, D, int(gs), w)


def case_rows(S, H, D, seed):
    """(S, H, D) float32 rows: cpu.transform of S seeded scenes."""
    robot, humans = cpu.scenes(seed, S, H)
    return torch.stack([cpu.transform(robot[s], humans[s], "holonomic", cpu.om_of(D)) for s in range(S)])


def case_targets(S, seed):
    return torch.tensor(np.random.RandomState(seed + 7919).uniform(0.0, 1.0, (S, 1)).astype(np.float32))


def case_seed(case):
    """The seed the generator settled on for `case` (the first of its sequence whose ReLU margin holds)."""
    fx = fixture()
    return int(fx["seeds"][[str(t) for t in fx["cases"]].index(case_tag(case))])


# ---- the network with switches ---------------------------------------------------------------------------------------------------
def _mlp(x, sd, name, indices, last_relu, pre):
    for k, i in enumerate(indices):
        x = x @ sd["%s.%d.weight" % (name, i)].t() + sd["%s.%d.bias" % (name, i)]
        if last_relu or k + 1 < len(indices):
            if pre is not None:
                pre.append(x.detach())
            x = torch.relu(x)
    return x


def network(rows, sd, with_global_state=True, dtype=torch.float64, detach_weights=False, detach_mean=False, pre=None):
    """cpu.value_network's value (S,); `sd` is used as given (leaf tensors of `dtype`).  detach_weights: no gradient through the
    softmax; detach_mean: none through the mean over the humans; pre (a list): receives every ReLU's pre-activations."""
    rows = torch.as_tensor(rows).to(dtype)
    S, H, D = rows.shape
    y = _mlp(rows.reshape(S * H, D), sd, "mlp1", (0, 2), True, pre)
    feat = _mlp(y, sd, "mlp2", (0, 2), False, pre).reshape(S, H, -1)
    if with_global_state:
        mean = y.reshape(S, H, -1).mean(dim=1, keepdim=True).expand(S, H, y.shape[1]).reshape(S * H, -1)
        att_in = torch.cat([y, mean.detach() if detach_mean else mean], dim=1)
    else:
        att_in = y
    scores = _mlp(att_in, sd, "attention", (0, 2, 4), False, pre).reshape(S, H)
    e = torch.exp(scores - scores.max(dim=1, keepdim=True).values)
    w = e / e.sum(dim=1, keepdim=True)
    if detach_weights:
        w = w.detach()
    joint = torch.cat([rows[:, 0, :6], (w.unsqueeze(2) * feat).sum(dim=1)], dim=1)
    return _mlp(joint, sd, "mlp3", (0, 2, 4, 6), False, pre)[:, 0]


def leaves(sd, dtype=torch.float64):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def mse_gradients(value_fn, sd, targets):
    """{name: d mean((value - target)^2) / d parameter}; a parameter the loss does not reach gets zeros."""
    loss = ((value_fn(sd) - targets[:, 0].to(next(iter(sd.values())).dtype)) ** 2).mean()
    grads = torch.autograd.grad(loss, [sd[k] for k in PARAMS], allow_unused=True)
    return {k: (torch.zeros_like(sd[k]) if g is None else g.detach()) for k, g in zip(PARAMS, grads)}


def reference_gradients(rows, targets, sd, with_global_state):
    """The yardstick: float64 autograd through tests/sarl_cpu.value_network."""
    sd64 = leaves(sd)
    return mse_gradients(lambda p: cpu.value_network(rows, p, with_global_state, torch.float64)[0], sd64, targets)


def switched_gradients(rows, targets, sd, with_global_state, **switches):
    sd64 = leaves(sd)
    return mse_gradients(lambda p: network(rows, p, with_global_state, torch.float64, **switches), sd64, targets)


def relu_margin(rows, sd, with_global_state):
    """The smallest |pre-activation| of any ReLU in the float64 pass."""
    pre = []
    with torch.no_grad():
        network(rows, {k: v.double() for k, v in sd.items()}, with_global_state, torch.float64, pre=pre)
    return min(float(p.abs().min()) for p in pre)


def max_abs(grads):
    return np.array([float(grads[k].abs().max()) for k in PARAMS])


def distances(grads, ref):
    return np.array([float((grads[k].double() - ref[k].double()).abs().max()) for k in PARAMS])


# ---- the bound -------------------------------------------------------------------------------------------------------------------
def relative_figures(weights):
    """Per parameter tensor the largest upstream distance / float64 max |g| over the fixture's cases of one weight set (a tensor
    whose gradient is identically zero in a case -- a single human's attention -- is left out of that case).  The entry of
    attention.4.bias is noise over noise and is not used."""
    fx = fixture()
    worst = np.zeros(len(PARAMS))
    for case in gradient_cases():
        if case[4] != weights:
            continue
        dist, ref = fx["grad.%s.dist" % case_tag(case)], fx["grad.%s.max64" % case_tag(case)]
        worst = np.maximum(worst, np.where(ref > 0, dist / np.where(ref > 0, ref, 1.0), 0.0))
    return worst


# relative_figures() as tests/test_sarl_train_cpu.py pins it, in the order of PARAMS -- the house rule of
# sarl_cpu.REFERENCE_DEVIATION: what UPSTREAM's float32 network stands from float64, the largest over the cases of a weight set.
# A single case's own figure is no bound: it is one draw of a rounding error (upstream's mlp3.6.bias gradient lands 2e-9 from
# float64 in s1_h21_d13_g1_plain and 1e-7 in its neighbours), and a gradient inherits the error of the forward value it starts
# from, which the training forward shares bit for bit with the evaluation kernel.
REFERENCE_GRADIENT_DEVIATION = {
    "plain": [3.49e-07, 3.48e-07, 4.58e-07, 3.16e-07, 3.33e-07, 3.27e-07, 5.15e-07, 2.74e-07, 2.78e-06, 2.76e-06, 1.09e-06, 1.12e-06,
              3.34e-06, None, 2.96e-07, 3.02e-07, 3.01e-07, 2.02e-07, 2.79e-07, 1.78e-07, 1.83e-07, 1.17e-07],
    "sharp": [5.81e-07, 5.67e-07, 6.73e-07, 5.24e-07, 3.62e-07, 3.36e-07, 3.98e-07, 3.52e-07, 1.44e-06, 1.41e-06, 1.32e-06, 1.19e-06,
              1.83e-06, None, 2.11e-07, 2.08e-07, 3.49e-07, 2.22e-07, 2.64e-07, 1.92e-07, 2.19e-07, 1.17e-07],
}


def gradient_bounds(case, ref_max):
    """Per parameter tensor, the largest distance from float64 the device may show in `case`: MARGIN_FACTOR times upstream's
    relative figure for the tensor (REFERENCE_GRADIENT_DEVIATION of the case's weight set) times the tensor's float64 max |g| in
    this case (`ref_max`, in the order of PARAMS) -- never the network's largest gradient: with the plain weights the attention
    tensors' gradients are a thousand times smaller than mlp3's.  A tensor whose float64 gradient is identically zero must come out
    zero.  attention.4.bias -- mathematically zero, the softmax being shift-invariant -- is bounded absolutely, by
    attention.4.weight's relative bound times attention.4.weight's float64 max |g| in the same case."""
    rel = REFERENCE_GRADIENT_DEVIATION[case[4]]
    w4, b4 = PARAMS.index("attention.4.weight"), PARAMS.index("attention.4.bias")
    bound = np.array([MARGIN_FACTOR * (rel[w4] if i == b4 else r) * (ref_max[w4] if i == b4 else m)
                      for i, (r, m) in enumerate(zip(rel, ref_max))], dtype=np.float64)
    return bound


# ---- the trainer loop --------------------------------------------------------------------------------------------------------------
TRAINER_N, TRAINER_BATCH, TRAINER_H, TRAINER_D = 48, 16, 5, 61
PARAMETER_BOUND, LOSS_BOUND = 2e-5, 1e-5         # tests/test_gpu_parity.py's path-G trainer fixture bounds
GAMMA_BAR = pow(0.9, 0.25 * 1)                   # upstream's VNRLTrainer defaults: gamma 0.9, time_step 0.25, v_pref 1
TRAINER_CASES = {"A": dict(weights="plain", optimizer="Adam", epochs=2, batches=2),
                 "B": dict(weights="sharp", optimizer="SGD", epochs=0, batches=2)}


_trainer_data = []


def trainer_data():
    """(states (48,5,61), values (48,1), rewards (48,1), next states): seeded transitions of five humans, rows of cpu.transform,
    values and rewards in the simulator's ranges.  Made once per process and shared."""
    if not _trainer_data:
        rng = np.random.RandomState(53)
        _trainer_data.extend([case_rows(TRAINER_N, TRAINER_H, TRAINER_D, 531),
                              torch.tensor(rng.uniform(0.0, 1.0, (TRAINER_N, 1)).astype(np.float32)),
                              torch.tensor(rng.uniform(-0.25, 1.0, (TRAINER_N, 1)).astype(np.float32)),
                              case_rows(TRAINER_N, TRAINER_H, TRAINER_D, 532)])
    return tuple(_trainer_data)


def trainer_loop(case, dtype=torch.float64):
    """crowd_nav/utils/trainer.py:199-250 on the restated network: un-shuffled batches of 16 of the 48 transitions, a frozen target
    (the initial weights), lr 1e-3; optimize_epoch(epochs) then optimize_batch(batches), which consumes batches + 1 batches and
    divides by `batches`.  Returns (final parameters, [reported losses])."""
    spec = TRAINER_CASES[case]
    states, values, rewards, next_states = (t.to(dtype) for t in trainer_data())
    sd = leaves(cpu.weight_set(spec["weights"], TRAINER_D, True), dtype)
    target = {k: v.detach().clone() for k, v in sd.items()}
    params = [sd[k] for k in PARAMS]
    opt = torch.optim.Adam(params, lr=1e-3) if spec["optimizer"] == "Adam" else torch.optim.SGD(params, lr=1e-3, momentum=0.9)
    losses = []

    def step(lo, goal):
        opt.zero_grad()
        out = network(states[lo:lo + TRAINER_BATCH], sd, True, dtype).unsqueeze(1)
        loss = torch.nn.functional.mse_loss(out, goal)
        loss.backward()
        opt.step()
        return float(loss.detach())
    average = 0.0
    for _ in range(spec["epochs"]):
        total = sum(step(lo, values[lo:lo + TRAINER_BATCH]) for lo in range(0, TRAINER_N, TRAINER_BATCH))
        average = total / TRAINER_N
    if spec["epochs"]:
        losses.append(average)
    total, count = 0.0, 0
    for lo in range(0, TRAINER_N, TRAINER_BATCH):
        with torch.no_grad():
            nxt = network(next_states[lo:lo + TRAINER_BATCH], target, True, dtype).unsqueeze(1)
        total += step(lo, rewards[lo:lo + TRAINER_BATCH] + GAMMA_BAR * nxt)
        count += 1
        if count > spec["batches"]:
            break
    losses.append(total / spec["batches"])
    return {k: v.detach() for k, v in sd.items()}, losses


def parameter_distance(sd, case):
    fx = fixture()
    return max(float((sd[k].detach().double().cpu() - torch.tensor(fx["tr.%s.model.%s" % (case, k)]).double()).abs().max())
               for k in PARAMS)
