"""SARL / OM-SARL training on the CPU, restated for the tests: seeded replay rows, the float64 gradient of the value network, its
ReLU margins, the two deliberately wrong gradients the bounds must catch, and the trainer loop.

The gradient reference is float64 torch autograd through tests/sarl_cpu.value_network.  `network` below is that function with
switches (detached softmax weights, detached mean, recorded pre-activations); with every switch off it returns value_network's bits
(tests/test_sarl_train_cpu.py).  Nothing here imports the package's kernels.

The wide cases (further down) are the batches and crowds one seed cannot serve: they are assembled scene by scene, each scene
keeping the ReLU margin on its own, and bounded by a table of their own.
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


def network(rows, sd, with_global_state=True, dtype=torch.float64, detach_weights=False, detach_mean=False, pre=None,
            detach_weights_from=None, drop_last_scene=False):
    """cpu.value_network's value (S,); `sd` is used as given (leaf tensors of `dtype`).  detach_weights: no gradient through the
    softmax; detach_mean: none through the mean over the humans; pre (a list): receives every ReLU's pre-activations;
    detach_weights_from (a human index): no gradient through the attention weights of that human and those behind it -- a softmax
    backward whose 64 threads never take a second trip; drop_last_scene: the last scene's value sends nothing back -- a product whose
    grid stride never reaches its last tile."""
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
    if detach_weights_from is not None and detach_weights_from < H:
        w = torch.cat([w[:, :detach_weights_from], w[:, detach_weights_from:].detach()], dim=1)
    joint = torch.cat([rows[:, 0, :6], (w.unsqueeze(2) * feat).sum(dim=1)], dim=1)
    value = _mlp(joint, sd, "mlp3", (0, 2, 4, 6), False, pre)[:, 0]
    if drop_last_scene:
        value = torch.cat([value[:-1], value[-1:].detach()])
    return value


def leaves(sd, dtype=torch.float64):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def loss_gradients(loss, sd):
    """{name: d loss / d parameter}; a parameter the loss does not reach gets zeros."""
    grads = torch.autograd.grad(loss, [sd[k] for k in PARAMS], allow_unused=True)
    return {k: (torch.zeros_like(sd[k]) if g is None else g.detach()) for k, g in zip(PARAMS, grads)}


def mse_gradients(value_fn, sd, targets):
    """{name: d mean((value - target)^2) / d parameter}."""
    return loss_gradients(((value_fn(sd) - targets[:, 0].to(next(iter(sd.values())).dtype)) ** 2).mean(), sd)


def weighted_gradients(value_fn, sd, grad_value):
    """{name: d sum(grad_value * value) / d parameter}: the gradient a backward is handed `grad_value` (S, 1) for."""
    return loss_gradients((grad_value[:, 0].to(next(iter(sd.values())).dtype) * value_fn(sd)).sum(), sd)


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
    relative figure for the tensor (REFERENCE_GRADIENT_DEVIATION of the case's weight set, WIDE_GRADIENT_DEVIATION for a wide case) times the tensor's float64 max |g| in
    this case (`ref_max`, in the order of PARAMS) -- never the network's largest gradient: with the plain weights the attention
    tensors' gradients are a thousand times smaller than mlp3's.  A tensor whose float64 gradient is identically zero must come out
    zero.  attention.4.bias -- mathematically zero, the softmax being shift-invariant -- is bounded absolutely, by
    attention.4.weight's relative bound times attention.4.weight's float64 max |g| in the same case."""
    rel = (WIDE_GRADIENT_DEVIATION if is_wide(case) else REFERENCE_GRADIENT_DEVIATION)[case[4]]
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


def trainer_loop(case, dtype=torch.float64, spec=None, data=None):
    """crowd_nav/utils/trainer.py:199-250 on the restated network: un-shuffled batches of 16 of the 48 transitions, a frozen target
    (the initial weights), lr 1e-3; optimize_epoch(epochs) then optimize_batch(batches), which consumes batches + 1 batches and
    divides by `batches`.  Returns (final parameters, [reported losses]).  `spec` and `data` replace the case's own and the 48
    transitions (the last batch is then as short as the data leave it, like a DataLoader's)."""
    spec = TRAINER_CASES[case] if spec is None else spec
    states, values, rewards, next_states = (t.to(dtype) for t in (trainer_data() if data is None else data))
    n = states.shape[0]
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
        total = sum(step(lo, values[lo:lo + TRAINER_BATCH]) for lo in range(0, n, TRAINER_BATCH))
        average = total / n
    if spec["epochs"]:
        losses.append(average)
    total, count = 0.0, 0
    for lo in range(0, n, TRAINER_BATCH):
        with torch.no_grad():
            nxt = network(next_states[lo:lo + TRAINER_BATCH], target, True, dtype).unsqueeze(1)
        total += step(lo, rewards[lo:lo + TRAINER_BATCH] + GAMMA_BAR * nxt)
        count += 1
        if count > spec["batches"]:
            break
    losses.append(total / spec["batches"])
    return {k: v.detach() for k, v in sd.items()}, losses


def parameter_distance(sd, case, fx=None):
    fx = fixture() if fx is None else fx
    return max(float((sd[k].detach().double().cpu() - torch.tensor(fx["tr.%s.model.%s" % (case, k)]).double()).abs().max())
               for k in PARAMS)


# ---- wide cases: batches assembled scene by scene ----------------------------------------------------------------------------------
# One seed for a whole batch keeps every ReLU pre-activation RELU_MARGIN from zero only up to about 200 rows.  Scenes do not
# interact in this network -- the mean and the softmax stay inside a scene -- so a batch keeps the margin exactly when each of its
# scenes does: candidate scene k of a shape is case_rows(1, H, D, base + k), it is kept when relu_margin on it alone holds for both
# weight sets, and the first S kept candidates, concatenated, are the batch.  make_golden_sarl_train_wide.py stores the kept
# indices; the tests rebuild only those scenes.  The selection uses the float64 restatement alone.
WIDE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sarl_train_wide.npz")
# (S, H, D, with_global_state): both sides of the softmax backward's 64-thread stride, the narrowest rows at it, the human limit
# (381 rows = 23 tiles of sixteen and 13: a ragged row tile and contraction tail), the first crowd past the forward's LDS parking
# with a partial scene tile, the trainer's published batches, and 13120 rows -- 820 x 10 = 8200 tiles of a 150-column product,
# 2050 blocks of four waves where a launch has 2048: the smallest batch at H = 5 whose last row tile only the grid stride reaches;
# and 256 and 258 rows, the two sides of the span in which sarl_gemm_kernel sums a contraction (the second span then has two rows)
WIDE_SHAPES = [(2, 64, 61, True), (2, 65, 61, True), (2, 64, 13, False), (3, 127, 61, True), (17, 22, 61, True), (100, 5, 61, True),
               (100, 19, 61, True), (2624, 5, 61, True), (128, 2, 61, True), (129, 2, 61, True)]
TAIL_SHAPES = [(3, 127, 61, True), (2624, 5, 61, True)]      # also run with a gradient that only the last two scenes carry
MODULE_ROWS = 1900                                           # up to 100 x 19 a case also runs through loss.backward()
MAX_REJECTED = 0.95                                          # a shape may reject at most this share of its candidates
_wide_fixture, _wide_rows = {}, {}


def wide_fixture():
    if not _wide_fixture:
        _wide_fixture.update(np.load(WIDE_GOLDEN, allow_pickle=False))
    return _wide_fixture


def wide_cases():
    return [shape + (w,) for shape in WIDE_SHAPES for w in ("plain", "sharp")]


def wide_entries():
    """[(case, kind)] in fixture order: every wide case under the MSE loss, then the tail-weighted ones."""
    return [(c, "mse") for c in wide_cases()] + [(shape + (w,), "tail") for shape in TAIL_SHAPES for w in ("plain", "sharp")]


def entry_tag(case, kind="mse"):
    return case_tag(case) + ("" if kind == "mse" else "_" + kind)


def shape_tag(shape):
    return "s%d_h%d_d%d_g%d" % (shape[0], shape[1], shape[2], int(shape[3]))


def is_wide(case):
    return tuple(case[:4]) in WIDE_SHAPES


def wide_base(shape):
    """The seed of a shape's candidate 0; far from every seed the single-seed cases can settle on."""
    return 100000 * (WIDE_SHAPES.index(tuple(shape[:4])) + 1)


def assemble(shape):
    """The generator's side: (kept candidate indices, rows (S, H, D)).  Fails where more than MAX_REJECTED of the candidates would
    have to be rejected; neither that share nor RELU_MARGIN is lowered."""
    S, H, D, gs = shape[:4]
    sds = [cpu.weight_set(w, D, gs) for w in ("plain", "sharp")]
    kept, rows, k = [], [], 0
    while len(kept) < S:
        if 1.0 - S / (k + 1.0) > MAX_REJECTED:               # even if every candidate from here on were kept
            raise RuntimeError("%s: %d of %d candidates kept, more than %g rejected" % (shape_tag(shape), len(kept), k, MAX_REJECTED))
        scene = case_rows(1, H, D, wide_base(shape) + k)
        if all(relu_margin(scene, sd, gs) >= RELU_MARGIN for sd in sds):
            kept.append(k)
            rows.append(scene)
        k += 1
    return np.asarray(kept, np.int32), torch.cat(rows)


def wide_rows(shape):
    """(S, H, D) float32 rows of a wide shape from the fixture's kept indices: made once per process, shared by both weight sets and
    every test, never changed."""
    shape = tuple(shape[:4])
    if shape not in _wide_rows:
        S, H, D, gs = shape
        kept = wide_fixture()["kept.%s" % shape_tag(shape)]
        assert len(kept) == S
        _wide_rows[shape] = torch.cat([case_rows(1, H, D, wide_base(shape) + int(k)) for k in kept])
    return _wide_rows[shape]


def wide_targets(shape):
    return case_targets(shape[0], wide_base(shape))


def tail_grad_value(S):
    """(S, 1) float32, zero but for the last two scenes: the gradient of a loss that only they enter.  A mistake confined to the
    last rows of the last tile is not diluted by 1 / S here."""
    gv = torch.zeros(S, 1)
    gv[S - 2, 0], gv[S - 1, 0] = 1.0, -0.5
    return gv


def wide_gradients(case, kind="mse", **switches):
    """float64 gradients of a wide case: of the MSE against wide_targets, or (kind "tail") of sum(tail_grad_value * value).  Without
    switches this is the yardstick, through tests/sarl_cpu.value_network."""
    S, H, D, gs, w = case
    rows, sd64 = wide_rows(case), leaves(cpu.weight_set(w, D, gs))
    if switches:
        def value_fn(p):
            return network(rows, p, gs, torch.float64, **switches)
    else:
        def value_fn(p):
            return cpu.value_network(rows, p, gs, torch.float64)[0]
    if kind == "tail":
        return weighted_gradients(value_fn, sd64, tail_grad_value(S))
    return mse_gradients(value_fn, sd64, wide_targets(case))


def wide_relative_figures(weights):
    """Per parameter tensor the larger of the pinned figure of the single-seed cases (REFERENCE_GRADIENT_DEVIATION, unchanged) and
    the largest upstream distance / float64 max |g| over the wide fixture's entries of one weight set: longer float32 sums stand
    further from float64.  Never one entry's own figure, never anything a device produced."""
    fx = wide_fixture()
    worst = np.array([0.0 if p is None else p for p in REFERENCE_GRADIENT_DEVIATION[weights]])
    for case, kind in wide_entries():
        if case[4] != weights:
            continue
        dist, ref = fx["grad.%s.dist" % entry_tag(case, kind)], fx["grad.%s.max64" % entry_tag(case, kind)]
        worst = np.maximum(worst, np.where(ref > 0, dist / np.where(ref > 0, ref, 1.0), 0.0))
    return worst


# wide_relative_figures() as tests/test_sarl_train_wide_cpu.py pins it, in the order of PARAMS: the table that bounds every wide case
WIDE_GRADIENT_DEVIATION = {
    "plain": [6.1e-07, 5.44e-07, 8.61e-07, 5.63e-07, 5.58e-07, 3.35e-07, 8.05e-07, 4.45e-07, 2.78e-06, 2.76e-06, 2.15e-06, 2.22e-06,
              3.34e-06, None, 4e-07, 3.17e-07, 6.72e-07, 2.13e-07, 5.64e-07, 1.78e-07, 6.2e-07, 1.17e-07],
    "sharp": [7.8e-07, 6.32e-07, 1.24e-06, 1.11e-06, 8.52e-07, 5.65e-07, 1.08e-06, 5.72e-07, 4.42e-06, 5.76e-06, 5.27e-06, 5.87e-06,
              7.25e-06, None, 4.54e-07, 3.38e-07, 1.28e-06, 2.22e-07, 6.94e-07, 1.92e-07, 5.93e-07, 1.17e-07],
}


# trainer case C: 50 transitions in batches of 16 leave a last batch of 2, a second shape for either kind of captured step;
# optimize_epoch(1) then optimize_batch(3, 0), which consumes four batches, the short one included.  The plain weights, like case
# A: under Adam an element whose gradient is rounding noise moves by the learning rate, and with the sharp weights upstream's
# float32 run and the float64 loop then end 5e-4 apart (attention.0.weight), which says nothing about either.
WIDE_TRAINER_N = 50
WIDE_TRAINER_CASE = dict(weights="plain", optimizer="Adam", epochs=1, batches=3)
_wide_trainer_data = []


def wide_trainer_data():
    """trainer_data()'s kind, 50 transitions from seeds of their own.  Made once per process and shared."""
    if not _wide_trainer_data:
        rng = np.random.RandomState(59)
        _wide_trainer_data.extend([case_rows(WIDE_TRAINER_N, TRAINER_H, TRAINER_D, 591),
                                   torch.tensor(rng.uniform(0.0, 1.0, (WIDE_TRAINER_N, 1)).astype(np.float32)),
                                   torch.tensor(rng.uniform(-0.25, 1.0, (WIDE_TRAINER_N, 1)).astype(np.float32)),
                                   case_rows(WIDE_TRAINER_N, TRAINER_H, TRAINER_D, 592)])
    return tuple(_wide_trainer_data)
