"""The MLP row kernels of csrc/rgl_rows.hip in every form they launch: the case table, the form each case takes (asked of
the library: rgl_plan_mlp_rows, host only) and the float64 references.  Nothing here needs a GPU.

A "run" is one model (x_dim, wr_dims, wh_dims, value_network_dims or motion_predictor_dims) on S scenes of H humans, through the
value estimator or the state predictor.  The tile pipeline runs each of the model's MLPs as a row job -- w_r and the value head
over S rows, w_h and the motion head over S * H rows -- and plan_rows_job picks a launch form per job.  FORMS names them:

  kind12 / kind21 / kind22   mlp2_rows_kernel<T0, T2>: two layers, hidden width 64, in <= 32, out <= 32
  kind1_le64k / kind1_gt64k  head_rows_kernel (<= 1024 tiles, weights from L2), without / with the raised dynamic-LDS limit
  coop1                      mlp_rows_kernel, a workgroup per tile, all weights in LDS (RGL_HEAD_ROWS_DIRECT=0)
  coop2_few / coop2_many     the same with one layer's weights in LDS at a time; up to / beyond 1024 tiles
  waves1 .. waves4           mlp_rows_kernel beyond 1024 tiles: that many waves per workgroup, each walking its own tiles
  waves0                     nothing fits: the pipeline answers "not mine"

kind11 (in <= 16 AND out <= 16) is not in the list because no job can take it: the embeddings end in x_dim and the heads begin
with it, and the tile kernels exist for x_dim 32 and 64 only.  mlp2_rows_kernel<1, 1> is compiled but unreachable through the ABI.

`jobs` of a run states the form of the jobs the run is there for, as (RGL_HEAD_ROWS_DIRECT unset, =0); tests/test_row_forms_cpu.py
holds every such statement against the library's answer in both settings, and FORMS against the table, so a GPU test that says "this
is the two-waves-per-workgroup form" is right.  The other jobs of a run (shipped embeddings: kind12) are planned too: a run is
"not mine" as soon as one of its jobs has no waves.
"""
import collections
import ctypes
import functools
import json

import numpy as np
import torch

import relationalgraphlearning_amd as rga
from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd.config import policy_config
from oracle import rgl_oracle as orc

FORMS = ("kind12", "kind21", "kind22", "kind1_le64k", "kind1_gt64k", "coop1", "coop2_few", "coop2_many",
         "waves1", "waves2", "waves3", "waves4", "waves0")
TWO_TILES = ("kind12", "kind21", "kind22", "coop2_many", "waves1", "waves2", "waves3", "waves4")      # forms in which a wave walks tiles
SHIPPED_E, SHIPPED_V, SHIPPED_M = [64, 32], [32, 100, 100, 1], [64, 5]
DISTINCT, DISTINCT_CROWDED = 37, 7  # different scenes of a run, up to 5 humans and beyond (see scenes)
SMALL_ROWS = 512                    # runs up to here are "small": every job's row count is no multiple of the 16-row tile

Run = collections.namedtuple("Run", "id module X wr wh head S H seed jobs")


def _run(id, module, head, S, H, jobs, X=32, wr=None, wh=None, seed=0):
    return Run(id, module, X, wr or [64, X], wh or [64, X], head, S, H, seed, jobs)


# seeds: the first of 0, 1, 2, .. at which the float32 and the float64 oracle agree on every ReLU mask with three times the margin
# tests/test_row_forms.py asserts for every run (`reference`: 24 where 8 is asserted; the float32 errors depend on the host's BLAS)
RUNS = [
    # value heads: a row per scene
    _run("V1-37", "value", [1], 37, 3, {"value": ("kind1_le64k", "coop1")}),
    _run("V1-16400", "value", [1], 16400, 1, {"value": ("waves4", "waves4")}),
    _run("V2-37", "value", [7, 1], 37, 3, {"value": ("kind1_le64k", "coop1")}),
    _run("V2-16400", "value", [7, 1], 16400, 2, {"value": ("waves4", "waves4")}, seed=1),
    _run("V3-21", "value", [256, 3, 130, 1], 21, 4, {"value": ("kind1_le64k", "coop1"), "w_r": ("kind1_le64k", "coop1")}, X=64, seed=1),
    _run("V4-17", "value", [256, 256, 256, 256, 256, 1], 17, 2, {"value": ("kind1_gt64k", "waves0")}, X=64),
    _run("V5-50", "value", [150, 100, 100, 1], 50, 5, {"value": ("kind1_le64k", "coop2_few")}),
    _run("V5-16400", "value", [150, 100, 100, 1], 16400, 1, {"value": ("coop2_many", "coop2_many")}),
    _run("V6-16400", "value", [128, 128, 1], 16400, 1, {"value": ("waves2", "waves2")}),
    _run("V7-37", "value", [200, 200, 1], 37, 3, {"value": ("kind1_le64k", "waves0")}),
    _run("V7-16400", "value", [200, 200, 1], 16400, 1, {"value": ("waves0", "waves0")}),
    _run("S-16400", "value", SHIPPED_V, 16400, 2, {"value": ("waves3", "waves3"), "w_r": ("kind12", "kind12"), "w_h": ("kind12", "kind12")}, seed=3),
    # motion heads: a row per human
    _run("M1-95", "motion", [64, 24], 5, 19, {"motion": ("kind22", "kind22")}),
    _run("M1-17100", "motion", [64, 24], 900, 19, {"motion": ("kind22", "kind22")}, seed=3),
    _run("M2-95", "motion", [100, 5], 5, 19, {"motion": ("kind1_le64k", "coop1")}),
    _run("M2-17100", "motion", [100, 5], 900, 19, {"motion": ("waves2", "waves2")}, seed=3),
    _run("M3-95", "motion", [5], 5, 19, {"motion": ("kind1_le64k", "coop1")}),
    _run("M4-95", "motion", [64, 64, 5], 5, 19, {"motion": ("kind1_le64k", "coop1")}),
    _run("M5-95", "motion", [64, 5], 5, 19, {"motion": ("kind1_le64k", "coop1")}, X=64),
    _run("M6-17100", "motion", [256, 5], 900, 19, {"motion": ("waves2", "waves2")}, seed=3),
    _run("S-95", "motion", SHIPPED_M, 5, 19, {"motion": ("kind21", "kind21"), "w_h": ("kind12", "kind12")}),
    # embeddings
    _run("E1-95", "value", SHIPPED_V, 5, 19, {"w_h": ("kind1_le64k", "coop1")}, wh=[48, 32]),
    _run("E1-17100", "value", SHIPPED_V, 900, 19, {"w_h": ("waves4", "waves4")}, wh=[48, 32], seed=1),
    _run("E2-17100", "value", [64, 1], 900, 19, {"w_h": ("waves1", "waves1")}, X=64, wh=[256, 64]),
    # w_r as a shared tile and w_h as four waves per workgroup: under RGL_HEAD_ROWS_DIRECT=0 both are mlp_rows_kernel jobs of ONE
    # launch, which then takes 512 threads while w_h's workgroups mask all but four waves
    _run("E3-17100", "value", SHIPPED_V, 900, 19, {"w_r": ("kind1_le64k", "coop1"), "w_h": ("waves4", "waves4")},
         wr=[128, 64, 32], wh=[48, 32]),
    # more tiles than the 2048 waves a job may have: some waves walk a second tile, whose gradients are added to the slab the first
    # one wrote (at 16 400 rows every wave has one tile) -- one run for each form that walks tiles (TWO_TILES)
    _run("A1-34200", "value", [64, 1], 1800, 19, {"w_h": ("waves1", "waves1")}, X=64, wh=[256, 64]),
    _run("A2-34200", "motion", [100, 5], 1800, 19, {"motion": ("waves2", "waves2"), "w_h": ("kind12", "kind12")}, seed=3),
    _run("A3-34200", "motion", [100, 100, 5], 1800, 19, {"motion": ("waves3", "waves3")}, seed=3),
    _run("A4-34200", "value", SHIPPED_V, 1800, 19, {"w_h": ("waves4", "waves4")}, wh=[48, 32], seed=1),
    _run("AC-34200", "motion", [150, 100, 100, 5], 1800, 19, {"motion": ("coop2_many", "coop2_many")}, seed=4),
    _run("AK-34200", "motion", [64, 24], 1800, 19, {"motion": ("kind22", "kind22")}, seed=3),
    _run("AS-34200", "motion", SHIPPED_M, 1800, 19, {"motion": ("kind21", "kind21")}, seed=3),
    # few scenes of many nodes: the caller's workspace (n_scenes x n_params floats) cannot hold a slab per tile of w_h, so the
    # backward halves max_waves and a wave walks several tiles (SHORT_WORKSPACE below)
    _run("W-248", "value", SHIPPED_V, 4, 62, {"w_h": ("kind1_le64k", "coop1")}, wh=[256, 32]),
]
RUN = {r.id: r for r in RUNS}
SHORT_WORKSPACE = "W-248"


def small(run):
    return run.S * run.H <= SMALL_ROWS


# ---------------------------------------------------------------------------------------------------------------------------
# the library's plan
# ---------------------------------------------------------------------------------------------------------------------------
def job_mlps(run):
    """{job: (dims, last_relu, rows)} of the run's pipeline (module "rgl" -- the graph model alone, tests/graph_forms.py -- has no head)."""
    jobs = collections.OrderedDict()
    jobs["w_r"] = ([9] + list(run.wr), 1, run.S)
    jobs["w_h"] = ([5] + list(run.wh), 1, run.S * run.H)
    if run.module != "rgl":
        jobs[run.module] = ([run.X] + list(run.head), 0, run.S if run.module == "value" else run.S * run.H)
    return jobs


def graph_flags(run):
    """(layers, similarity, layerwise, skip, scenes per crowd) of a run: the shipped graph unless the run's table has these columns
    (tests/graph_forms.py)."""
    return (getattr(run, "L", 2), getattr(run, "sim", "embedded_gaussian"), bool(getattr(run, "lw", False)),
            bool(getattr(run, "skip", True)), getattr(run, "spc", 1))


def plan(dims, rows, max_waves=2048, last_relu=0):
    """rgl_plan_mlp_rows for an MLP of these widths: a dict of the plan's fields and its form."""
    m = nat.RglMlp()
    m.n_layers, m.last_relu = len(dims) - 1, last_relu
    for i, d in enumerate(dims):
        m.dims[i] = d
    p = nat.RglRowsPlan()
    nat.check(nat.lib().rgl_plan_mlp_rows(ctypes.byref(m), rows, max_waves, ctypes.byref(p)), "rgl_plan_mlp_rows")
    out = {k: int(getattr(p, k)) for k, _ in nat.RglRowsPlan._fields_ if k != "reserved"}
    out["form"] = form_of(out)
    return out


def form_of(p):
    if p["waves_per_wg"] == 0:
        return "waves0"
    if p["kind"] >= 10:
        return "kind%d" % p["kind"]
    if p["kind"] == 1:
        return "kind1_le64k" if p["lds_bytes"] <= 64 * 1024 else "kind1_gt64k"
    if p["coop"]:
        return "coop1" if p["coop"] == 1 else ("coop2_few" if p["n_tiles"] <= 1024 else "coop2_many")
    return "waves%d" % p["waves_per_wg"]


def plans(run, max_waves=2048):
    return {job: plan(dims, rows, max_waves, relu) for job, (dims, relu, rows) in job_mlps(run).items()}


def not_mine(run):
    """The pipeline refuses the run in this process's RGL_HEAD_ROWS_DIRECT setting: one of its jobs has no waves."""
    return any(p["form"] == "waves0" for p in plans(run).values())


def dump_plans():
    """Entry point of the CPU test's child processes (the switch is read once per process): every run's plans as one JSON line."""
    print(json.dumps({r.id: plans(r) for r in RUNS}))


def n_params(run):
    """(w_r, w_h, graph, head) parameter counts: the slab widths of the backward."""
    count = lambda dims: sum(a * b + b for a, b in zip(dims[:-1], dims[1:]))
    mlps = job_mlps(run)
    L, sim = graph_flags(run)[:2]
    return (count(mlps["w_r"][0]), count(mlps["w_h"][0]), ((1 if sim == "embedded_gaussian" else 0) + L) * run.X * run.X,
            count(mlps[run.module][0]) if run.module in mlps else 0)


def backward_workspace(run, max_waves, graph_workgroups=None, row_slabs=True):
    """(bytes the tile backward takes at `max_waves`, bytes the caller provides).  The accounting of backward_tiles, not the planner:
    three [S][N][X] feature arrays, a slab per wave of every row job (the waves from rgl_plan_mlp_rows; row_slabs=False leaves them
    out: a lower bound, whatever the launcher's rebalancing of narrow jobs does to their waves) and per workgroup of the graph kernel
    (graph_workgroups; None: a workgroup per scene, as at the row tables' sizes), every piece a multiple of 256 bytes."""
    wr, wh, graph, head = n_params(run)
    p = plans(run, max_waves)
    piece = lambda floats: (floats * 4 + 255) // 256 * 256
    feat = run.S * (run.H + 1) * run.X
    used = 3 * piece(feat) + piece((min(run.S, max_waves) if graph_workgroups is None else graph_workgroups) * graph)
    if row_slabs:
        used += piece(p["w_r"]["n_waves"] * wr) + piece(p["w_h"]["n_waves"] * wh)
        if run.module in p:
            used += piece(p[run.module]["n_waves"] * head)
    return used, run.S * (wr + wh + graph + head) * 4


# ---------------------------------------------------------------------------------------------------------------------------
# models, inputs and the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def build(run):
    """(module, graph model, head) on the CPU: random initialisation under the run's seed, w_a / Ws scaled to the size trained
    weights have (the reference draws them from randn), the head by 0.5."""
    L, sim, lw, skip, _ = graph_flags(run)
    cfg = policy_config("model_predictive_rl", gcn__X_dim=run.X, gcn__final_state_dim=run.X, gcn__wr_dims=list(run.wr),
                        gcn__wh_dims=list(run.wh), gcn__num_layer=L, gcn__similarity_function=sim, gcn__layerwise_graph=lw,
                        gcn__skip_connection=skip,
                        model_predictive_rl__value_network_dims=list(run.head) if run.module == "value" else SHIPPED_V,
                        model_predictive_rl__motion_predictor_dims=list(run.head) if run.module == "motion" else SHIPPED_M)
    torch.manual_seed(1000 + run.seed)
    g = rga.RGL(cfg, 9, 5)
    if run.module == "value":
        mod = rga.ValueEstimator(cfg, g)
        head = mod.value_network
    elif run.module == "motion":
        mod = rga.StatePredictor(cfg, g, 0.25)
        head = mod.human_motion_predictor
    else:                                   # "rgl": the graph model alone, no head
        mod, head = g, None
    with torch.no_grad():
        for n_, p_ in g.named_parameters():
            if n_ == "w_a" or n_.startswith("Ws"):
                p_.mul_(1.0 / run.X ** 0.5)
        for p_ in (head.parameters() if head is not None else ()):
            p_.mul_(0.5)
    return mod, g, head


def scenes(run):
    """S scenes from seeded_scenes: DISTINCT different ones (DISTINCT_CROWDED of more than five humans: 133 human rows at H = 19),
    repeated in that order (periods that share no factor with the 16-row tile; every row still has an upstream gradient of its own).  A ReLU whose pre-activation lies within float32 rounding of zero may
    fall on either side in a float32 kernel, and ONE row on the other side moves a gradient summed over 16 400 rows by 1e-4 of its
    largest entry -- five times the regression-level bound.  Among the millions of pre-activations of 16 400 different scenes some
    always lie that close; among those of DISTINCT scenes a seed is found at which none does (reference: `margin`)."""
    from tests.test_gpu_parity import seeded_scenes
    distinct = DISTINCT if run.H <= 5 else DISTINCT_CROWDED
    first = getattr(run, "first", 0)        # tests/per_scene_backward.py: the run is scenes first .. first + S - 1 of the sequence
    robot, humans = seeded_scenes(7000 + run.seed + run.H, min(first + run.S, distinct), run.H)
    reps = -(-(first + run.S) // distinct)
    crowds = run.S // graph_flags(run)[4]   # sibling scenes share a crowd (forward only): humans [S / spc][H][5]
    return robot.repeat(reps, 1)[first:first + run.S].contiguous(), humans.repeat(reps, 1, 1)[first:first + crowds].contiguous()


def upstream(run):
    """The gradient fed into the module's output, as test_gradients_value_estimator_and_state_predictor feeds it.  A table whose
    Run has `first` and `dark` (tests/per_scene_backward.py) takes scenes first .. first + S - 1 of the sequence's gradient, zero
    for the scenes of the sequence below `dark`."""
    first, dark = getattr(run, "first", 0), getattr(run, "dark", 0)
    S = first + run.S
    if run.module == "value":
        up = torch.linspace(-1.0, 1.5, S).reshape(S, 1)
    elif run.module == "rgl":               # d_H on all rows, as test_gradients_rgl_output_and_path_g feeds it
        up = torch.randn(S, run.H + 1, run.X, generator=torch.Generator().manual_seed(5))
    else:
        up = torch.randn(S, run.H, run.head[-1], generator=torch.Generator().manual_seed(3))
    up[:dark] = 0.0
    return up[first:].contiguous()


class relu_inputs(object):
    """Records the pre-activations of every torch.relu the oracle applies inside the block."""

    def __enter__(self):
        self.seen, self._relu = [], torch.relu

        def relu(x):
            self.seen.append(x.detach().numpy().astype(np.float64))
            return self._relu(x)
        torch.relu = relu
        return self.seen

    def __exit__(self, *exc):
        torch.relu = self._relu
        return False


def oracle(run, dtype, detach=False):
    """Autograd over the oracle in `dtype`: (output, {name: gradient}, every ReLU's pre-activations), numpy float64."""
    mod, g, head = build(run)
    robot, humans = scenes(run)
    leafs = lambda sd: {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    gsd, hsd = leafs(g.state_dict()), leafs(head.state_dict() if head is not None else {})
    L, sim, lw, skip, spc = graph_flags(run)
    cfg = orc.OracleConfig(x_dim=run.X, num_layer=L, similarity=sim, layerwise_graph=lw, skip_connection=skip)
    r, h = robot.unsqueeze(1).to(dtype), humans.repeat_interleave(spc, 0).to(dtype)
    with relu_inputs() as pre:
        if run.module == "value":
            out = orc.value_estimator_forward(r, h, gsd, hsd, cfg)
        elif run.module == "rgl":
            out, _ = orc.rgl_forward(r, h, gsd, cfg)
        else:
            emb, _ = orc.rgl_forward(r, h, gsd, cfg)
            if detach:
                emb = emb.detach()
            out = orc.mlp_forward(emb, orc.mlp_layers(hsd, ""), last_relu=False)[:, 1:, :]
    (out * upstream(run).to(dtype)).sum().backward()
    grads = {}
    for prefix, sd in (("graph.", gsd), (run.module + ".", hsd)):
        for k, v in sd.items():
            if v.grad is not None:
                grads[prefix + k] = v.grad.numpy().astype(np.float64)
    return out.detach().numpy().astype(np.float64), grads, pre


def forward_error(got, want):
    """Scaled like test_gpu_parity.close: of max(1, the largest entry)."""
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / max(1.0, float(np.abs(want).max()))


def grad_error(got, want):
    """Scaled like test_gpu_parity._grad_close: of the gradient's largest entry."""
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / max(1e-3, float(np.abs(want).max()))


TABLES = {"rows": RUN}              # tests/graph_forms.py and tests/per_scene_backward.py add their own


def _margin(a, b, zeros_decided):
    """(a ReLU layer's smallest float64 |pre-activation|) / (the float32 evaluation's largest error in the layer)."""
    small = np.abs(a)
    if zeros_decided:
        small = small[~((a == 0) & (b == 0))]
        if small.size == 0:
            return float("inf")
    return float(small.min()) / max(float(np.abs(a - b).max()), 1e-300)


@functools.lru_cache(maxsize=None)
def reference(run_id, detach=False, table="rows"):
    """The float64 result of a run, computed once, with the yardstick for the regression-level bounds: the worst deviation of the
    SAME oracle evaluated in float32 on the CPU (forward; gradients, worst over the parameters), scaled like the assertions.
    masks_agree: the two evaluations took the same side of every ReLU.  margin: the smallest over the ReLU layers of (the layer's
    smallest float64 |pre-activation|) / (the float32 evaluation's largest error in that layer); at 8 and above -- the factor the
    regression-level bounds keep -- no float32 summation order puts a row on the other side of a ReLU.  A table whose Run says
    `zeros_decided` (tests/per_scene_backward.py) leaves out of the smallest the entries that are EXACTLY 0 in both evaluations:
    the unnormalised adjacency of `concatenation` has all-zero rows, whose T_i and GCN pre-activations are 0 in any precision and
    any summation order, and torch and the kernels both close a ReLU at 0."""
    run = TABLES[table][run_id]
    out, grads, pre = oracle(run, torch.float64, detach)
    out32, grads32, pre32 = oracle(run, torch.float32, detach)
    assert sorted(grads) == sorted(grads32) and len(pre) == len(pre32)
    ref = {"out": out, "grads": grads,
           "yard_fwd": forward_error(out32, out), "yard_grad": max(grad_error(grads32[k], grads[k]) for k in grads),
           "masks_agree": all(np.array_equal(a > 0, b > 0) for a, b in zip(pre, pre32)), "n_masks": len(pre),
           "margin": min(_margin(a, b, getattr(run, "zeros_decided", False)) for a, b in zip(pre, pre32))}
    for a in [out] + list(grads.values()):
        a.setflags(write=False)
    return ref
