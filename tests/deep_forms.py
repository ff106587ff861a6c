"""children_deep_kernel<NT, F16, SKIP, SOFT, T4> of csrc/rgl_deep.hip -- stage 1 of "value of the sibling children" for three-layer
graphs and for two-layer graphs beyond 32 nodes -- in every form it launches: the table of runs, the form each takes (asked of the
library: rgl_plan_deep_children, host only) and the float64 / float32 references.  Nothing here needs a GPU.

  instantiations  NT 1..4 (node tiles) x {f32 softmax, f32 plain-weight, f16 softmax} x skip on / off, and the T4 forms (f32 softmax,
                  NT >= 2, three layers, at most four valid nodes in the last node tile) x skip: 30
  run time        L 2 | 3;  CT = ceil(A / 16) child tiles (the crowd waves join them when CT > 8 - NT);  stage 2 inside the launch
                  (a packed image at hand) or in robot_head_kernel;  workgroups striding the parents (b, b + grid, ..) or owning
                  parents_per_wg contiguous ones

Every run goes through TreeSearch.value_children: with the shipped value head the Python layer always has the packed image for the
f32 and f16 modes (mprl_children_image_bytes), so the stand-alone call IS the one that runs stage 2 inside the launch; under
RGL_DEEP_FUSE_HEAD=0, and in the bf16x6 mode (whose image is in another layout), stage 2 is robot_head_kernel's.

Node counts: N = H + 1 with 1, 4, 5 and 16 valid nodes in the last node tile of every NT; the largest N the planner covers at
A = 81 (60 with three layers, 64 with two) and at A = 96 (48), and the first N beyond each, which the tile kernel answers (N = 65:
the one-wave-per-child kernel).  Action tables: speeds x rotations + 1 = 2, 16, 17, 49, 81, 96 children; the 81 are 40 speeds x 2
rotations, so that the last child and its neighbour head opposite ways and a kernel that clamps a child index one short shows.
The trained weights were trained with skip connections: without them the values of a crowd's children differ by 1e-4 at most, which
is why the f16 runs without skip use `gaussian` (the f16 bound is 1e-5; `embedded_gaussian` without skip runs in the table and
walking runs, where no such condition on the inputs is asserted).

Walking runs: P = 300 (one: 257) parents on at most 256 workgroup slots.  A launch only walks when a workgroup's LDS exceeds half a
CU's (one workgroup per CU: 256 slots, not 512), so each of these runs has the smallest action table of the list at which the
planner says so for its NT -- 40x2 at NT = 1, 3x16 at NT = 2, 4x4 at NT = 3 (NT = 4 walks with any table: 3x5 there);
tests/test_deep_forms_cpu.py holds it.
"""
import collections
import ctypes
import functools

import numpy as np
import torch

from oracle import rgl_oracle as orc
from relationalgraphlearning_amd import _native as nat
from tests import golden_io as gio
from tests.helpers import dense_scenes

TOL, REG_F32, REG_F16, F16_TOL = 1e-4, 1e-6, 1e-5, 1e-3      # tests/test_gpu_parity.py's (held equal by test_deep_forms_cpu)

Run = collections.namedtuple("Run", "id H L sim skip flavour contraction speeds rots P seed dense kind expect")
SIMS = {"eg": "embedded_gaussian", "ga": "gaussian", "sq": "squared", "eq": "equal_attention", "di": "diagonal"}
NORM = {"eg": 0, "ga": 0, "sq": 1, "eq": 2, "di": 3}
# the thirty instantiations as (NT, family, skip, t4); family: "soft" f32 softmax, "plain" f32 plain-weight, "f16"
INSTANTIATIONS = [(nt, fam, skip, False) for nt in (1, 2, 3, 4) for fam in ("soft", "plain", "f16") for skip in (True, False)] + \
                 [(nt, "soft", skip, True) for nt in (2, 3, 4) for skip in (True, False)]
# N with 1, 4, 5, 16 valid nodes in the last node tile; the last of NT = 4 at three layers is the largest N the planner covers
EDGE_N3 = {1: (2, 4, 5, 16), 2: (17, 20, 21, 32), 3: (33, 36, 37, 48), 4: (49, 52, 53, 60)}
EDGE_N2 = {3: (33, 36, 37, 48), 4: (49, 52, 53, 64)}
LIMITS = [(81, 3, 60), (81, 2, 64), (96, 3, 48), (96, 2, 48)]      # (A, L, largest covered N): asserted from the planner
TABLES = {2: (1, 1), 16: (3, 5), 17: (4, 4), 49: (3, 16), 81: (40, 2), 96: (19, 5)}


# seeds: the first of 0, 1, 2, .. at which (edge runs) dropping the last human, the first human of the last node tile or the last
# child's own robot state moves the float64 reference by 15 x the run's regression bound (test_deep_forms_cpu asserts 10 x), and
# (f16 runs) rounding layer 1's operands to f16 -- reference_f16, on the CPU -- costs no more than REG_F16 less an f32 form's bound.
# The second condition is about the number format, not the kernel: with skip connections and one to three humans that rounding alone
# costs 0.8e-5 to 1.8e-5 (median 1.2e-5 over 40 seeds at N = 2 and N = 4; 1e-6 to 6e-6 at N >= 16 and without skip), so REG_F16 can only
# be asked of inputs on which the format itself stays below it; on every such input the kernel is also held to reference_f16.
SEEDS = {"N2-L3-eg-skip-f16-40x2": 6, "N21-L3-ga-noskip-f16-40x2": 4, "N32-L3-ga-skip-f16-40x2": 5, "N36-L3-ga-noskip-f16-40x2": 1,
         "N37-L3-ga-noskip-f16-40x2": 12, "N48-L3-ga-skip-f16-40x2": 2, "N52-L3-ga-noskip-f16-40x2": 7, "N53-L3-ga-noskip-f16-40x2": 30,
         "N60-L3-ga-skip-f16-40x2": 1}


def _r(N, L, sim, skip, dt="f32", A=81, P=3, seed=None, flavour="trained", dense=False, kind="edge", expect="deep", tag=""):
    speeds, rots = TABLES[A]
    id = "N%d-L%d-%s-%s-%s-%dx%d%s%s" % (N, L, sim, "skip" if skip else "noskip", dt, speeds, rots, tag, "" if P == 3 else "-P%d" % P)
    return Run(id, N - 1, L, SIMS[sim], skip, flavour, dt, speeds, rots, P, SEEDS.get(id, 0) if seed is None else seed, dense, kind, expect)


def _table():
    runs = []
    plain3 = [("sq", True), ("eq", False), ("di", True), ("sq", False)]
    half3 = [("eg", True), ("ga", False), ("ga", False), ("ga", True)]
    for nt, ns in EDGE_N3.items():
        for i, N in enumerate(ns):
            runs.append(_r(N, 3, "eg", True))                    # T4 (skip) at the first two N of NT >= 2, the 16-row form at the others
            runs.append(_r(N, 3, "ga", False))                   # the same without skip; Wa = I built in LDS
            runs.append(_r(N, 3, plain3[i][0], plain3[i][1]))
            runs.append(_r(N, 3, half3[i][0], half3[i][1], "f16"))
    two = [[("eg", True), ("sq", False)], [("ga", False), ("eq", True)], [("eg", False), ("di", False)], [("ga", True), ("sq", True)]]
    for nt, ns in EDGE_N2.items():
        for i, N in enumerate(ns):
            for sim, skip in two[i]:
                runs.append(_r(N, 2, sim, skip))
    # action tables: A = 2, 16, 17 (one child tile; a full last tile; a tile with a single valid child) and 96 (CT = 6)
    for A in (2, 16, 17):
        runs.append(_r(21, 3, "eg", True, A=A, kind="table"))
        runs.append(_r(50, 3, "ga", False, A=A, kind="table"))                  # T4
        runs.append(_r(53, 3, "eg", A != 16, "f16", A=A, kind="table"))
    runs += [_r(5, 3, "sq", True, A=16, kind="table"), _r(37, 3, "eq", False, A=17, kind="table"), _r(21, 3, "di", False, A=2, kind="table"),
             _r(40, 2, "eg", True, A=17, kind="table"), _r(64, 2, "sq", False, A=2, kind="table"),
             _r(48, 3, "eg", True, A=96, kind="table"), _r(48, 3, "ga", False, "f16", A=96, kind="table"),
             _r(36, 3, "eg", False, A=96, kind="table"), _r(16, 3, "sq", True, A=96, kind="table"), _r(48, 2, "eg", True, A=96, kind="table")]
    # workgroups that walk several parents, each with a crowd of its own
    runs += [_r(5, 3, "eg", True, A=81, P=300, seed=3, kind="walk"), _r(21, 3, "eg", False, "f16", A=49, P=300, seed=4, kind="walk"),
             _r(37, 3, "sq", False, A=17, P=257, seed=5, kind="walk"), _r(52, 3, "ga", True, A=16, P=300, seed=6, kind="walk")]
    # raw random-init weights (hidden features of 10..100): the north-star bound only; dense crowds; the bf16x6 mode (f32 form here)
    runs += [_r(N, 3, "eg", True, flavour="rand", kind="rand", tag="-rand") for N in (5, 21, 37, 53)]
    runs += [_r(N, 3, "eg", True, dense=True, seed=11, kind="dense", tag="-dense") for N in (9, 25, 41, 57)]
    runs += [_r(21, 3, "eg", True, "bf16x6", kind="b6"), _r(50, 3, "ga", False, "bf16x6", kind="b6"), _r(40, 2, "eg", True, "bf16x6", kind="b6")]
    # beyond each LDS limit: the planner refuses, another MFMA kernel answers (expect "other"); f16 has no other kernel (expect "error")
    runs += [_r(61, 3, "eg", True, kind="beyond", expect="other"), _r(65, 2, "eg", True, kind="beyond", expect="other"),
             _r(49, 3, "ga", False, A=96, kind="beyond", expect="other"), _r(49, 2, "eg", True, A=96, kind="beyond", expect="other"),
             _r(61, 3, "eg", True, "f16", kind="beyond", expect="error"), _r(40, 2, "eg", True, "f16", kind="beyond", expect="error")]
    return runs


RUNS = _table()
RUN = {r.id: r for r in RUNS}
VALID = "N21-L3-eg-skip-f32-40x2"           # the call that must still be right after a refusal
COVERED = [r for r in RUNS if r.expect == "deep"]
EDGE = [r for r in RUNS if r.kind == "edge"]
WALK = [r for r in RUNS if r.kind == "walk"]
BEYOND = [r for r in RUNS if r.kind == "beyond"]


def num_actions(run):
    return run.speeds * run.rots + 1


def family(run):
    return "f16" if run.contraction == "f16" else ("soft" if NORM[short(run)] == 0 else "plain")


def short(run):
    return [k for k, v in SIMS.items() if v == run.sim][0]


def walk_sample(P):
    """Parents of a walking launch compared with launches of their own: the first and last of workgroups under both ownerships
    (contiguous pairs; b and b + 256), the turn of the stride, the last parent of the launch."""
    picks = list(range(0, 8)) + list(range(40, 48)) + list(range(84, 92)) + list(range(126, 130)) + list(range(250, 260)) + list(range(P - 4, P))
    return sorted({p for p in picks if 0 <= p < P})


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------------------------------------------------------
def seeded_scenes(seed, B, H):
    """tests/test_gpu_parity.py's seeded scenes (the same draws; that module needs no GPU to import, but is the GPU suite's)."""
    rng = np.random.RandomState(seed)
    robot = np.zeros((B, 9), np.float32)
    humans = np.zeros((B, H, 5), np.float32)
    ang = rng.uniform(0, 2 * np.pi, B)
    robot[:, 0], robot[:, 1] = 4 * np.cos(ang), 4 * np.sin(ang)
    robot[:, 2:4] = rng.uniform(-0.7, 0.7, (B, 2))
    robot[:, 4] = 0.3
    robot[:, 5], robot[:, 6] = -4 * np.cos(ang), -4 * np.sin(ang)
    robot[:, 7] = 1.0
    robot[:, 8] = np.pi / 2
    humans[:, :, 0:2] = rng.uniform(-5, 5, (B, H, 2))
    humans[:, :, 2:4] = rng.uniform(-1, 1, (B, H, 2))
    humans[:, :, 4] = 0.3
    return torch.tensor(robot), torch.tensor(humans)


@functools.lru_cache(maxsize=None)
def inputs(run_id):
    """(child_robot (P, A, 9), humans (P, H, 5)) float32: a crowd of its own per parent, the children of the run's action table."""
    run = RUN[run_id]
    seed = 4100 + 7 * run.H + run.seed
    robot, humans = dense_scenes(np.random.RandomState(seed), run.P, run.H) if run.dense else seeded_scenes(seed, run.P, run.H)
    acts, _ = orc.mprl_action_space(orc.OracleConfig(speed_samples=run.speeds, rotation_samples=run.rots), 1.0)
    return orc._children_robot(robot, acts, orc.OracleConfig()), humans


def params(run, dtype):
    ck = gio.checkpoint(run.flavour, run.L, "separate", run.sim)
    return orc.MprlParams.from_checkpoint({k: {kk: vv.to(dtype) for kk, vv in v.items()} for k, v in ck.items()})


def evaluate(run, cr, humans, dtype):
    """orc.value_estimator_forward over every child scene of (cr (P, A, 9), humans (P, H, 5)) in `dtype` -> (P, A) float64 array."""
    P, A, H = cr.shape[0], cr.shape[1], humans.shape[1]
    Pm = params(run, dtype)
    cfg = orc.OracleConfig(num_layer=run.L, similarity=run.sim, skip_connection=run.skip)
    with torch.no_grad():
        out = orc.value_estimator_forward(cr.to(dtype).reshape(P * A, 1, 9), humans.to(dtype)[:, None].expand(P, A, H, 5).reshape(P * A, H, 5),
                                          Pm.ve_graph, Pm.value_network, cfg)
    return out.double().numpy().reshape(P, A)


@functools.lru_cache(maxsize=None)
def reference64(run_id):
    """The children's values with parameters and inputs in float64."""
    out = evaluate(RUN[run_id], *inputs(run_id), torch.float64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference32(run_id):
    """The same evaluation in float32 on the CPU: its deviation from reference64 is what the regression bound is measured against."""
    out = evaluate(RUN[run_id], *inputs(run_id), torch.float32)
    out.setflags(write=False)
    return out


def error(got, want):
    """Deviation relative to max(1, max|want|), as test_gpu_parity.close measures it."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def yardstick(run):
    return error(reference32(run.id), reference64(run.id))


def bounds(run):
    """(north-star bound, regression-level bound or None) of the run's output against reference64, both relative (see `error`).
    f32 forms (and the bf16x6 mode, which runs the f32 form here): TOL and max(REG_F32, 8 x the float32 oracle's deviation); f16:
    F16_TOL and REG_F16; raw random-init weights: the north-star bound only."""
    if run.contraction == "f16":
        return F16_TOL, (None if run.flavour == "rand" else REG_F16)
    return TOL, (None if run.flavour == "rand" else max(REG_F32, 8 * yardstick(run)))


def teeth(run):
    """How far (relative, as `error`) the reference moves when the kernel's edge cases go wrong: {"last human": dropped, "tile
    human": the first human of the last node tile dropped, "last child": the last child given its neighbour's robot state}."""
    cr, humans = inputs(run.id)
    want = reference64(run.id)
    H = run.H
    first = max(16 * ((H + 1 + 15) // 16 - 1) - 1, 0)          # node 16 (NT - 1) is human 16 (NT - 1) - 1; NT = 1: the first human
    keep = [h for h in range(H) if h != first]
    cr2 = cr.clone()
    cr2[:, -1] = cr[:, -2]
    return {"last human": error(evaluate(run, cr, humans[:, :H - 1], torch.float64), want),
            "tile human": error(evaluate(run, cr, humans[:, keep], torch.float64), want),
            "last child": error(evaluate(run, cr2, humans, torch.float64), want)}


# ---------------------------------------------------------------------------------------------------------------------------
# the library's plan
# ---------------------------------------------------------------------------------------------------------------------------
def _mlp(dims, last_relu):
    m = nat.RglMlp()
    m.n_layers, m.last_relu = len(dims) - 1, int(last_relu)
    for i, d in enumerate(dims):
        m.dims[i] = d
    return m


def planner(L, sim, skip, A, contraction):
    """The shipped value estimator's descriptor with dimensions and modes only: the planner export reads no pointer."""
    pl = nat.MprlPlanner()
    g = nat.RglGraph()
    g.w_r, g.w_h = _mlp((9, 64, 32), True), _mlp((5, 64, 32), True)
    g.x_dim, g.num_layer, g.similarity, g.skip_connection = 32, L, nat.SIMILARITY[sim], int(skip)
    pl.value_graph, pl.value_head = g, _mlp((32, 32, 100, 100, 1), False)
    pl.num_actions, pl.contraction_dtype = A, nat.CONTRACTION_DTYPES[contraction]
    return pl


def plan_of(pl, P, H, with_image):
    p = nat.RglDeepChildrenPlan()
    nat.check(nat.lib().rgl_plan_deep_children(ctypes.byref(pl), P, H, int(with_image), ctypes.byref(p)), "rgl_plan_deep_children")
    out = {k: int(getattr(p, k)) for k, _ in nat.RglDeepChildrenPlan._fields_}
    fam = "f16" if out["f16"] else ("soft" if out["norm"] == 0 else "plain")
    out["inst"] = (out["node_tiles"], fam, bool(out["skip"]), bool(out["t4"])) if out["covered"] else None
    return out


def has_image(run):
    """The Python layer packs the value estimator's image for the f32 and f16 modes; the bf16x6 image is the fused kernel's only."""
    return run.contraction != "bf16x6"


def plan(run, with_image=None, P=None):
    """rgl_plan_deep_children for the run (a stand-alone call): a dict of the plan's fields and `inst` (NT, family, skip, t4)."""
    return plan_of(planner(run.L, run.sim, run.skip, num_actions(run), run.contraction), run.P if P is None else P, run.H,
                   has_image(run) if with_image is None else with_image)


def form(run, p=None):
    """"<instantiation>, grid <g>, <k> parent(s) per workgroup, stage 2 inside | outside" of the run's launch."""
    p = plan(run) if p is None else p
    if not p["covered"]:
        return "not the deep kernel"
    nt, fam, skip, t4 = p["inst"]
    return "NT=%d %s%s%s L=%d CT=%d, grid %d, %d parent%s per workgroup, stage 2 %s" % (
        nt, fam, " skip" if skip else "", " T4" if t4 else "", p["layers"], p["child_tiles"], p["grid"], p["parents_per_wg"],
        "" if p["parents_per_wg"] == 1 else "s", "inside" if p["fuse_head"] else "outside")


# ---------------------------------------------------------------------------------------------------------------------------
# what the f16 forms round
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_f16(run_id):
    """The float64 evaluation of a three-layer softmax run in which ONLY the operands of layer 1's two dense products are rounded
    to f16, as the F16 instantiations feed them to v_mfma_f32_16x16x32_f16: H1 and W2 (O = H1 W2), and for E O the crowd block
    E_ij = e^(S_ij - max_j S_ij) (i, j >= 1; the robot column enters through b_i O_0, unrounded) with the robot row p in its
    first row, and O.  Everything else -- the row scalars a, b, the p-weighted sum, the last layer, the head -- stays float64.
    Its deviation from reference64 is what f16 inputs cost on the run's data; a kernel further from reference64 than this
    restatement by more than an f32 form's error has a defect that is not rounding."""
    run = RUN[run_id]
    assert run.L == 3 and NORM[short(run)] == 0, run_id
    cr, humans = inputs(run_id)
    P, A, H = cr.shape[0], cr.shape[1], run.H
    Pm = params(run, torch.float64)
    g = Pm.ve_graph
    f16 = lambda t: t.half().double()
    with torch.no_grad():
        X = orc.rgl_embed(cr.double().reshape(P * A, 1, 9), humans.double()[:, None].expand(P, A, H, 5).reshape(P * A, H, 5), g)
        S = X @ g["w_a"] @ X.transpose(1, 2) if run.sim == "embedded_gaussian" else X @ X.transpose(1, 2)
        Adj = torch.softmax(S, dim=2)
        skip = (lambda new, old: new + old) if run.skip else (lambda new, old: new)
        H1 = skip(torch.relu(Adj @ X @ g["Ws.0"]), X)
        O = f16(H1) @ f16(g["Ws.1"])                                   # f32 accumulators in the kernel: not rounded again
        p = Adj[:, 0, :]
        D0 = torch.einsum("bj,bjf->bf", f16(p), f16(O))
        H2_0 = skip(torch.relu(D0), H1[:, 0])
        t = p[:, :1] * H2_0
        if H > 0:
            Sc = S[:, 1:, 1:]
            msh = Sc.max(dim=2, keepdim=True).values
            E = torch.exp(Sc - msh)
            m = torch.maximum(msh, S[:, 1:, :1])
            al, be = torch.exp(msh - m), torch.exp(S[:, 1:, :1] - m)
            Z = al * E.sum(dim=2, keepdim=True) + be
            D = f16(E) @ f16(O[:, 1:])
            H2 = skip(torch.relu(al / Z * D + be / Z * O[:, :1]), H1[:, 1:])
            t = t + torch.einsum("bj,bjf->bf", p[:, 1:], H2)
        H3_0 = skip(torch.relu(t @ g["Ws.2"]), H2_0)
        out = orc.mlp_forward(H3_0, orc.mlp_layers(Pm.value_network, ""), last_relu=False)
    out = out.numpy().reshape(P, A)
    out.setflags(write=False)
    return out
