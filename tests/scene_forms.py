"""scene_graph_kernel<NT, SK, WAVES, CH, SPLIT, EMB, BX> of csrc/rgl_scene.hip (body: csrc/rgl_scene_body.h) -- the one-wave-per-scene
MFMA forward -- in every f32 form it launches: the table of runs, the form each takes (stated here from the header's rules, and asked
of the library: rgl_plan_scene_forward, host only) and the float64 / float32 references.  Nothing here needs a GPU; building the
table asks the planner for the walking runs' scene counts, so the library must be built.

  instantiations  (NT, SK, WAVES, SPLIT, EMB), each with and without the riding reward work (CH): 28
                  NT 1: embeddings inside, and SK 0..3 unsplit;  NT 2 | 4: embeddings inside + split, SK 0..2 split and unsplit, SK 3
                  unsplit;  NT 3: SK 0..3;  NT 8: SK 0..2 (always split).  The three bf16x6 instantiations are only REPORTED here
                  (tests/test_bf16x6_kernels.py holds their numbers).
  SK              0 softmax (embedded_gaussian eg, gaussian ga: Wa = I), 1 plain weights (squared sq, equal_attention eq, diagonal
                  di), 2 cosine (co, cosine_softmax cs), 3 concatenation (cc)
  routes          forward   nets.graph_forward with the value head (value rows + the head's row kernel) or the motion head,
                            scenes_per_crowd 1 | 3
                  expand    TreeSearch.expand: the state predictor of P parents, the level's reward work offered to the launch
                  children  TreeSearch.value_children of graphs the shared-crowd kernels do not cover (cosine, cosine_softmax,
                            concatenation, layerwise): crowds_per = A, value rows
                  pathg     gcn_search().search: 6 / 7-wide inputs through row_mlp2_pair_kernel<6, 7>, value rows

Edge runs (kind "edge", all `forward`): for every NT and every SK it has, N = 16 (NT - 1) + {1, 4, 5, 8, 9, 12, 13, 16} -- the node
counts at which last_steps = (N - 16 (NT - 1) + 3) >> 2 changes and the ones just before.  NT 1 begins at N = 2 (N = 1 has no human:
RGL_ERR_BAD_SHAPE).  NT 8 has them in its last tile (113 .. 128), and 65, 68, 80, 96, 112 -- last tiles of padding only -- in
"wide" runs.  Over the eight N of an (NT, SK) the runs rotate L = 1..4, skip, layerwise, the similarity of the family, the head and
the dealing: fewer scenes than a workgroup's slots, one more than a multiple of them (the split forms' idle slot), scenes_per_crowd
3 with crowd boundaries inside a workgroup and across two.

Walking runs (kind "walk"): n_scenes = grid_cap x slots + slots + 1 (+ up to 2: whole crowds) BY THE PLANNER, for unsplit NT 1 | 2,
split NT 2, NT 3, split and unsplit NT 4 and NT 8 -- the smallest H of the NT, the forward route, a plain-weight similarity (so that
a launch of a few of its scenes takes the same instantiation: a softmax run of few scenes embeds inside).

Teeth (`teeth`): how far reference64 moves when (a) the last human is dropped, (b) the first human of the last node tile is dropped,
(c) the last k-step group of the last tile -- its last N - 4 (last_steps - 1) - 16 (NT - 1) nodes -- is dropped, (d) scene s is given
crowd s + 1.  What does not apply, by construction of the similarity:
  diagonal          A = I: no node reads another.  (a), (b), (c) move nothing; the runs have the motion head, whose every row is an
                    output, so a dropped node shows as that row itself, and (d) applies.
  concatenation     no node permutation in the last tile (last_steps = 4 always): (c) is not a form of that kernel.
  N <= 4            one k-step holds every node, the robot included: (c) would drop the whole scene.
"""
import collections
import ctypes
import functools
import os

import numpy as np
import torch

from oracle import rgl_oracle as orc
from relationalgraphlearning_amd import _native as nat
from tests import golden_io as gio
from tests.deep_forms import REG_F32, TOL, error, seeded_scenes

Run = collections.namedtuple("Run", "id route H L sim lw skip flavour head spc P seed kind table expect")
SIMS = {"eg": "embedded_gaussian", "ga": "gaussian", "sq": "squared", "eq": "equal_attention", "di": "diagonal",
        "co": "cosine", "cs": "cosine_softmax", "cc": "concatenation"}
SHORT = {v: k for k, v in SIMS.items()}
FAMILY = {"eg": 0, "ga": 0, "sq": 1, "eq": 1, "di": 1, "co": 2, "cs": 2, "cc": 3}
FAMILIES = {0: ("eg", "ga"), 1: ("sq", "eq", "di"), 2: ("co", "cs"), 3: ("cc",)}
# the 28 f32 instantiations as (NT, SK, WAVES, SPLIT, EMB)
INSTANTIATIONS = [(1, 0, 8, 0, 1)] + [(1, k, 8, 0, 0) for k in range(4)] + \
                 [i for nt, w in ((2, 8), (4, 4)) for i in [(nt, 0, 8, 1, 1)] + [(nt, k, 8, 1, 0) for k in range(3)] + [(nt, k, w, 0, 0) for k in range(4)]] + \
                 [(3, k, 4, 0, 0) for k in range(4)] + [(8, k, 8, 1, 0) for k in range(3)]
BF16X6_INSTANTIATIONS = [(2, 0, 8, 1, 1), (2, 0, 8, 1, 0), (2, 0, 8, 0, 0)]        # with BX: reported by the planner, not run here
SK_OF_NT = {1: (0, 1, 2, 3), 2: (0, 1, 2, 3), 3: (0, 1, 2, 3), 4: (0, 1, 2, 3), 8: (0, 1, 2)}
RESIDUES = (1, 4, 5, 8, 9, 12, 13, 16)
# what a forced environment changes in the launcher's rules (section 4's environments; tests/test_scene_forms_cpu.py asks the planner
# under each): (RGL_SCENE_SPLIT_BELOW, RGL_SCENE_EMBED_INSIDE, RGL_SCENE_CHILDREN_BELOW)
RULES = {"default": (None, True, 3072), "unsplit": (0, True, 3072), "split": (1000000, True, 3072), "noembed": (None, False, 3072),
         "ride0": (None, True, 0), "ride1": (None, True, 1000000)}
SCENE_ENVS = {"default": {}, "unsplit": {"RGL_SCENE_SPLIT_BELOW": "0"}, "split": {"RGL_SCENE_SPLIT_BELOW": "1000000"},
              "noembed": {"RGL_SCENE_EMBED_INSIDE": "0"}, "ride0": {"RGL_SCENE_CHILDREN_BELOW": "0"},
              "ride1": {"RGL_SCENE_CHILDREN_BELOW": "1000000"}}


def node_tiles(N):
    return 8 if N > 64 else (N + 15) // 16


def actions_of(run):
    return run.table[0] * run.table[1] + 1


def n_scenes(run):
    return run.P * actions_of(run) if run.route in ("children", "pathg") else run.P


def scenes_per_crowd(run):
    return actions_of(run) if run.route == "children" else (run.spc if run.route == "forward" else 1)


def expected(run, env="default", scenes=None):
    """The instantiation (NT, SK, WAVES, SPLIT, EMB, CH) of the run's launch under `env`, restated from the rules include/rgl_hip.h
    gives for rgl_plan_scene_forward -- tests/test_scene_forms_cpu.py holds it against the planner itself."""
    below, embed, ride_below = RULES[env]
    S = n_scenes(run) if scenes is None else scenes
    N = run.H + 1
    NT, SK = node_tiles(N), FAMILY[SHORT[run.sim]]
    split_below = below if below is not None else (3072 if NT == 2 else 4096)
    offered = run.route == "expand"
    riding = offered and S < ride_below
    emb = embed and not (offered and not riding) and run.route != "pathg" and SK == 0 and NT in (1, 2, 4) and S <= 512 and \
        (NT == 1 or S < split_below)
    if NT == 8:
        return (8, SK, 8, 1, 0, int(riding))
    if emb:
        return (NT, 0, 8, int(NT != 1), 1, int(riding))
    split = SK != 3 and NT in (2, 4) and S < split_below
    return (NT, SK, 8 if split or NT <= 2 else 4, int(split), 0, int(riding))


# ---------------------------------------------------------------------------------------------------------------------------
# the library's plan
# ---------------------------------------------------------------------------------------------------------------------------
def _mlp(dims, last_relu):
    m = nat.RglMlp()
    m.n_layers, m.last_relu = len(dims) - 1, int(last_relu)
    for i, d in enumerate(dims):
        m.dims[i] = d
    return m


def graph_of(sim, L, lw=False, skip=True, path_g=False):
    """The shipped graph's descriptor with dimensions and modes only: the planner export reads no pointer."""
    g = nat.RglGraph()
    g.w_r, g.w_h = _mlp((6 if path_g else 9, 64, 32), True), _mlp((7 if path_g else 5, 64, 32), True)
    g.x_dim, g.num_layer, g.similarity, g.layerwise_graph, g.skip_connection = 32, L, nat.SIMILARITY[sim], int(lw), int(skip)
    if sim == "concatenation":
        g.w_a_mlp = _mlp((64, 64, 1), True)
    return g


def plan_of(g, motion, S, spc, H, image=False, reward=False):
    p = nat.RglSceneForwardPlan()
    nat.check(nat.lib().rgl_plan_scene_forward(ctypes.byref(g), int(motion), S, spc, H, int(image), int(reward), ctypes.byref(p)),
              "rgl_plan_scene_forward")
    out = {k: int(getattr(p, k)) for k, _ in nat.RglSceneForwardPlan._fields_ if k != "reserved"}
    out["inst"] = (out["node_tiles"], out["family"], out["waves"], out["split"], out["embed_inside"], out["children_riding"]) if out["covered"] else None
    return out


def plan(run, scenes=None):
    """rgl_plan_scene_forward for the run's launch (under this process's switches): a dict of the plan's fields and `inst`."""
    return plan_of(graph_of(run.sim, run.L, run.lw, run.skip, run.route == "pathg"), run.head == "motion",
                   n_scenes(run) if scenes is None else scenes, scenes_per_crowd(run), run.H, False, run.route == "expand")


def form(p):
    if not p["covered"]:
        return "not the scene kernel"
    nt, sk, w, split, emb, ch = p["inst"]
    return "NT=%d SK=%d %d waves%s%s%s, grid %d of at most %d x %d slots, last_steps %d" % (
        nt, sk, w, " split" if split else "", " embeddings inside" if emb else "", " + reward work" if ch else "", p["grid"], p["grid_cap"],
        p["slots"], p["last_steps"])


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
# seeds of the edge runs: the first of 0, 1, 2, .. at which every tooth that applies moves the float64 reference by 15 x the run's
# regression bound (test_scene_forms_cpu asserts 10 x); runs not listed meet it at seed 0
SEEDS = {'forward-N113-L1-eg-value-P1': 6, 'forward-N120-L2-ga-lw-value-P2': 1}


def _r(route, N, L, sim, kind, head="value", lw=False, skip=True, flavour="trained", spc=1, P=3, seed=None, table=(1, 4), tag=""):
    table = (5, 16) if route == "pathg" else table          # path G searches the CADRL table: 5 speeds x 16 rotations + 1
    id = "%s-N%d-L%d-%s%s%s-%s%s-P%d%s%s" % (route, N, L, sim, "-lw" if lw else "", "" if skip else "-noskip", head, "" if spc == 1 else "-spc%d" % spc,
                                             P, "" if flavour == "trained" else "-" + flavour, tag)
    run = Run(id, route, N - 1, L, SIMS[sim], lw, skip, flavour, head, spc, P, SEEDS.get(id, 0) if seed is None else seed, kind, table, None)
    return run._replace(expect=expected(run))


def slots_few(nt, sk):
    """Slots of a workgroup of the form a FEW scenes of (NT, SK) take without switches."""
    return {1: 8, 2: 8 if sk == 3 else 4, 3: 4, 4: 4 if sk == 3 else 2, 8: 1}[nt]


def _edge(nt, sk):
    """The eight last-tile edges of (NT, SK), rotating the run-time forms and the dealing."""
    s = slots_few(nt, sk)
    few = 3 if s >= 4 else 1
    dealing = [(few, 1), (2 * s + 1, 1), (9, 3), (s + 1, 1), (15, 3), (few + 1, 1), (3 * s + 1, 1), (12, 3)]
    runs = []
    for i, res in enumerate(RESIDUES):
        N = 16 * (nt - 1 if nt < 8 else 7) + res
        if N == 1:
            N = 2
        sim = FAMILIES[sk][i % len(FAMILIES[sk])]
        L = 1 + (3 * i + i // 4 + sk) % 4          # 1, 4, 3, 2, 2, 1, 4, 3 (+ SK): every similarity of a family meets short and long stacks
        lw = i in (3, 6) and sim not in ("eq", "di")
        skip = i % 3 != 2
        head = "motion" if sim == "di" else ("value", "motion")[(i // 2 + i + nt) % 2]
        P, spc = dealing[(i + sk) % 8]
        runs.append(_r("forward", N, L, sim, "edge", head, lw, skip, spc=spc, P=P))
    return runs


# switches the library reads once per process and that change the form of a launch
SWITCHES = ("RGL_SCENE_SPLIT_BELOW", "RGL_SCENE_EMBED_INSIDE", "RGL_SCENE_CHILDREN_BELOW", "RGL_SCENE_WIDE_SLOTS", "RGL_FORCE_GENERIC",
            "RGL_TILES_FORWARD", "RGL_REQUIRE_MFMA_FORWARD", "RGL_REQUIRE_MFMA_CHILDREN", "RGL_CONTRACT_F32_AS")
# A process under one of the forced environments cannot ask its own planner for the walking runs' scene counts (the answer would be
# that environment's): the process that starts it hands its own table's counts on in this variable, in the order of the table.
WALK_SCENES = "RGL_TEST_SCENE_FORMS_WALK_SCENES"


def _walk_scenes(N, sim, spc, probe, head="value"):
    """n_scenes just above grid_cap x slots of the form `probe` scenes take, by the planner; whole crowds."""
    if WALK_SCENES in os.environ:
        return _given.pop(0)
    assert not any(k in os.environ for k in SWITCHES[:5]), "a forced environment without %s" % WALK_SCENES
    run = _r("forward", N, 2, sim, "walk", head, spc=spc, P=-(-probe // spc) * spc)
    p = plan(run)
    P = p["grid_cap"] * p["slots"] + p["slots"] + 1
    return -(-P // spc) * spc


_given = [int(v) for v in os.environ.get(WALK_SCENES, "").split(",") if v]


def _table():
    runs = []
    for nt, sks in SK_OF_NT.items():
        for sk in sks:
            runs += _edge(nt, sk)
    # the eight-tile form whose last tiles are padding only (last_steps = 0), and its first N
    runs += [_r("forward", 65, 2, "eg", "wide", "motion", P=2), _r("forward", 68, 3, "sq", "wide", P=3), _r("forward", 80, 1, "cs", "wide", "motion", skip=False, P=2),
             _r("forward", 96, 4, "ga", "wide", lw=True, P=2), _r("forward", 112, 2, "co", "wide", spc=3, P=6)]
    # more than 512 scenes: NT 1 softmax with its rows from the embedding launch; unsplit NT 2 at 3072 and more: every slot busy
    runs += [_r("forward", 10, 3, "eg", "many", "motion", P=517), _r("forward", 17, 2, "eq", "many", P=3077), _r("forward", 20, 1, "cs", "many", "motion", P=3074), _r("forward", 21, 3, "ga", "many", P=3073, skip=False)]
    # walking launches: the smallest N of the NT; plain weights, so that a few scenes alone take the same instantiation
    for N, sim, spc, probe, head in ((2, "sq", 3, 5000, "value"), (17, "sq", 1, 5000, "motion"), (17, "eq", 1, 2500, "value"), (33, "sq", 1, 5000, "value"),
                                    (49, "sq", 1, 2000, "value"), (49, "eq", 3, 5000, "motion"), (65, "sq", 1, 600, "value"),
                                    (49, "eg", 1, 5000, "value"), (49, "co", 1, 5000, "value")):
        runs.append(_r("forward", N, 2, sim, "walk", head, spc=spc, P=_walk_scenes(N, sim, spc, probe, head)))
    # raw random-init weights (features of 10..100): the north-star bound only
    runs += [_r("forward", N, 2, sim, "rand", head, flavour="rand", P=5) for N, sim, head in
             ((5, "eg", "value"), (21, "sq", "motion"), (37, "co", "value"), (53, "cc", "value"), (70, "ga", "motion"))]
    # the state predictor of a tree level, the reward work riding (CH) in every instantiation few scenes reach
    for N, sim, L, P in ((5, "eg", 2, 3), (6, "ga", 1, 9), (7, "eg", 3, 520), (9, "sq", 2, 600), (12, "co", 3, 5), (13, "cc", 2, 4),
                         (20, "eg", 2, 5), (21, "eg", 2, 600), (24, "di", 4, 7), (29, "cs", 2, 6), (32, "cc", 1, 9),
                         (33, "ga", 2, 5), (37, "eq", 3, 9), (40, "co", 2, 6), (48, "cc", 2, 5),
                         (49, "eg", 3, 3), (52, "eg", 2, 700), (53, "sq", 2, 5), (60, "cs", 1, 7), (64, "cc", 2, 6),
                         (65, "ga", 2, 3), (72, "eq", 2, 2), (128, "co", 2, 2)):
        runs.append(_r("expand", N, L, sim, "expand", "motion", P=P))
    # every child's graph in full: crowds_per = A = 11 (a crowd boundary inside every workgroup), value rows
    for N, sim, L, lw, P in ((6, "co", 2, False, 3), (20, "cs", 3, False, 2), (21, "eg", 2, True, 3), (40, "cc", 2, False, 2), (53, "co", 4, True, 2),
                             (66, "cs", 1, False, 1), (16, "sq", 2, True, 4)):
        runs.append(_r("children", N, L, sim, "children", lw=lw, P=P, table=(2, 5)))
    # path G: rotated 6 / 7-wide rows, 81 scenes per root (its weights are scaled random draws: the north-star bound only)
    runs += [_r("pathg", N, 2, "eg", "pathg", flavour="path_g", P=P) for N, P in ((6, 2), (20, 3), (36, 2), (50, 1), (66, 1))]
    # beyond the envelope
    runs += [_r("forward", 65, 2, "cc", "beyond", P=3), _r("forward", 6, 5, "eg", "beyond", P=3), _r("forward", 129, 2, "eg", "beyond", P=3)]
    return runs


RUNS = _table()
RUN = {r.id: r for r in RUNS}
assert len(RUN) == len(RUNS)
EDGE = [r for r in RUNS if r.kind == "edge"]
WALK = [r for r in RUNS if r.kind == "walk"]
assert not _given


def child_environment(switches):
    """os.environ without the switches above, with `switches` and this table's walking scene counts."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    env[WALK_SCENES] = ",".join(str(r.P) for r in WALK)
    return env
BEYOND = [r for r in RUNS if r.kind == "beyond"]
EXPAND = [r for r in RUNS if r.route == "expand"]
ANSWERED = [r for r in RUNS if r.kind != "beyond"]
VALID = [r.id for r in EDGE if r.H + 1 == 20 and FAMILY[SHORT[r.sim]] == 1][0]          # the call that must still be right after a refusal
# what each run beyond the envelope does: in the scene environments (the general kernel refused) and in the `generic` environment
REFUSALS = {BEYOND[0].id: ("RGL_ERR_BAD_MODE", "answers"), BEYOND[1].id: ("RGL_ERR_BAD_MODE", "answers"),
            BEYOND[2].id: ("RGL_ERR_BAD_SHAPE", "RGL_ERR_BAD_SHAPE")}


def walk_sample(run, p):
    """Scenes of a walking launch compared with a launch of their own (whole crowds): the first workgroups' slots, the turn of the
    first pass into the second (scene grid x slots), the middle, the last scenes of the launch."""
    S, spc, turn = n_scenes(run), scenes_per_crowd(run), p["grid"] * p["slots"]
    picks = list(range(0, 16)) + list(range(turn - 9, turn + 9)) + list(range(S // 2, S // 2 + 9)) + list(range(S - 9, S))
    crowds = sorted({s // spc for s in picks if 0 <= s < S})
    return [c * spc + k for c in crowds for k in range(spc)]


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(run_id):
    """float32 tensors.  forward: robot (S, 9), humans (S / spc, H, 5);  expand, pathg: robot (P, 9), humans (P, H, 5);  children:
    child_robot (P, A, 9), humans (P, H, 5)."""
    run = RUN[run_id]
    seed = 7300 + 11 * run.H + run.seed
    if run.route == "forward":
        robot, humans = seeded_scenes(seed, run.P, run.H)
        return robot, humans[:run.P // run.spc].contiguous()
    robot, humans = seeded_scenes(seed, run.P, run.H)
    if run.route == "children":
        acts, _ = orc.mprl_action_space(orc.OracleConfig(speed_samples=run.table[0], rotation_samples=run.table[1]), 1.0)
        return orc._children_robot(robot, acts, orc.OracleConfig()), humans
    return robot, humans


def checkpoint(run):
    """The state dicts of the run's policy; five layers (beyond the envelope): the golden sets hold four, Ws.4 repeats Ws.0."""
    ck = gio.checkpoint(run.flavour, min(run.L, 4), "separate", run.sim)
    for l in range(4, run.L):
        for g in ("graph_model1", "graph_model2"):
            ck[g]["Ws.%d" % l] = ck[g]["Ws.0"].clone()
    return ck


def config(run):
    return orc.OracleConfig(num_layer=run.L, similarity=run.sim, layerwise_graph=run.lw, skip_connection=run.skip,
                            speed_samples=run.table[0], rotation_samples=run.table[1])


def evaluate(run, a, humans, dtype):
    """The oracle over the run's scenes in `dtype` -> float64 array: forward (S, 1) | (S, H, 5), expand (P, H, 5), children (P, A),
    pathg (B, 81)."""
    cfg = config(run)
    with torch.no_grad():
        if run.route == "pathg":
            sd = {k: v.to(dtype) for k, v in gio.path_g_sd().items()}
            return orc.gcn_predict_batched(a.numpy(), humans.numpy(), sd, cfg, dtype=dtype)[1]
        Pm = orc.MprlParams.from_checkpoint({k: {kk: vv.to(dtype) for kk, vv in v.items()} for k, v in checkpoint(run).items()})
        H = humans.shape[1]
        if run.route == "children":
            P, A = a.shape[0], a.shape[1]
            out = orc.value_estimator_forward(a.to(dtype).reshape(P * A, 1, 9), humans.to(dtype)[:, None].expand(P, A, H, 5).reshape(P * A, H, 5),
                                              Pm.ve_graph, Pm.value_network, cfg)
            return out.double().numpy().reshape(P, A)
        S = a.shape[0]
        spc = S // humans.shape[0]
        hum = humans.to(dtype)[:, None].expand(S // spc, spc, H, 5).reshape(S, H, 5)
        if run.head == "motion":
            out = orc.state_predictor_humans(a.to(dtype).reshape(S, 1, 9), hum, Pm.sp_graph, Pm.motion_predictor, cfg)
        else:
            out = orc.value_estimator_forward(a.to(dtype).reshape(S, 1, 9), hum, Pm.ve_graph, Pm.value_network, cfg)
        return out.double().numpy()


@functools.lru_cache(maxsize=None)
def reference64(run_id):
    out = evaluate(RUN[run_id], *inputs(run_id), torch.float64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference32(run_id):
    """The same evaluation in float32 on the CPU: its deviation from reference64 is what the regression bound is measured against."""
    out = evaluate(RUN[run_id], *inputs(run_id), torch.float32)
    out.setflags(write=False)
    return out


def yardstick(run):
    return error(reference32(run.id), reference64(run.id))


def bounds(run):
    """(north-star bound, regression-level bound or None) of the run's output against reference64, both relative (deep_forms.error):
    TOL and max(REG_F32, 8 x the float32 oracle's deviation); raw random-init weights (and path G's): the north-star bound only."""
    return TOL, (None if run.flavour != "trained" else max(REG_F32, 8 * yardstick(run)))


def last_tile(N):
    return (N - 1) // 16


def teeth(run):
    """{tooth: how far (relative, as `error`) reference64 moves} for the teeth that apply to the run (see the module's docstring):
    "last human", "tile human", "step group" (dropped), "next crowd"."""
    assert run.route == "forward"
    robot, humans = inputs(run.id)
    want = reference64(run.id)
    H, N, sk = run.H, run.H + 1, FAMILY[SHORT[run.sim]]
    lt = last_tile(N)

    def dropped(drop):
        keep = [h for h in range(H) if h not in drop]
        got = evaluate(run, robot, humans[:, keep], torch.float64)
        return error(got, want[:, keep] if run.head == "motion" else want)
    out = {}
    if run.sim != "diagonal" and H >= 2:
        out["last human"] = dropped({H - 1})
        out["tile human"] = dropped({max(16 * lt - 1, 0)})
        steps = (N - 16 * lt + 3) >> 2
        group = N - 4 * (steps - 1) - 16 * lt
        if sk != 3 and N > 4 and H - group >= 1:
            out["step group"] = dropped(set(range(H - group, H)))
    if humans.shape[0] > 1 and not (run.sim == "diagonal" and run.head == "value"):
        out["next crowd"] = error(evaluate(run, robot, torch.roll(humans, -1, 0), torch.float64), want)
    return out
