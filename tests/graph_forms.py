"""graph_kernel<NT, XT, L, BWD, COS, LW> of csrc/rgl_graph_kernel.h -- the tile pipeline's similarity block, its normalisation,
the GCN layers and the way back -- in every instantiation launch_graph reaches: the case table, the instantiation and grid each
run takes (asked of the library: rgl_plan_graph_tiles, host only) and the float64 references (tests/row_forms.py's).  Nothing
here needs a GPU.

The kernel is persistent: grid = min(S, resident) workgroups, workgroup b walks scenes b, b + grid, ..; it prefetches the next
scene into registers, keeps the weight gradients in its accumulators over all its scenes and relies on the padding rows of its
LDS staying zero from one scene to the next.  A run whose S is at most `resident` (256 to 1536) gives every workgroup ONE scene
and sees none of that, so S here comes from the planner's `resident`: a "multi" run has S = 2 resident + 5 -- five workgroups
walk three scenes, the others two -- and there is one for each of the 42 (family, NT, XT, L) combinations, through the value
estimator or the state predictor, whose backward launches the forward build too.  Two of the 42 have no backward run: graph_kernel<4, 4, 3, true, *> (plain
and cosine) is compiled but no shape reaches it -- at x_dim 64 with three layers already the 33 nodes NT = 4 begins with take more
than a CU's LDS in the backward build -- and their forward builds run in forward-only runs: 82 instantiations.

  family   P plain (norm 0-3: embedded_gaussian eg, gaussian ga, squared sq, equal_attention eq, diagonal di), C cosine (norm 4-5:
           cosine co, cosine_softmax cs), W layerwise (eg, ga, sq; a layerwise eq / di graph IS the plain one: its adjacency is a
           constant)
  NT       node tiles: 1 (N <= 16), 2 (N <= 32), 4 (N <= 64);  XT feature tiles: 2 (x_dim 32), 4 (x_dim 64);  L layers 1-3
  route    of the upstream gradient: value (row 0, value estimator), motion (rows 1..H, state predictor, detach False and True),
           rgl (d_H on all rows: the graph model alone; its forward is the general kernel's, the backward the tile pipeline's)
  forward  forward-only runs: hl_row0 (value head: only the robot row is written), all rows (motion head), scenes_per_crowd 1 | 3

`inst` of a run states the instantiation it is there for as "family/NT/XT/L"; tests/test_graph_forms_cpu.py holds every such
statement, and the coverage conditions of the table, against the planner.

The embeddings: the runs of up to 32 nodes have the shipped w_r / w_h (9-64-X, 5-64-X).  The caller's workspace is n_scenes x
n_params floats, and the backward needs three [S][N][X] feature arrays and a slab per wave of every row job in it: beyond 32 nodes
that only fits a model with many parameters per scene in a job of few waves -- w_r 9-256-256-X (a row per scene) and w_h 5-X (a row
per human) there.  CAPPED is the run in which it does NOT fit at first: backward_tiles halves its cap until the graph kernel's
grid is below S.
"""
import collections
import ctypes

from relationalgraphlearning_amd import _native as nat
from tests import row_forms as rf

Run = collections.namedtuple("Run", "id module X wr wh head S H seed jobs L sim lw skip spc forward_only inst multi")
FAMILIES = ("P", "C", "W")
SIMS = {"eg": "embedded_gaussian", "ga": "gaussian", "sq": "squared", "eq": "equal_attention", "di": "diagonal",
        "co": "cosine", "cs": "cosine_softmax", "cc": "concatenation"}
NORMS = {"P": ("eg", "ga", "sq", "eq", "di"), "C": ("co", "cs"), "W": ("eg", "ga", "sq")}
NORM_INDEX = {"eg": 0, "ga": 0, "sq": 1, "eq": 2, "di": 3, "co": 4, "cs": 5}
COMBINATIONS = [("P", nt, xt, l) for nt in (1, 2, 4) for xt in (2, 4) for l in (1, 2, 3)] + \
               [("C", nt, xt, l) for nt in (1, 2, 4) for xt in (2, 4) for l in (1, 2, 3)] + \
               [("W", nt, 2, l) for nt in (1, 2) for l in (1, 2, 3)]
WIDE_R = [256, 256]                 # w_r's hidden layers beyond 32 nodes (see above)


def _g(id, route, sim, inst, H, S, seed=0, lw=False, skip=True, spc=1, fwd=False, multi=True, wide=None, head=None, wr=None, wh=None):
    fam, nt, xt, L = inst.split("/")
    X = 16 * int(xt)
    wide = H > 31 if wide is None else wide
    head = head or (rf.SHIPPED_V if route == "value" else (rf.SHIPPED_M if route == "motion" else []))
    return Run(id, route, X, wr or (WIDE_R if wide else [64]) + [X], wh or ([X] if wide else [64, X]), list(head), S, H, seed, {}, int(L),
               SIMS[sim], lw, skip, spc, fwd, inst, multi)


# seeds: the first of 0, 1, 2, .. at which the float32 and the float64 oracle agree on every ReLU mask -- the GCN layers' included --
# with three times the margin tests/test_graph_forms.py asserts (row_forms.reference: 24 where 8 is asserted)
RUNS = [
    # a multi-scene run for each reachable (family, NT, XT, L): S = 2 resident + 5
    _g("P12L1-eg-value", "value", "eg", "P/1/2/1", 1, 3077),
    _g("P12L2-ga-motion", "motion", "ga", "P/1/2/2", 5, 3077, skip=False, seed=2),
    _g("P12L3-sq-value", "value", "sq", "P/1/2/3", 15, 2053, skip=False, seed=1),
    _g("P14L1-eq-motion", "motion", "eq", "P/1/4/1", 6, 2053, skip=False),
    _g("P14L2-di-value", "value", "di", "P/1/4/2", 12, 1029, skip=False),
    _g("P14L3-eg-motion", "motion", "eg", "P/1/4/3", 2, 1029, seed=1),
    _g("P22L1-sq-value", "value", "sq", "P/2/2/1", 16, 2053, seed=1),
    _g("P22L2-eq-motion", "motion", "eq", "P/2/2/2", 31, 2053, skip=False),
    _g("P22L3-di-value", "value", "di", "P/2/2/3", 22, 1541, skip=False, seed=2),
    _g("P24L1-eg-motion", "motion", "eg", "P/2/4/1", 31, 1029, skip=False, seed=4),
    _g("P24L2-ga-value", "value", "ga", "P/2/4/2", 16, 1029, skip=False, seed=1),
    _g("P24L3-sq-motion", "motion", "sq", "P/2/4/3", 19, 517, seed=6),
    _g("P42L1-di-value", "value", "di", "P/4/2/1", 63, 517, skip=False),
    _g("P42L2-eg-motion", "motion", "eg", "P/4/2/2", 32, 517),
    _g("P42L3-ga-value", "value", "ga", "P/4/2/3", 48, 517, seed=3),
    _g("P44L1-sq-motion", "motion", "sq", "P/4/4/1", 63, 517, seed=13),
    _g("P44L2-eq-value", "value", "eq", "P/4/4/2", 43, 517),
    _g("C12L1-co-motion", "motion", "co", "C/1/2/1", 4, 3077),
    _g("C12L2-cs-value", "value", "cs", "C/1/2/2", 15, 3077),
    _g("C12L3-co-motion", "motion", "co", "C/1/2/3", 1, 3077, skip=False, seed=19),
    _g("C14L1-cs-value", "value", "cs", "C/1/4/1", 15, 1541),
    _g("C14L2-co-motion", "motion", "co", "C/1/4/2", 1, 1029, skip=False, seed=8),
    _g("C14L3-cs-value", "value", "cs", "C/1/4/3", 9, 517, skip=False, seed=2),
    _g("C22L1-cs-motion", "motion", "cs", "C/2/2/1", 31, 2053),
    _g("C22L2-co-value", "value", "co", "C/2/2/2", 16, 2053, seed=1),
    _g("C22L3-cs-motion", "motion", "cs", "C/2/2/3", 25, 1541, skip=False, seed=2),
    _g("C24L1-co-value", "value", "co", "C/2/4/1", 18, 1029, seed=2),
    _g("C24L2-cs-motion", "motion", "cs", "C/2/4/2", 31, 517, skip=False, seed=2),
    _g("C24L3-co-value", "value", "co", "C/2/4/3", 16, 517, skip=False, seed=1),
    _g("C42L1-co-motion", "motion", "co", "C/4/2/1", 32, 517, skip=False),
    _g("C42L2-cs-value", "value", "cs", "C/4/2/2", 63, 517, skip=False),
    _g("C42L3-cs-motion", "motion", "cs", "C/4/2/3", 37, 517, seed=1),
    _g("C44L1-co-value", "value", "co", "C/4/4/1", 40, 517, skip=False),
    _g("C44L2-co-motion", "motion", "co", "C/4/4/2", 32, 517, seed=11),
    _g("W12L1-eg-value", "value", "eg", "W/1/2/1", 5, 1029, lw=True, skip=False),
    _g("W12L2-ga-motion", "motion", "ga", "W/1/2/2", 15, 1029, lw=True),
    _g("W12L3-sq-value", "value", "sq", "W/1/2/3", 1, 1029, lw=True, skip=False),
    _g("W22L1-sq-motion", "motion", "sq", "W/2/2/1", 31, 1029, lw=True, seed=2),
    _g("W22L2-eg-value", "value", "eg", "W/2/2/2", 16, 1029, lw=True, skip=False, seed=1),
    _g("W22L3-ga-motion", "motion", "ga", "W/2/2/3", 21, 1029, lw=True, seed=2),
    # the third route, d_H on all rows, at every NT and in every family
    _g("P12L2-eg-rgl", "rgl", "eg", "P/1/2/2", 5, 3077),
    _g("C22L3-cs-rgl", "rgl", "cs", "C/2/2/3", 19, 2053, skip=False, seed=1),
    _g("P42L1-sq-rgl", "rgl", "sq", "P/4/2/1", 35, 517),
    _g("W22L2-ga-rgl", "rgl", "ga", "W/2/2/2", 17, 1029, lw=True),
    # layerwise graphs of constant adjacencies: the plain builds
    _g("P12L2-eq-value-lw", "value", "eq", "P/1/2/2", 5, 3077, lw=True, skip=False),
    _g("P22L3-di-motion-lw", "motion", "di", "P/2/2/3", 19, 2053, lw=True, seed=1),
    # forward only: the value head's robot row (hl_row0) and the motion head's all rows, sibling scenes sharing a crowd (spc = 3);
    # P/4/4/3 and C/4/4/3 have no backward run -- no scene of 33 nodes fits their backward build -- their forward build runs here
    _g("F-P14L2-eg-value-spc1", "value", "eg", "P/1/4/2", 5, 1029, fwd=True, seed=8),
    _g("F-C24L1-co-motion-spc3", "motion", "co", "C/2/4/1", 19, 1029, spc=3, fwd=True, seed=2),
    _g("F-P44L3-eg-value-spc3", "value", "eg", "P/4/4/3", 34, 519, spc=3, fwd=True, seed=231),
    _g("F-C44L3-cs-motion-spc1", "motion", "cs", "C/4/4/3", 32, 517, skip=False, fwd=True),
    _g("F-P42L2-sq-motion-spc3", "motion", "sq", "P/4/2/2", 63, 519, spc=3, fwd=True, seed=29),
    _g("F-W22L3-ga-value-spc3", "value", "ga", "W/2/2/3", 31, 1029, lw=True, spc=3, fwd=True, seed=4),
    # few scenes of many nodes and few parameters beside the graph's: the workspace holds 64 slabs of the graph kernel, not 150
    _g("CAP", "value", "eg", "P/2/4/3", 31, 150, seed=30, multi=False, wr=[64], wh=[64], head=[1]),
]
RUN = {r.id: r for r in RUNS}
CAPPED = "CAP"
VALID = "P12L1-eg-value"            # the call that must still be right after a refusal

# configurations the tile pipeline refuses (covered = 0): (id, similarity, layerwise, x_dim, H, L, seed)
REFUSED = [
    ("layerwise-cosine", "co", True, 32, 5, 2, 0),
    ("layerwise-cosine_softmax", "cs", True, 32, 5, 2, 0),
    ("layerwise-x64", "eg", True, 64, 5, 2, 0),
    ("layerwise-33-nodes", "sq", True, 32, 32, 2, 0),
    ("concatenation", "cc", False, 32, 5, 2, 1),
    ("65-nodes", "eg", False, 32, 64, 2, 0),
    ("4-layers", "eg", False, 32, 5, 4, 0),
]


def refused_run(entry):
    """A value-estimator run of a refused configuration: three scenes."""
    id, sim, lw, X, H, L, seed = entry
    return Run("refused-" + id, "value", X, [64, X], [64, X], list(rf.SHIPPED_V), 3, H, seed, {}, L, SIMS[sim], lw, True, 1, False, None, False)


rf.TABLES["graph"] = dict(RUN, **{refused_run(e).id: refused_run(e) for e in REFUSED})


def reference(run, detach=False):
    return rf.reference(run.id, detach, "graph")


# ---------------------------------------------------------------------------------------------------------------------------
# the library's plan
# ---------------------------------------------------------------------------------------------------------------------------
def plan(run, backward, max_workgroups=2048):
    """rgl_plan_graph_tiles for the run's graph: a dict of the plan's fields and `inst` ("family/NT/XT/L", None: not covered)."""
    g = nat.RglGraph()
    g.x_dim, g.num_layer, g.similarity, g.layerwise_graph = run.X, run.L, nat.SIMILARITY[run.sim], int(run.lw)
    p = nat.RglGraphTilesPlan()
    nat.check(nat.lib().rgl_plan_graph_tiles(ctypes.byref(g), run.S, run.H, int(backward), max_workgroups, ctypes.byref(p)),
              "rgl_plan_graph_tiles")
    out = {k: int(getattr(p, k)) for k, _ in nat.RglGraphTilesPlan._fields_}
    out["inst"] = "%s/%d/%d/%d" % (FAMILIES[out["family"]], out["node_tiles"], out["feature_tiles"], out["layers"]) if out["covered"] else None
    return out


def backward_cap(run):
    """The cap backward_tiles ends with: the first of 2048, 1024, .. at which the pipeline's intermediates fit the caller's workspace
    (row_forms.backward_workspace's accounting with the planner's grid; None: at none), as (cap, cap by the lower bound that leaves
    the row jobs' slabs out).  The two agree wherever the table relies on the cap."""
    caps = []
    for rows in (True, False):
        fits = [mw for mw in (1 << k for k in range(11, -1, -1))
                if (lambda u: u[0] <= u[1])(rf.backward_workspace(run, mw, plan(run, True, mw)["grid"], rows))]
        caps.append(fits[0] if fits else None)
    return tuple(caps)


def scenes_walked(run, grid):
    """(fewest, most) scenes a workgroup of the run walks on `grid` workgroups."""
    return run.S // grid, -(-run.S // grid)
