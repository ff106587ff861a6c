"""rgl_scene_backward_kernel of csrc/rgl_backward.hip where no other kernel can take the call: the case table of the configurations the
tile pipeline refuses (tests/graph_forms.py: REFUSED), the launch each run takes (asked of the library: rgl_plan_scene_backward and
rgl_plan_graph_tiles, host only) and the float64 references (tests/row_forms.py's).  Nothing here needs a GPU.

The kernel is one workgroup of 1024 threads per scene with every activation of the scene in LDS; every loop over a scene's entries is
`for (idx = threadIdx.x; idx < n; idx += 1024)`, so a loop's SECOND pass begins where n passes 1024: N * N from N = 33, N * x_dim from
N = 33 (x_dim 32) or 17 (x_dim 64), N * hid of the pair MLP (hid = 2 x_dim: 64, the only width RGL builds -- the configuration does not
expose it) from N = 17.  Beyond 4096 scenes a workgroup walks scenes b, b + 4096, ..; reduce_slabs_kernel adds the scenes' slabs in
blocks of 256, 16 at a time with a tail.

  family   cc concatenation (the pair MLP: P, Q, dP, dQ, two ReLU masks), plain and layerwise (the `first ? acc : g + acc` accumulation
           of all four pair-MLP gradients); colw / cslw layerwise cosine, cosine_softmax (the cosine block re-entered per layer); lw
           layerwise eg / ga / sq outside the pipeline (x_dim 64, more than 32 nodes: w_a accumulated over layers); deep L = 4, 8
           (RGL_MAX_GCN_LAYERS) and 0, plain and layerwise; wide 65 and 80 nodes with narrow embeddings; limit the largest H that fits the
           LDS of a CU for three models (LIMITS; H + 1 is refused: REFUSALS); batch S = 1, 100, 257, 273 and the walking pair
  route    of the upstream gradient: value, motion (detach False and True), rgl -- as in tests/graph_forms.py

num_layer = 0: validate_graph accepts it, the kernel has a branch for it and rga.RGL builds such a model (H_L = X: the general
forward kernel runs it), so there is a run per route.  torch gives the similarity block's parameters NO gradient then (the adjacency
is never used); the kernel writes zeros, which tests/test_per_scene_backward.py asserts to be exact.

The walking pair: WALK has S = 4101 scenes (five workgroups take a second scene) and an upstream gradient that is zero for scenes 0 to
4095 (`dark`); WALK_TAIL is scenes 4096 to 4100 of the same sequence launched alone (`first`).  Their gradients are bit-identical: a
workgroup's second scene owes nothing to its first, and the slabs of dark scenes are zeros.

Seeds: the first of 0, 1, 2, .. (at most 64) at which the float32 and the float64 oracle agree on every ReLU mask with margin >= 24 (8 is
asserted), entries that are exactly 0 in both evaluations left out (`zeros_decided`: row_forms.reference) -- with `concatenation` the
adjacency is not normalised, a node whose whole row is closed has T_i = 0 and GCN pre-activations that are 0 in any precision.  For
a concatenation run the seed must also leave the graph alive: at many seeds the pair MLP's output ReLU is closed for EVERY pair (A = 0:
the margin is then easy and the run tests nothing), so at least a tenth of every adjacency's entries are open; a layerwise run with
parameters in the block has every layer's contribution at 10 regression bounds (the sensitivity tests/test_per_scene_backward_cpu.py
asserts); and the 33-node concatenation runs (one scene each: two gave no seed) have closed entries beyond the first 1024.
"""
import collections
import ctypes
import functools

import numpy as np
import torch

from relationalgraphlearning_amd import _native as nat
from oracle import rgl_oracle as orc
from tests import graph_forms as gf
from tests import row_forms as rf

# graph_forms.Run and: first, dark (row_forms.scenes / upstream), zeros_decided (row_forms.reference)
Run = collections.namedtuple("Run", gf.Run._fields + ("first", "dark", "zeros_decided"))
NARROW_MOTION = [5]


def _p(id, route, sim, H, L, S=3, X=32, lw=False, skip=True, narrow=False, head=None, seed=0, first=0, dark=0):
    """narrow: w_r [X], w_h [X] and a one-layer head, as graph_forms' CAP run."""
    head = head or (([1] if route == "value" else NARROW_MOTION) if narrow else
                    (rf.SHIPPED_V if route == "value" else (rf.SHIPPED_M if route == "motion" else [])))
    if route == "rgl":
        head = []
    return Run(id, route, X, [X] if narrow else [64, X], [X] if narrow else [64, X], list(head), S, H, seed, {}, L, gf.SIMS[sim], lw, skip,
               1, False, None, False, first, dark, True)


RUNS = [
    # concatenation, one adjacency: N = 2, 6, 17 (N hid: second pass), 20, 33 (N N: second pass), x_dim 64; L 1-3; skip on and off
    _p("cc-N2-L1-value", "value", "cc", 1, 1),
    _p("cc-N6-L2-motion", "motion", "cc", 5, 2, skip=False),
    _p("cc-N6-L3-rgl", "rgl", "cc", 5, 3),
    _p("cc-N17-L1-value", "value", "cc", 16, 1, skip=False),
    _p("cc-N20-L2-value", "value", "cc", 19, 2, skip=False, seed=18),
    _p("cc-N20-L1-motion", "motion", "cc", 19, 1, S=2, seed=2),
    _p("cc-N33-L2-value", "value", "cc", 32, 2, S=1, seed=13),
    _p("cc-N33-L1-rgl", "rgl", "cc", 32, 1, S=1, skip=False, seed=13),
    _p("cc-x64-N6-L2-value", "value", "cc", 5, 2, X=64),
    # concatenation, an adjacency per layer: all four pair-MLP gradients accumulated over the layers
    _p("cclw-N6-L2-value", "value", "cc", 5, 2, lw=True),
    _p("cclw-N6-L3-motion", "motion", "cc", 5, 3, lw=True, skip=False),
    _p("cclw-N2-L4-rgl", "rgl", "cc", 1, 4, lw=True),
    _p("cclw-N20-L2-motion", "motion", "cc", 19, 2, S=2, lw=True, seed=32),
    _p("cclw-N33-L2-value", "value", "cc", 32, 2, S=1, lw=True, skip=False, seed=36),
    # layerwise cosine and cosine_softmax: L 1-3, N = 2, 6, 20, 34, x_dim 64
    _p("colw-N2-L1-value", "value", "co", 1, 1, lw=True),
    _p("colw-N6-L2-motion", "motion", "co", 5, 2, lw=True, skip=False),
    _p("colw-N20-L3-rgl", "rgl", "co", 19, 3, lw=True),
    _p("colw-N34-L2-value", "value", "co", 33, 2, lw=True, skip=False),
    _p("cslw-N2-L3-motion", "motion", "cs", 1, 3, lw=True),
    _p("cslw-N6-L1-rgl", "rgl", "cs", 5, 1, lw=True, skip=False),
    _p("cslw-N20-L2-value", "value", "cs", 19, 2, lw=True),
    _p("cslw-N34-L1-motion", "motion", "cs", 33, 1, lw=True, skip=False, seed=1),
    _p("cslw-x64-N6-L2-value", "value", "cs", 5, 2, X=64, lw=True),
    _p("colw-x64-N17-L2-rgl", "rgl", "co", 16, 2, X=64, lw=True),
    # layerwise softmax / squared graphs outside the pipeline: x_dim 64; 33 and 40 nodes
    _p("eglw-x64-N6-L2-value", "value", "eg", 5, 2, X=64, lw=True),
    _p("galw-x64-N6-L3-motion", "motion", "ga", 5, 3, X=64, lw=True, skip=False),
    _p("sqlw-x64-N6-L2-rgl", "rgl", "sq", 5, 2, X=64, lw=True),
    _p("eglw-N33-L2-motion", "motion", "eg", 32, 2, lw=True),
    _p("galw-N33-L3-value", "value", "ga", 32, 3, lw=True, skip=False),
    _p("sqlw-N40-L2-value", "value", "sq", 39, 2, lw=True, skip=False),
    _p("eglw-N40-L3-rgl", "rgl", "eg", 39, 3, lw=True),
    # depth: L = 4 and L = 8, plain and layerwise, a softmax, a cosine and a concatenation graph each
    _p("eg-L4-N6-value", "value", "eg", 5, 4),
    _p("co-L4-N6-motion", "motion", "co", 5, 4, skip=False),
    _p("cc-L4-N6-rgl", "rgl", "cc", 5, 4),
    _p("eg-L8-N6-motion", "motion", "eg", 5, 8),
    _p("co-L8-N20-value", "value", "co", 19, 8),
    _p("cc-L8-N6-value", "value", "cc", 5, 8),
    _p("galw-L4-N6-motion", "motion", "ga", 5, 4, lw=True),
    _p("cslw-L4-N6-value", "value", "cs", 5, 4, lw=True, skip=False),
    _p("eglw-L8-N6-value", "value", "eg", 5, 8, lw=True),
    _p("colw-L8-N6-rgl", "rgl", "co", 5, 8, lw=True),
    _p("cclw-L8-N3-value", "value", "cc", 2, 8, lw=True),
    # no GCN layer: H_L = X; the block's parameters receive zeros (torch: no gradient at all)
    _p("eg-L0-N6-value", "value", "eg", 5, 0),
    _p("cc-L0-N6-motion", "motion", "cc", 5, 0),
    _p("co-L0-N6-rgl", "rgl", "co", 5, 0),
    # many nodes, narrow embeddings (80 nodes fit the LDS of a CU at x_dim 16 only: the narrow model's limit at x_dim 32 is 75)
    _p("eg-N65-L1-value", "value", "eg", 64, 1, S=2, narrow=True),
    _p("sq-N80-L1-motion", "motion", "sq", 79, 1, S=2, X=16, narrow=True, skip=False),
    _p("co-N80-L1-rgl", "rgl", "co", 79, 1, S=2, X=16, narrow=True),
    # batch: S = 1, 100 (the reference's), 257 and 273 (reduce_slabs_kernel: a second block; a 16-unrolled step and a tail in it)
    _p("cslw-N6-L2-value-S1", "value", "cs", 5, 2, S=1, lw=True),
    _p("cc-N3-L2-value-S100", "value", "cc", 2, 2, S=100, seed=4),
    _p("colw-N6-L2-motion-S257", "motion", "co", 5, 2, S=257, lw=True, seed=3),
    _p("cclw-N3-L2-value-S273", "value", "cc", 2, 2, S=273, lw=True, narrow=True, seed=2),
    # the walking pair
    _p("WALK", "value", "cc", 2, 2, S=4101, lw=True, narrow=True, dark=4096, seed=2),
    _p("WALK-TAIL", "value", "cc", 2, 2, S=5, lw=True, narrow=True, first=4096, seed=2),
]
WALK, WALK_TAIL = "WALK", "WALK-TAIL"
VALID = "cc-N2-L1-value"            # the call that must still be right after a refusal

# the LDS limit: (id, route, similarity, L, layerwise, narrow, scenes); H comes from the export (limit_H)
LIMIT_MODELS = [
    ("limit-cc-value", "value", "cc", 2, False, False, 1),
    ("limit-cslw-motion", "motion", "cs", 2, True, False, 2),
    ("limit-eg-narrow-value", "value", "eg", 1, False, True, 2),
]
LIMIT_SEEDS = {"limit-cc-value": 18, "limit-cslw-motion": 0, "limit-eg-narrow-value": 0}


# ---------------------------------------------------------------------------------------------------------------------------
# the library's plans
# ---------------------------------------------------------------------------------------------------------------------------
def _mlp(dims, last_relu):
    m = nat.RglMlp()
    m.n_layers, m.last_relu = len(dims) - 1, int(last_relu)
    for i, d in enumerate(dims):
        m.dims[i] = d
    for l in range(len(dims) - 1):          # validated as the launch validates them (not NULL); never read on the host
        m.weight[l] = m.bias[l] = 4096
    return m


def descriptors(run, H=None):
    """(graph, value head or None, motion head or None) of the run with dimensions and flags only."""
    g = nat.RglGraph()
    g.w_r, g.w_h = _mlp([9] + list(run.wr), True), _mlp([5] + list(run.wh), True)
    g.x_dim, g.num_layer, g.similarity = run.X, run.L, nat.SIMILARITY[run.sim]
    g.layerwise_graph, g.skip_connection = int(run.lw), int(run.skip)
    if run.sim == "embedded_gaussian":
        g.w_a = 4096
    if run.sim == "concatenation":
        g.w_a_mlp = _mlp([2 * run.X, 2 * run.X, 1], True)
    for l in range(run.L):
        g.Ws[l] = 4096
    head = _mlp([run.X] + list(run.head), False) if run.module != "rgl" else None
    return g, (head if run.module == "value" else None), (head if run.module == "motion" else None)


def plan(run, H=None, S=None):
    """rgl_plan_scene_backward for the run (at H humans and S scenes instead of its own, if given): a dict of the plan's fields."""
    g, vh, mh = descriptors(run)
    p = nat.RglSceneBackwardPlan()
    ref = lambda m: ctypes.byref(m) if m is not None else None
    nat.check(nat.lib().rgl_plan_scene_backward(ctypes.byref(g), ref(vh), ref(mh), run.S if S is None else S,
                                                run.H if H is None else H, ctypes.byref(p)), "rgl_plan_scene_backward")
    return {k: int(getattr(p, k)) for k, _ in nat.RglSceneBackwardPlan._fields_ if k != "reserved"}


def covered(run):
    """The tile pipeline's answer for the run's graph, forward or backward build."""
    return any(gf.plan(run, backward)["covered"] for backward in (False, True))


def _limit_run(entry, H, seed=0):
    id, route, sim, L, lw, narrow, S = entry
    return _p(id, route, sim, H, L, S=S, lw=lw, narrow=narrow, seed=seed)


@functools.lru_cache(maxsize=None)
def limit_H(id):
    """The largest H at which the export says the model's scene fits the LDS of a CU."""
    entry = [e for e in LIMIT_MODELS if e[0] == id][0]
    probe = _limit_run(entry, 1)
    fits = [H for H in range(1, nat.MAX_NODES - 1) if plan(probe, H=H)["fits"]]
    assert fits and fits == list(range(1, fits[-1] + 1)) and fits[-1] + 1 < nat.MAX_NODES, (id, fits[-3:])
    return fits[-1]


LIMITS = [_limit_run(e, limit_H(e[0]), LIMIT_SEEDS[e[0]]) for e in LIMIT_MODELS]
REFUSALS = [_limit_run(e, limit_H(e[0]) + 1)._replace(id=e[0] + "-plus-1") for e in LIMIT_MODELS]
RUNS = RUNS + LIMITS
RUN = {r.id: r for r in RUNS}
rf.TABLES["scene_backward"] = dict(RUN, **{r.id: r for r in REFUSALS})


def reference(run, detach=False):
    return rf.reference(run.id, detach, "scene_backward")


def short(run):
    return [k for k, v in gf.SIMS.items() if v == run.sim][0]


def family(run):
    """cc | cclw | colw | cslw | lw (layerwise eg / ga / sq) | plain (one adjacency of the other functions: depth and many nodes)."""
    s = short(run)
    if s == "cc":
        return "cclw" if run.lw else "cc"
    if run.lw:
        return s + "lw" if s in ("co", "cs") else "lw"
    return "plain"


def block_parameters(run):
    """Names of the similarity block's parameters (graph.<state-dict key>): w_a, or the pair MLP's four."""
    if run.sim == "embedded_gaussian":
        return ["graph.w_a"]
    if run.sim == "concatenation":
        return ["graph.w_a.0.weight", "graph.w_a.0.bias", "graph.w_a.2.weight", "graph.w_a.2.bias"]
    return []


# ---------------------------------------------------------------------------------------------------------------------------
# what the float64 reference says about a run, and how far it moves when the kernel's accumulations go wrong
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adjacency(run_id):
    """The float64 oracle's adjacencies of a run: a list (one per similarity call) of [S][N][N] arrays."""
    run, seen, inner = RUN[run_id], [], orc.similarity_matrix

    def recording(X, gsd, mode):
        A = inner(X, gsd, mode)
        seen.append(A.detach().numpy().copy())
        return A
    orc.similarity_matrix = recording
    try:
        rf.oracle(run, torch.float64)
    finally:
        orc.similarity_matrix = inner
    return seen


def _variant(run, similarity):
    """The float64 gradients of the run with orc.similarity_matrix replaced by similarity(inner, call index, X, gsd, mode)."""
    inner, calls = orc.similarity_matrix, [0]

    def patched(X, gsd, mode):
        calls[0] += 1
        return similarity(inner, calls[0] - 1, X, gsd, mode)
    orc.similarity_matrix = patched
    try:
        return rf.oracle(run, torch.float64)[1]
    finally:
        orc.similarity_matrix = inner


def without_layer(run, layer):
    """The float64 gradients when layer `layer`'s pass through the similarity block adds nothing to the block's parameter gradients
    (what `gW[idx] = acc` instead of `first ? acc : gW[idx] + acc` loses, for one layer)."""
    keys = [k[len("graph."):] for k in block_parameters(run)]

    def sim(inner, call, X, gsd, mode):
        return inner(X, dict(gsd, **{k: gsd[k].detach() for k in keys}) if call == layer else gsd, mode)
    return _variant(run, sim)


def without_column_term(run):
    """The float64 gradients of a cosine-family run when the norm m_j enters C_ij = S_ij / (m_i m_j) as a constant in its column role:
    dm loses sum_j dC_ji C_ji."""
    def sim(inner, call, X, gsd, mode):
        S = torch.matmul(X, X.transpose(1, 2))
        m = torch.norm(S, dim=2, keepdim=True)
        C = S / torch.matmul(m, m.detach().transpose(1, 2))
        return C if mode == "cosine" else torch.softmax(C, dim=2)
    return _variant(run, sim)


def without_mask_beyond(run, n=1024):
    """The float64 gradients of a concatenation run when the output ReLU's mask is applied to the first `n` entries of a scene's
    adjacency (row-major [N][N]) only: a closed entry beyond them passes its gradient on as if it were open."""
    def sim(inner, call, X, gsd, mode):
        B, N, xd = X.shape
        xi, xj = X.unsqueeze(2).expand(B, N, N, xd), X.unsqueeze(1).expand(B, N, N, xd)
        z = orc.mlp_forward(torch.cat([xi, xj], dim=3).reshape(B, N * N, -1), orc.mlp_layers(gsd, "w_a."), last_relu=False)
        z = z.reshape(B, N * N)
        leak = ((torch.arange(N * N) >= n) & (z.detach() <= 0)).to(z.dtype)
        return (torch.clamp(z, min=0) + (z - z.detach()) * leak).reshape(B, N, N)
    return _variant(run, sim)
