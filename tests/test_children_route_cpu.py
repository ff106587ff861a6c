"""Which kernel family takes a value-of-children call (route_value_children of csrc/rgl_fast.hip, read through the host-only export
rgl_plan_value_children), held to the ladder the launcher followed before the route existed -- on both sides of every boundary
that ladder has.  Nothing here needs a GPU.

The ladder (A = 81 children, the shipped embeddings and value head, a full workspace, unless a row says otherwise):
  1. a contraction mode other than f32 / f16 / bf16x6: RGL_ERR_BAD_MODE
  2. staged = a stage-2 head exists and the workspace holds mprl_value_children_workspace_bytes
  3. staged, not f16: FUSED (two layers, N <= 32, a row normalisation of the shared-crowd kernels, no layerwise graph, the shipped
     head; in f32 from RGL_FUSED_MIN_TILES = 1200 tiles of 16 children up; in bf16x6 at every size where the form fits a CU --
     N <= 16, and 17..20 with a softmax similarity -- and otherwise as the f32 form on an image the call packs itself)
  4. staged: RANK1 (not f16; two layers, N <= 32), then DEEP (two or three layers, tables within a CU's LDS: N <= 64 / 60; f16:
     three layers and a softmax similarity or RGL_ERR_BAD_MODE), then TILE (softmax similarities, any depth, N <= 64), then, not
     f16, SCENE (every similarity and layerwise graphs, N <= 128)
  5. not f16: TILES_FORWARD (any embedding MLPs, x_dim 32 | 64, N <= 64, a workspace), else GENERIC

The expected column was derived from that ladder as the parent commit's launch_value_children wrote it, and then confirmed against
the parent commit's library on an MI355X: one rocprofv3 --kernel-trace run of stand-alone mprl_value_children_f32 calls over ROWS
(random weights; the first kernel name of each call mapped to its family, profiles/children_route.txt).  All 46 traced rows
agree: the family, for the fused rows also the form (the bf16x6 instantiation, or the f32 one behind a pack_images_kernel of the
call's own), and for the refusals the return code.  One refusal differs in what happens before it: on "f16-L2" the parent
launched the deep kernel's f32 form and THEN returned RGL_ERR_BAD_MODE; the route refuses before anything is launched.  Not traced
(UNTRACED): "head-relu" -- a head that ends in a ReLU is not one the Python layer builds; its row follows from `staged` alone.
"""
import collections
import ctypes

import pytest

from relationalgraphlearning_amd import _native as nat
from tests import prologue_embedding as pe

REFUSED, FUSED, RANK1, DEEP, TILE, SCENE, TILES_FORWARD, GENERIC = range(8)      # RGL_CHILDREN_* of include/rgl_hip.h
BAD_MODE = -2
SHIPPED_HEAD = (32, 32, 100, 100, 1)

# a row: the planner (layers, similarity, layerwise, contraction, value head dims, its last_relu, w_r dims, x_dim), the call (P, H,
# workspace at hand) and what the ladder answers (family, refusal, fused_mode, own_image, f16)
Row = collections.namedtuple("Row", "id L sim layerwise contraction head head_relu wr X P H workspace family refusal fused_mode own_image f16")


def _row(id, family, P, H, L=2, sim="embedded_gaussian", layerwise=False, contraction="f32", head=SHIPPED_HEAD, head_relu=False,
         wr=(9, 64, 32), X=32, workspace=True, refusal=0, fused_mode=0, own_image=0, f16=0):
    return Row(id, L, sim, layerwise, contraction, head, head_relu, wr, X, P, H, workspace, family, refusal, fused_mode, own_image, f16)


ROWS = [
    # RGL_FUSED_MIN_TILES: 6 tiles of 16 per parent of 81 children
    _row("f32-1194-tiles", RANK1, 199, 19), _row("f32-1200-tiles", FUSED, 200, 19),
    # N = 32 | 33: the end of the fused and of the rank-1 envelope
    _row("N32-fused", FUSED, 200, 31), _row("N33-past-fused", DEEP, 200, 32),
    _row("N32-rank1", RANK1, 3, 31), _row("N33-past-rank1", DEEP, 3, 32),
    # N = 64 | 65: the end of deep and tile (two layers); three layers: deep's tables end at N = 60, the tile kernel answers to 64
    _row("N64-L2-deep", DEEP, 3, 63), _row("N65-L2-scene", SCENE, 3, 64),
    _row("N60-L3-deep", DEEP, 3, 59, L=3), _row("N61-L3-tile", TILE, 3, 60, L=3),
    _row("N64-L3-tile", TILE, 3, 63, L=3), _row("N65-L3-scene", SCENE, 3, 64, L=3),
    # L = 2 | 3 (and 1: neither shared-crowd kernel)
    _row("L2-small", RANK1, 3, 19), _row("L3-small", DEEP, 3, 19, L=3), _row("L3-large", DEEP, 200, 19, L=3),
    _row("L1", TILE, 3, 19, L=1),
    # similarities: a plain-weight one stays on the shared-crowd kernels; beyond deep's N, the tile kernel is softmax only
    _row("squared-fused", FUSED, 200, 19, sim="squared"), _row("squared-L3", DEEP, 3, 19, L=3, sim="squared"),
    _row("squared-N61-L3", SCENE, 3, 60, L=3, sim="squared"),
    _row("cosine", SCENE, 200, 19, sim="cosine"), _row("cosine-softmax-L3", SCENE, 3, 19, L=3, sim="cosine_softmax"),
    _row("layerwise", SCENE, 200, 19, layerwise=True), _row("layerwise-L3", SCENE, 3, 19, L=3, layerwise=True),
    # f16: the deep kernel's three-layer softmax form or nothing
    _row("f16-L3", DEEP, 3, 19, L=3, contraction="f16", f16=1), _row("f16-L3-large", DEEP, 200, 19, L=3, contraction="f16", f16=1),
    _row("f16-L2", REFUSED, 3, 19, contraction="f16", refusal=BAD_MODE, f16=1),
    _row("f16-L3-squared", REFUSED, 3, 19, L=3, sim="squared", contraction="f16", refusal=BAD_MODE, f16=1),
    _row("f16-L3-N61", REFUSED, 3, 60, L=3, contraction="f16", refusal=BAD_MODE, f16=1),
    # bf16x6: the fused kernel at every size where its form fits a CU (tests/test_bf16x6_kernels.py pins that envelope) ...
    _row("b6-N20", FUSED, 3, 19, contraction="bf16x6", fused_mode=2), _row("b6-N16-squared", FUSED, 3, 15, sim="squared", contraction="bf16x6", fused_mode=2),
    # ... beyond it the f32 form on an image of the call's own -- from the f32 form's threshold up; below it the two-stage pair
    _row("b6-N21-large", FUSED, 200, 20, contraction="bf16x6", own_image=1), _row("b6-N21-small", RANK1, 199, 20, contraction="bf16x6"),
    _row("b6-N20-squared-large", FUSED, 200, 19, sim="squared", contraction="bf16x6", own_image=1),
    _row("b6-N32-large", FUSED, 200, 31, contraction="bf16x6", own_image=1), _row("b6-N33", DEEP, 200, 32, contraction="bf16x6"),
    _row("b6-L3", DEEP, 3, 19, L=3, contraction="bf16x6"),
    # no workspace: never staged, and no tile pipeline either
    _row("no-workspace", GENERIC, 200, 19, workspace=False), _row("no-workspace-L3", GENERIC, 3, 19, L=3, workspace=False),
    _row("no-workspace-f16", REFUSED, 3, 19, L=3, contraction="f16", workspace=False, refusal=BAD_MODE),
    # other value heads: with a stage-2 kernel (path G's head; any other within the ABI's widths) the two-stage pair, never the
    # fused kernel; without one (a ReLU behind the last layer) the call is not staged
    _row("head-150", RANK1, 200, 19, head=(32, 150, 100, 100, 1)), _row("head-64", RANK1, 200, 19, head=(32, 64, 1)),
    _row("head-64-L3", DEEP, 3, 19, L=3, head=(32, 64, 1)),
    _row("head-relu", TILES_FORWARD, 200, 19, head_relu=True),
    # other embedding MLPs: the tile pipeline at x_dim 32 | 64, the general kernel otherwise
    _row("wr-48", TILES_FORWARD, 3, 19, wr=(9, 48, 32)), _row("x-64", TILES_FORWARD, 3, 19, wr=(9, 64, 64), X=64, head=(64, 100, 100, 1)),
    _row("x-48", GENERIC, 3, 19, wr=(9, 64, 48), X=48, head=(48, 100, 100, 1)),
    # a contraction mode the library does not know (2 was the split-f16 mode of ABI 4..7)
    _row("mode-2", REFUSED, 3, 19, contraction=2, refusal=BAD_MODE),
]
UNTRACED = ("head-relu",)


def _mlp(dims, last_relu):
    m = nat.RglMlp()
    m.n_layers, m.last_relu = len(dims) - 1, int(last_relu)
    for i, d in enumerate(dims):
        m.dims[i] = d
    return m


def planner(row):
    """The row's value estimator with dimensions and modes only: the planner exports read no pointer."""
    pl = nat.MprlPlanner()
    g = nat.RglGraph()
    g.w_r, g.w_h = _mlp(row.wr, True), _mlp((5, 64, row.X), True)
    g.x_dim, g.num_layer, g.similarity, g.skip_connection, g.layerwise_graph = row.X, row.L, nat.SIMILARITY[row.sim], 1, int(row.layerwise)
    pl.value_graph, pl.value_head = g, _mlp(row.head, row.head_relu)
    pl.num_actions = 81
    pl.contraction_dtype = row.contraction if isinstance(row.contraction, int) else nat.CONTRACTION_DTYPES[row.contraction]
    return pl


def route(row, image_at_hand=1):
    pl, p = planner(row), nat.RglValueChildrenPlan()
    nat.check(nat.lib().rgl_plan_value_children(ctypes.byref(pl), row.P, row.H, int(row.workspace), image_at_hand, ctypes.byref(p)),
              "rgl_plan_value_children")
    return p


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_route_follows_the_ladder(row):
    p = route(row)
    assert (p.family, p.refusal) == (row.family, row.refusal), (row.id, p.family, p.refusal)
    if row.family == FUSED:
        assert (p.fused_mode, p.own_image) == (row.fused_mode, row.own_image), (row.id, p.fused_mode, p.own_image)
    if row.family == DEEP:
        assert p.f16 == row.f16, row.id
    # the two-stage pair copies its weights from a packed image outside bf16x6 -- if there is one; the family does not depend on it
    if row.family in (RANK1, DEEP, TILE):
        assert p.pair_image == int(row.contraction != "bf16x6"), row.id
    q = route(row, image_at_hand=0)
    assert (q.family, q.refusal, q.fused_mode, q.own_image, q.pair_image) == (p.family, p.refusal, p.fused_mode, p.own_image, 0), row.id


def test_the_table_has_both_sides_of_every_boundary():
    fam = {r.id: r.family for r in ROWS}
    assert {r.family for r in ROWS} == set(range(8))
    for below, above in (("f32-1194-tiles", "f32-1200-tiles"), ("N32-fused", "N33-past-fused"), ("N32-rank1", "N33-past-rank1"),
                         ("N64-L2-deep", "N65-L2-scene"), ("N60-L3-deep", "N61-L3-tile"), ("N64-L3-tile", "N65-L3-scene"),
                         ("L2-small", "L3-small"), ("f16-L3", "f16-L2"), ("b6-N21-small", "b6-N21-large"), ("head-64", "head-relu"),
                         ("wr-48", "x-48"), ("f32-1200-tiles", "no-workspace")):
        assert fam[below] != fam[above], (below, above)
    own = {r.id: (r.family, r.fused_mode, r.own_image) for r in ROWS}      # the bf16x6 form's end is a boundary inside one family
    assert own["b6-N20"] == (FUSED, 2, 0) and own["b6-N21-large"] == (FUSED, 0, 1)


def test_argument_checks():
    lib, ref = nat.lib(), ctypes.byref
    pl, p = planner(ROWS[0]), nat.RglValueChildrenPlan()
    assert lib.rgl_plan_value_children(None, 3, 19, 1, 1, ref(p)) == -3 and lib.rgl_plan_value_children(ref(pl), 3, 19, 1, 1, None) == -3
    assert lib.rgl_plan_value_children(ref(pl), 0, 19, 1, 1, ref(p)) == -1 and lib.rgl_plan_value_children(ref(pl), 3, 0, 1, 1, ref(p)) == -1
    assert "rgl_plan_value_children" in nat.SIGNATURES and "rgl_plan_value_children" in nat.ADDITIVE


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_deep_plan_is_covered_exactly_where_the_route_says_deep(row):
    """rgl_plan_deep_children answers for a call with a full workspace."""
    full = row._replace(workspace=True)
    pl, d = planner(full), nat.RglDeepChildrenPlan()
    nat.check(nat.lib().rgl_plan_deep_children(ctypes.byref(pl), row.P, row.H, 1, ctypes.byref(d)), "rgl_plan_deep_children")
    r = route(full)
    assert bool(d.covered) == (r.family == DEEP), (row.id, d.covered, r.family)
    if d.covered:
        assert d.f16 == r.f16 and d.layers == row.L, row.id


def test_prologue_threshold_and_form():
    """The level prologue takes a level from ceil(P / 256) >= 4 parents per CU (256 CUs without a device: the MI355X's) -- where the
    route gives the call that carries it to the fused kernel's prologue form (bf16x6, 17..20 nodes, softmax similarity)."""
    lib, ref, p = nat.lib(), ctypes.byref, nat.RglPrologueEmbeddingPlan()

    def ask(pl, P, H=19):
        assert lib.rgl_plan_prologue_embedding(ref(pl), P, H, 1, 1, ref(p)) == 0
        return p.prologue

    assert (ask(pe.planner(2, 2), 768), ask(pe.planner(2, 2), 769)) == (0, 1)
    # without the form, on either side: a plain-weight value graph (its bf16x6 form of 17..20 nodes does not fit a CU: the fused
    # kernel still takes the call, as the f32 form -- which has no prologue), f32 contractions, 21 nodes, a head the fused kernel lacks
    for change in ("squared", "f32", "N21", "head"):
        pl = pe.planner(2, 2)
        if change == "squared":
            pl.value_graph.similarity = nat.SIMILARITY["squared"]
        if change == "f32":
            pl.contraction_dtype = nat.CONTRACTION_DTYPES["f32"]
        if change == "head":
            pl.value_head = _mlp((32, 150, 100, 100, 1), False)
        H = 20 if change == "N21" else 19
        assert (ask(pl, 768, H), ask(pl, 769, H), ask(pl, 4096, H)) == (0, 0, 0), change
