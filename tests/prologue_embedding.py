"""Shared by tests/test_prologue_embedding_cpu.py and tests/test_prologue_embedding.py: the searches whose levels take the fused
children kernel's level prologue with the workgroup-cooperative embeddings, the launch plan of each of their levels (asked of the
library: rgl_plan_prologue_embedding, host only) and what each search is in the table for."""
import ctypes

from relationalgraphlearning_amd import _native as nat

CUS = 256                   # MI355X; what the planner assumes without a device
MIN_PARENTS_PER_CU = 4      # the prologue's threshold (kPrologueMinParentsPerCu): ceil(P / CUs) >= 4

# (humans, roots, depth, width, seed) -> what the search exercises
CASES = {
    (19, 800, 1, 2, 21): "about the smallest level above the threshold; short workgroups",
    (16, 1024, 2, 2, 22): "N = 17: one valid node in the second tile; crowds of exactly one tile",
    (17, 1024, 2, 2, 23): "rows straddle tiles and crowds",
    (18, 1001, 2, 2, 24): "rows straddle tiles and crowds; short last workgroups (1 of 4 and 2 of 8 parents)",
    (19, 400, 3, 3, 25): "middle level of 1200 parents: crowds_per 3, workgroups that do not own whole crowds",
    (19, 2048, 3, 2, 26): "8192 parents at the last level: several chunks per workgroup",
    (19, 2048, 2, 2, 27): "the workload's own launch plan",
    (19, 4096, 1, 2, 28): "16 root parents per workgroup, a crowd each: the crowd bound cuts the chunks (12 + 4)",
}


def _mlp(dims, last_relu):
    m = nat.RglMlp()
    m.n_layers, m.last_relu = len(dims) - 1, int(last_relu)
    for i, d in enumerate(dims):
        m.dims[i] = d
    return m


def _graph():
    g = nat.RglGraph()
    g.w_r, g.w_h = _mlp((9, 64, 32), True), _mlp((5, 64, 32), True)
    g.x_dim, g.num_layer, g.similarity, g.skip_connection = 32, 2, nat.SIMILARITY["embedded_gaussian"], 1
    return g


def planner(depth, width):
    """The shipped model's descriptor with dimensions and modes only: the planner export reads no pointer."""
    pl = nat.MprlPlanner()
    pl.value_graph, pl.predictor_graph = _graph(), _graph()
    pl.value_head, pl.motion_head = _mlp((32, 32, 100, 100, 1), False), _mlp((32, 64, 5), False)
    pl.num_actions, pl.planning_depth, pl.planning_width, pl.do_action_clip = 81, depth, width, 1
    pl.contraction_dtype = nat.CONTRACTION_DTYPES["bf16x6"]
    return pl


def levels(case):
    """(level, parents, crowds_per, unit) of the search's levels: level l expands roots width^l parents, the W siblings below the root
    level share their parent's predicted crowd, and the deepest level hands whole roots to workgroups (the back-up chain runs in the
    kernel's tail) while that leaves at least half the CUs a root."""
    H, roots, depth, width, _ = case
    out = []
    for l in range(depth):
        unit = width ** l if (l == depth - 1 and roots >= CUS // 2) else 1
        out.append((l, roots * width ** l, 1 if l == 0 else width, unit))
    return out


def plan(case, level):
    H, roots, depth, width, _ = case
    l, P, cp, unit = levels(case)[level]
    pl, p = planner(depth, width), nat.RglPrologueEmbeddingPlan()
    nat.check(nat.lib().rgl_plan_prologue_embedding(ctypes.byref(pl), P, H, cp, unit, ctypes.byref(p)), "rgl_plan_prologue_embedding")
    d = {name: getattr(p, name) for name, _ in p._fields_}
    d.update(P=P, H=H, crowds_per=cp, unit=unit)
    return d


def chunks(p, first, end):
    """The chunks [c0, c1) a workgroup that owns parents [first, end) walks: at most 16 parents of at most chunk_crowds crowds."""
    out, c0 = [], first
    while c0 < end:
        c1 = min(c0 + 16, (c0 // p["crowds_per"] + p["chunk_crowds"]) * p["crowds_per"], end)
        out.append((c0, c1))
        c0 = c1
    return out
