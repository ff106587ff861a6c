"""CPU half of the graph-kernel form tests (-m "not gpu"): the conditions on the case table of tests/graph_forms.py, held against the
library's own planner (rgl_plan_graph_tiles: host only).  Each fails when the run that meets it is taken out of the table."""
import ctypes
import math

import pytest

from relationalgraphlearning_amd import _native as nat
from tests import graph_forms as gf
from tests import row_forms as rf

BACKWARD = [r for r in gf.RUNS if not r.forward_only]
FORWARD = [r for r in gf.RUNS if r.forward_only]
# the two backward builds no shape reaches: at x_dim 64 with three layers a scene of 33 nodes (the fewest of NT = 4) already takes
# more than the 160 KB of a CU (test_the_backward_builds_without_a_run_are_unreachable); their forward builds are reachable
UNREACHABLE_BACKWARD = [("P", 4, 4, 3), ("C", 4, 4, 3)]


def inst(r):
    fam, nt, xt, L = r.inst.split("/")
    return fam, int(nt), int(xt), int(L)


def period(r):
    return rf.DISTINCT if r.H <= 5 else rf.DISTINCT_CROWDED


def short(r):
    return [k for k, v in gf.SIMS.items() if v == r.sim][0]


def multi_scene(r, p):
    """Some workgroup walks three scenes and others two, the tail is uneven, and no workgroup meets the same scene twice."""
    return r.S >= 2 * p["grid"] + 1 and r.S % p["grid"] != 0 and math.gcd(p["grid"], period(r)) == 1 and p["grid"] == p["resident"]


def test_every_run_is_covered_and_takes_the_instantiation_it_names():
    assert len(gf.RUN) == len(gf.RUNS) and gf.VALID in gf.RUN and gf.CAPPED in gf.RUN
    for r in gf.RUNS:
        fam, nt, xt, L = inst(r)
        assert (r.X, r.L) == (16 * xt, L) and r.S % r.spc == 0, r.id
        for backward in ((False,) if r.forward_only else (False, True)):
            p = gf.plan(r, backward)
            assert p["covered"] == 1 and p["inst"] == r.inst, (r.id, backward, p)
            assert (p["node_tiles"], p["feature_tiles"], p["layers"], gf.FAMILIES[p["family"]]) == (nt, xt, L, fam), (r.id, p)
            # a layerwise graph of a constant adjacency is the plain graph; every other layerwise run is family W
            assert p["norm"] == gf.NORM_INDEX[short(r)] and (fam == "W") == (r.lw and p["norm"] <= 1), (r.id, p)
            assert 256 <= p["resident"] <= 1536 and p["resident"] % 256 == 0 and p["grid"] == min(r.S, p["resident"]), (r.id, p)
            assert 0 < p["lds_bytes"] <= 160 * 1024, (r.id, p)
        assert not rf.not_mine(r), (r.id, "a row job of the run has no form")
        if r.multi:
            assert multi_scene(r, gf.plan(r, not r.forward_only)), (r.id, gf.plan(r, not r.forward_only))
            assert r.S > gf.plan(r, False)["grid"], (r.id, "the forward build's workgroups walk several scenes too")


def test_every_instantiation_has_a_multi_scene_backward_run():
    """A backward run launches the forward build too (value and motion routes: the heads read H_L)."""
    reached = {inst(r) for r in BACKWARD if r.multi and r.module in ("value", "motion") and multi_scene(r, gf.plan(r, True))
               and r.S > gf.plan(r, False)["grid"]}
    assert len(gf.COMBINATIONS) == 42
    missing = sorted(set(gf.COMBINATIONS) - reached)
    assert missing == sorted(UNREACHABLE_BACKWARD), missing
    # 2 x 40 instantiations by the backward runs; the forward builds of the other two by forward-only runs: 82 of the 84 compiled
    fwd = {inst(r) for r in FORWARD if multi_scene(r, gf.plan(r, False))}
    assert set(UNREACHABLE_BACKWARD) <= fwd, sorted(fwd)
    for r in BACKWARD:
        if r.multi:                 # S comes from the planner: between about 520 and 3100
            assert 517 <= r.S <= 3100, (r.id, r.S)


def test_the_backward_builds_without_a_run_are_unreachable():
    """graph_kernel<4, 4, 3, true, *>: the planner covers no node count that selects it -- if this fails, the table needs the run."""
    for fam, nt, xt, L in UNREACHABLE_BACKWARD:
        for N in range(33, 65):
            for sim in gf.NORMS[fam]:
                r = gf._g("probe", "value", sim, "%s/%d/%d/%d" % (fam, nt, xt, L), N - 1, 600)
                assert gf.plan(r, True)["covered"] == 0, (fam, N, sim)
        probe = gf._g("probe", "value", gf.NORMS[fam][0], "%s/%d/%d/%d" % (fam, nt, xt, L), 32, 600)
        assert gf.plan(probe, False)["inst"] == probe.inst


def test_normalisations_skip_routes_and_node_counts():
    multi = [r for r in BACKWARD if r.multi]
    for fam in gf.FAMILIES:
        for nt in (1, 2) if fam == "W" else (1, 2, 4):
            have = {short(r) for r in multi if inst(r)[:2] == (fam, nt)}
            assert have == set(gf.NORMS[fam]), (fam, nt, sorted(have))
        for L in (2, 3):
            skips = {r.skip for r in multi if inst(r)[0] == fam and r.L == L}
            assert skips == {True, False}, (fam, L, skips)
    for nt in (1, 2, 4):
        routes = {r.module for r in multi if inst(r)[1] == nt}
        assert routes == {"value", "motion", "rgl"}, (nt, routes)
    # layerwise graphs of constant adjacencies are held to the plain family
    for sim in ("eq", "di"):
        runs = [r for r in BACKWARD if r.lw and short(r) == sim]
        assert runs and all(inst(r)[0] == "P" and gf.plan(r, True)["family"] == 0 for r in runs), sim
    N = {r.H + 1 for r in BACKWARD}
    assert 2 in N and 64 in N and N & {16, 17} and N & {32, 33} and any(n % 4 for n in N), sorted(N)
    assert {16, 17} <= N and {32, 33} <= N, sorted(N)


def test_backward_runs_fit_the_workspace_the_python_layer_provides():
    """The caller's workspace is n_scenes x n_params floats (rgl_graph_backward_workspace_bytes).  Every backward run but CAPPED fits it
    at a cap that leaves the graph kernel its full grid -- the runs of 64 nodes included -- so `grid` above is the grid they launch
    (the row jobs of a run may have to share waves first: the cap is counted with all their slabs)."""
    for r in BACKWARD:
        cap, cap_low = gf.backward_cap(r)
        if r.id == gf.CAPPED:
            continue
        full = gf.plan(r, True)["grid"]
        assert cap is not None and cap_low == 2048 and gf.plan(r, True, cap)["grid"] == full, (r.id, cap, cap_low, full)
    assert any(r.H + 1 == 64 and r.X == 64 for r in BACKWARD) and any(r.H + 1 == 64 and r.X == 32 for r in BACKWARD)


def test_the_capped_run_launches_fewer_workgroups_than_scenes():
    """Few scenes of many nodes: the slabs do not fit beside the feature arrays until backward_tiles has halved its cap below the
    number of scenes, so the graph kernel's workgroups walk several scenes each although S is below `resident`.  The bound that
    counts every row job's slabs and the one that counts none agree on the cap."""
    r = gf.RUN[gf.CAPPED]
    cap, cap_low = gf.backward_cap(r)
    full = gf.plan(r, True)
    assert cap is not None and cap == cap_low and cap < r.S <= full["resident"], (cap, cap_low, r.S, full)
    p = gf.plan(r, True, cap)
    assert p["grid"] == cap and p["resident"] == full["resident"] and full["grid"] == r.S
    assert r.S >= 2 * cap + 1 and r.S % cap != 0 and math.gcd(cap, period(r)) == 1, (r.S, cap)


def test_forward_only_runs():
    """hl_row0 (value head), all rows (motion head), scenes_per_crowd 1 and 3, each with a workgroup walking several scenes; one of each
    at XT = 4 and one at NT = 4."""
    assert all(multi_scene(r, gf.plan(r, False)) for r in FORWARD)
    kinds = lambda runs: {(r.module, r.spc) for r in runs}
    for sel in (lambda r: inst(r)[2] == 4, lambda r: inst(r)[1] == 4):
        got = kinds([r for r in FORWARD if sel(r)])
        assert {m for m, _ in got} == {"value", "motion"} and {s for _, s in got} == {1, 3}, got


def test_refusals_are_outside_the_envelope():
    ids = [e[0] for e in gf.REFUSED]
    assert ids == ["layerwise-cosine", "layerwise-cosine_softmax", "layerwise-x64", "layerwise-33-nodes", "concatenation", "65-nodes",
                   "4-layers"]
    for e in gf.REFUSED:
        r = gf.refused_run(e)
        for backward in (False, True):
            p = gf.plan(r, backward)
            assert p["covered"] == 0 and not any(v for k, v in p.items() if k != "inst") and p["inst"] is None, (e, p)
    # the neighbours inside the envelope are covered
    for sim, lw, X, H, L in (("sq", True, 32, 31, 3), ("eg", False, 32, 63, 2), ("eq", True, 64, 63, 1), ("co", False, 64, 5, 3)):
        r = gf.refused_run(("x", sim, lw, X, H, L, 0))
        assert gf.plan(r, True)["covered"] == 1, (sim, lw, X, H, L)


def test_plan_export_checks_its_arguments():
    lib = nat.lib()
    g, p = nat.RglGraph(), nat.RglGraphTilesPlan()
    g.x_dim, g.num_layer, g.similarity = 32, 2, nat.SIMILARITY["embedded_gaussian"]
    ref = ctypes.byref
    assert lib.rgl_plan_graph_tiles(None, 8, 5, 1, 2048, ref(p)) == -3 and lib.rgl_plan_graph_tiles(ref(g), 8, 5, 1, 2048, None) == -3
    for S, H, mw in ((0, 5, 2048), (8, 0, 2048), (8, 5, 0)):
        assert lib.rgl_plan_graph_tiles(ref(g), S, H, 1, mw, ref(p)) == -1, (S, H, mw)
    # no pointer of the graph is read: they are NULL here
    assert lib.rgl_plan_graph_tiles(ref(g), 5000, 5, 1, 2048, ref(p)) == 0
    assert (p.covered, p.node_tiles, p.feature_tiles, p.layers, p.family, p.norm) == (1, 1, 2, 2, 0, 0)
    assert p.grid == p.resident == 1536 and p.lds_bytes > 0
    assert lib.rgl_plan_graph_tiles(ref(g), 5000, 5, 1, 100, ref(p)) == 0 and (p.grid, p.resident) == (100, 1536)
    assert lib.rgl_plan_graph_tiles(ref(g), 7, 5, 0, 2048, ref(p)) == 0 and (p.grid, p.resident) == (7, 1536)
    g.x_dim = 48
    assert lib.rgl_plan_graph_tiles(ref(g), 7, 5, 0, 2048, ref(p)) == 0 and p.covered == 0 and p.grid == 0
    assert ctypes.sizeof(nat.RglGraphTilesPlan) == 8 * 4 + 8
