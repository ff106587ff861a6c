"""CPU half of the two-stage pair's form tests (-m "not gpu"): the conditions on the run table of tests/two_stage_forms.py, held
against the library's own planner (rgl_plan_two_stage_children: host only) as a process of each environment answers it, the
float64 reference against the oracle, and the conditions on the inputs that give the GPU tests their teeth.  Each coverage
condition fails when the run that meets it is taken out of the table."""
import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import rgl_oracle as orc
from relationalgraphlearning_amd import _native as nat
from tests import deep_forms as df
from tests import two_stage_forms as ts

RANK1 = 2               # RGL_CHILDREN_RANK1 of include/rgl_hip.h


def test_the_pair_takes_a_run_exactly_where_the_table_says_in_each_environment():
    assert len(ts.RUN) == len(ts.RUNS) and ts.VALID in ts.RUN and ts.RUN[ts.VALID].kind == "edge"
    hdr = open(ts.ROOT + "/include/rgl_hip.h").read()
    assert int(re.search(r"#define RGL_CHILDREN_RANK1 (\d+)", hdr).group(1)) == RANK1
    for env in ts.ENVS:
        plans = ts.plans_under(env)
        for r in ts.RUNS:
            p, want = plans[r.id], ts.expects_pair(r, env)
            assert (p["family"] == RANK1) == want and p["pair"] == int(want), (env, r.id, p)
            if not want:
                assert not any(p[k] for k in ts.PLAN_FIELDS) and p["inst"] is None, (env, r.id, p)
                continue
            N, A = r.H + 1, ts.num_actions(r)
            hr, nt = [k for k, (lo, hi) in ts.BUCKETS.items() if lo <= N <= hi][0]
            assert p["inst"] == (hr, nt, r.skip, ts.NORM[ts.short(r)] == 0), (env, r.id, p)
            assert (p["child_tiles"], p["norm"], p["sld"]) == ((A + 15) // 16, ts.NORM[ts.short(r)], 16 * nt + 1), (env, r.id, p)
            # the packed image: the shipped head's f32 calls have one; bf16x6 and every other head copy matrix by matrix
            assert p["image"] == p["image_at_hand"] * int(r.contraction == "f32") == int(r.head == "ship" and r.contraction == "f32"), (env, r.id, p)
            assert p["grid"] == min(r.P, 256) and p["parents_per_wg"] == -(-r.P // 256) and 0 < p["lds_bytes"] <= 160 * 1024, (env, r.id, p)
            assert p["head_variant"] == ts.VARIANT[r.head] and p["head_tiles"] == -(-r.P * A // 16), (env, r.id, p)
            waves, cap = ((8, 512), (8, 256), (4, 256))[p["head_variant"]]
            assert p["head_grid"] == min(-(-p["head_tiles"] // waves), cap), (env, r.id, p)
            assert p["head_tiles_per_wave"] == -(-p["head_tiles"] // (waves * p["head_grid"])), (env, r.id, p)
            assert p["head_lds_bytes"] == (74176, 148416, 131072)[p["head_variant"]], (env, r.id, p)


def reached(envs=ts.PAIR_ENVS, runs=None):
    """{environment: [(run, plan)]} of the runs the pair takes."""
    runs = ts.RUNS if runs is None else runs
    return {env: [(r, ts.plans_under(env)[r.id]) for r in runs if ts.plans_under(env)[r.id]["pair"]] for env in envs}


def test_every_instantiation_and_every_head_variant_has_a_run(runs=None):
    """... in the default environment alone (the twostage environment adds the shipped head's large launches), at both ends of its
    (HR, NT): a form that loses its last run fails here."""
    assert len(ts.INSTANTIATIONS) == 16 == len(set(ts.INSTANTIATIONS))
    mine = reached(("default",), runs)["default"]
    trained = [(r, p) for r, p in mine if r.flavour == "trained" and not r.dense]
    by_inst = {}
    for r, p in trained:
        by_inst.setdefault(p["inst"], set()).add(r.H + 1)
    assert set(by_inst) == set(ts.INSTANTIATIONS), sorted(set(ts.INSTANTIATIONS) ^ set(by_inst))
    for (hr, nt, skip, soft), ns in by_inst.items():
        assert set(ts.BUCKETS[(hr, nt)]) <= ns, ((hr, nt, skip, soft), sorted(ns))
    for hr, nt in ts.BUCKETS:
        sims = {ts.short(r) for r, p in trained if p["inst"][:2] == (hr, nt) and r.kind == "edge"}
        assert sims == set(ts.SIMS), ((hr, nt), sorted(sims))                       # gaussian and every plain-weight normalisation
        assert any(r.flavour == "rand" and p["inst"][:2] == (hr, nt) for r, p in mine), (hr, nt)
        assert any(r.dense and p["inst"][:2] == (hr, nt) for r, p in mine), (hr, nt)
    # both sources of the weights, one of the image-less runs with gaussian (Wa = I built in the kernel) and one in the bf16x6 mode
    assert {p["image"] for r, p in trained} == {0, 1}
    assert any(r.sim == "gaussian" and r.contraction == "bf16x6" and not p["image"] for r, p in trained)
    assert {r.H + 1 for r, p in trained if r.contraction == "bf16x6" and r.head == "ship"} >= {21, 32}
    # every CT, and CT + NT from 2 to 8 of the 8 waves; the action tables of the list
    assert {p["child_tiles"] for r, p in trained} == {1, 2, 3, 4, 5, 6}
    assert {p["child_tiles"] + p["node_tiles"] for r, p in trained} == {2, 3, 4, 5, 6, 7, 8}
    for nt in (1, 2):
        assert {p["child_tiles"] for r, p in trained if p["node_tiles"] == nt} == {1, 2, 3, 4, 5, 6}, nt
    assert {ts.num_actions(r) for r, p in trained} >= {2, 16, 17, 33, 49, 65, 81, 96}
    # every head variant with a wave walking one tile and at least two; a last tile of one valid row and a full one
    for v in (0, 1, 2):
        env = "twostage" if v == 0 else "default"                   # (the shipped head's 4096 tiles are the fused kernel's by default)
        heads = [(r, p) for r, p in reached((env,), runs)[env] if p["head_variant"] == v]
        assert {min(p["head_tiles_per_wave"], 2) for r, p in heads} == {1, 2}, v
        assert {(r.P * ts.num_actions(r)) % 16 for r, p in heads} >= {0, 1}, v
    assert {r.head for r, p in mine if p["head_variant"] == 2} == {"h64", "h7x130"}


def test_the_instantiation_check_bites():
    """Without its only runs the check above fails: the (20, 2) plain-weight form without skip connections at 17 nodes."""
    runs = [r for r in ts.RUNS if not (r.H + 1 == 17 and not r.skip and ts.NORM[ts.short(r)] != 0)]
    assert len(runs) < len(ts.RUNS)
    with pytest.raises(AssertionError):
        test_every_instantiation_and_every_head_variant_has_a_run(runs)
    runs = [r for r in ts.RUNS if r.kind != "stride" or r.head != "h150"]
    with pytest.raises(AssertionError):
        test_every_instantiation_and_every_head_variant_has_a_run(runs)


def test_the_planner_reports_no_instantiation_outside_the_sixteen():
    """Every answer of the planner over the kernel's whole envelope is one of the sixteen the table reaches, in the bucket of its N."""
    seen = set()
    for sim in ts.SIMS:
        for skip in (True, False):
            for N in range(2, 40):
                p = ts.plan(ts._r(N, sim, skip, A=17), with_image=True)
                if N > 32:
                    assert not p["pair"], (sim, skip, N)
                elif p["pair"]:
                    assert ts.BUCKETS[p["inst"][:2]][0] <= N <= ts.BUCKETS[p["inst"][:2]][1], (N, p)
                    seen.add(p["inst"])
    if not any(k in ts.os.environ for k in ts.STRIPPED):            # (this process's own switches: the default environment)
        assert seen == set(ts.INSTANTIATIONS), sorted(seen ^ set(ts.INSTANTIATIONS))


def test_walking_and_striding_runs_walk_and_stride():
    """One walking run per (HR, NT) with the shipped head in the default environment, both skip settings, a softmax and a plain-weight
    similarity, two and three parents per workgroup; the 81-children runs; the striding runs sit just past the library's own turn."""
    default, two = ts.plans_under("default"), ts.plans_under("twostage")
    assert sorted({r.P for r in ts.WALK}) == [257, 300, 520]
    small = [r for r in ts.WALK if r.head == "ship" and default[r.id]["pair"]]
    assert sorted(default[r.id]["inst"][:2] for r in small) == sorted(ts.BUCKETS) and all(ts.num_actions(r) == 17 for r in small)
    assert {r.skip for r in small} == {True, False} and {ts.NORM[ts.short(r)] == 0 for r in small} == {True, False}
    assert {default[r.id]["parents_per_wg"] for r in small} == {2, 3}
    assert {default[r.id]["parents_per_wg"] for r in small if default[r.id]["node_tiles"] == 2} >= {3}        # the epoch flags, three times
    big = [r for r in ts.WALK if ts.num_actions(r) == 81]
    assert {r.head for r in big} == {"ship", "h150"}
    for r in big:
        assert two[r.id]["pair"] and two[r.id]["parents_per_wg"] >= 2 and two[r.id]["child_tiles"] == 6, r.id
        assert default[r.id]["pair"] == int(r.head != "ship"), r.id
    for r in ts.WALK:
        assert two[r.id]["grid"] == 256 and two[r.id]["head_tiles_per_wave"] == 1, r.id
        sample = ts.walk_sample(r.P)
        assert {0, 255, 256, r.P - 1} <= set(sample) and (r.P < 512 or {511, 512} <= set(sample)) and len(sample) >= 24, r.id
    # walking depths 1, 2 and 3 over the table
    assert {p["parents_per_wg"] for r, p in reached(("twostage",))["twostage"]} >= {1, 2, 3}
    assert sorted(r.head for r in ts.STRIDE) == sorted(ts.HEADS) and all(r.H == 1 for r in ts.STRIDE)
    for r in ts.STRIDE:
        env = "twostage" if r.head == "ship" else "default"
        at, before = ts.plans_under(env)[r.id], ts.plans_under(env)[r.id + "/before"]
        assert at["pair"] and before["pair"] and at["head_tiles_per_wave"] == 2 and before["head_tiles_per_wave"] == 1, (r.id, at, before)
        assert at["head_tiles"] > at["head_grid"] * (4 if at["head_variant"] == 2 else 8) >= before["head_tiles"], (r.id, at, before)
        assert r.P * ts.num_actions(r) <= 66000 and {0, r.P - 1} <= set(ts.walk_sample(r.P)), r.id
    assert max(r.P * ts.num_actions(r) for r in ts.RUNS) == 810 * 81 and max(r.P for r in ts.WALK) == 520


def test_heads_without_an_image_are_the_librarys_answer():
    """mprl_children_image_bytes: an image for the shipped head only (f32: whatever the graph), none for the others."""
    for r in ts.RUNS:
        if r.contraction == "f32":
            assert ts.has_image(r) == (r.head == "ship"), r.id
        if r.head != "ship":
            assert not ts.has_image(r), r.id
    for name, dims in ts.HEADS.items():
        sd = ts.head_sd(name) if name != "ship" else None
        if sd:
            assert [tuple(sd["%d.weight" % (2 * i)].shape) for i in range(len(dims))] == list(zip(dims, (32,) + dims[:-1]))


def test_plan_export_checks_its_arguments_and_modes():
    lib, ref = nat.lib(), ctypes.byref
    run = ts.RUN[ts.VALID]
    pl, p = ts.planner(run), nat.RglTwoStageChildrenPlan()
    assert ctypes.sizeof(nat.RglTwoStageChildrenPlan) == 14 * 4 + 2 * 8
    assert lib.rgl_plan_two_stage_children(None, 3, 20, 1, ref(p)) == -3 and lib.rgl_plan_two_stage_children(ref(pl), 3, 20, 1, None) == -3
    for P, H in ((0, 20), (3, 0), (-1, 20)):
        assert lib.rgl_plan_two_stage_children(ref(pl), P, H, 1, ref(p)) == -1, (P, H)
    if any(k in ts.os.environ for k in ts.STRIPPED):
        return                                                      # (the rest describes the default environment)
    # no pointer of the planner is read: they are NULL here
    assert lib.rgl_plan_two_stage_children(ref(pl), 3, 20, 1, ref(p)) == 0
    assert (p.pair, p.hr, p.node_tiles, p.child_tiles, p.image, p.grid, p.head_variant, p.head_grid) == (1, 32, 2, 6, 1, 3, 0, 2)
    assert lib.rgl_plan_two_stage_children(ref(pl), 3, 20, 0, ref(p)) == 0 and (p.pair, p.image) == (1, 0)
    # from 1200 child tiles the fused kernel takes the shipped head's calls: 200 x 6 tiles, and 199 x 6 below
    assert lib.rgl_plan_two_stage_children(ref(pl), 200, 20, 1, ref(p)) == 0 and p.pair == 0 and p.grid == 0 and p.head_lds_bytes == 0
    assert lib.rgl_plan_two_stage_children(ref(pl), 199, 20, 1, ref(p)) == 0 and (p.pair, p.grid, p.parents_per_wg) == (1, 199, 1)
    for change, why in ((lambda q: setattr(q, "num_actions", 97), "97 children"), (lambda q: setattr(q.value_graph, "layerwise_graph", 1), "layerwise"),
                        (lambda q: setattr(q.value_graph, "similarity", nat.SIMILARITY["cosine"]), "cosine"),
                        (lambda q: setattr(q.value_graph, "num_layer", 3), "three layers"), (lambda q: setattr(q.value_graph, "x_dim", 64), "x_dim 64"),
                        (lambda q: setattr(q, "contraction_dtype", 1), "f16"), (lambda q: setattr(q, "contraction_dtype", 2), "the mode ABI 8 removed"),
                        (lambda q: setattr(q.value_head, "last_relu", 1), "a head without a stage-2 kernel")):
        q = ts.planner(run)
        change(q)
        assert lib.rgl_plan_two_stage_children(ref(q), 3, 20, 1, ref(p)) == 0 and p.pair == 0 and p.grid == 0 and p.lds_bytes == 0, why
    assert lib.rgl_plan_two_stage_children(ref(pl), 3, 32, 1, ref(p)) == 0 and p.pair == 0             # 33 nodes


def test_bounds_are_the_projects():
    """two_stage_forms takes the bounds from deep_forms, which test_deep_forms_cpu holds to tests/test_gpu_parity.py's: held again."""
    src = open(ts.ROOT + "/tests/test_gpu_parity.py").read()
    got = {k: float(re.search(r"^%s = (\S+)" % k, src, flags=re.M).group(1)) for k in ("TOL", "REG_F32")}
    assert got == {"TOL": ts.TOL, "REG_F32": ts.REG_F32} == {"TOL": 1e-4, "REG_F32": 1e-6}
    # the threshold is the default of the library's switch table (csrc/rgl_switches.hip): what an unset RGL_FUSED_MIN_TILES parses to
    lib, unset = nat.lib(), ctypes.c_int(-1)
    row = [i for i in range(64) if lib.rgl_switch_name(i) == b"RGL_FUSED_MIN_TILES"]
    assert len(row) == 1 and lib.rgl_switch_parse(row[0], None, ctypes.byref(unset)) == 0
    assert ts.FUSED_MIN_TILES == 1200 == unset.value and "fused_min_tiles()" in open(ts.ROOT + "/relationalgraphlearning_amd/csrc/rgl_fused.hip").read()
    assert set(df.TABLES.items()) <= set(ts.TABLES.items())


@pytest.mark.parametrize("run_id", ["N2-di-noskip-f32-40x2", "N20-ga-skip-f32-40x2", "N18-eq-skip-f32-40x2-h7x130", "N5-eg-skip-f32-40x2-rand",
                                    "N10-eg-skip-f32-40x2-layerwise"])
def test_reference64_is_the_oracle(run_id):
    """reference64 within 1e-6 of the oracle's existing float32 path on the same checkpoint (relative to max(1, max|want|))."""
    r = ts.RUN[run_id]
    cr, humans = ts.inputs(run_id)
    P, A, H = cr.shape[0], cr.shape[1], r.H
    Pm = orc.MprlParams.from_checkpoint(ts.checkpoint(r))
    with torch.no_grad():
        want = orc.value_estimator_forward(cr.reshape(P * A, 1, 9), humans[:, None].expand(P, A, H, 5).reshape(P * A, H, 5), Pm.ve_graph,
                                           Pm.value_network, orc.OracleConfig(num_layer=r.L, similarity=r.sim, skip_connection=r.skip,
                                                                              layerwise_graph=r.layerwise))
    want = want.numpy().reshape(P, A)
    assert ts.reference64(run_id).dtype == np.float64 and ts.reference64(run_id).shape == (r.P, ts.num_actions(r))
    assert ts.error(want, ts.reference64(run_id)) <= 1e-6, run_id
    assert np.array_equal(want.astype(np.float64), ts.reference32(run_id))
    with pytest.raises(ValueError):
        ts.reference64(run_id)[0, 0] = 0.0              # shared among the tests: read-only


@pytest.mark.parametrize("run_id", [r.id for r in ts.EDGE])
def test_the_edge_runs_have_teeth(run_id):
    """A kernel that drops the last human, the first human of the last node tile, or gives the last child its neighbour's robot state
    moves at least one value by 10 x the run's regression bound (`diagonal`: the child condition only, see two_stage_forms.needed)."""
    r = ts.RUN[run_id]
    reg = ts.bounds(r)[1]
    assert reg is not None and reg >= ts.REG_F32
    for what, by in ts.needed(r, ts.teeth(r)).items():
        assert by >= 10 * reg, (run_id, what, by, reg)


def test_parents_have_crowds_of_their_own_and_the_float32_yardstick_is_small():
    for r in ts.COVERED:
        cr, humans = ts.inputs(r.id)
        assert cr.shape == (r.P, ts.num_actions(r), 9) and humans.shape == (r.P, r.H, 5) and cr.dtype == humans.dtype == torch.float32
        flat = humans.reshape(r.P, -1).numpy()
        assert len({row.tobytes() for row in flat}) == r.P, r.id
        tol, reg = ts.bounds(r)
        if reg is not None:
            assert ts.REG_F32 <= reg <= tol / 4, (r.id, reg)
