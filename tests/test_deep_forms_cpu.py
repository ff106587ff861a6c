"""CPU half of the deep children kernel's form tests (-m "not gpu"): the conditions on the run table of tests/deep_forms.py, held
against the library's own planner (rgl_plan_deep_children: host only), the planner against a Python restatement of plan_deep's LDS
arithmetic, the float64 reference against the oracle, and the conditions on the inputs that give the GPU tests their teeth.  Each
coverage condition fails when the run that meets it is taken out of the table."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import rgl_oracle as orc
from relationalgraphlearning_amd import _native as nat
from tests import deep_forms as df
from tests import golden_io as gio


def plans():
    return {r.id: df.plan(r) for r in df.RUNS}


def test_every_run_takes_the_kernel_it_names_and_every_instantiation_has_a_run():
    assert len(df.RUN) == len(df.RUNS) and df.VALID in df.RUN and df.RUN[df.VALID].expect == "deep"
    assert len(df.INSTANTIATIONS) == 30 == len(set(df.INSTANTIATIONS))
    reached = {}
    for r in df.RUNS:
        # only shapes the fused and the rank-1 kernel cannot take: three layers, or two layers beyond 32 nodes
        assert r.L == 3 or (r.L == 2 and r.H + 1 > 32), r.id
        for image in (True, False):
            p = df.plan(r, image)
            assert p["covered"] == (1 if r.expect == "deep" else 0), (r.id, image, p)
            if not p["covered"]:
                assert not any(v for k, v in p.items() if k != "inst") and p["inst"] is None, (r.id, p)
                continue
            N, A = r.H + 1, df.num_actions(r)
            assert p["inst"][:3] == ((N + 15) // 16, df.family(r), r.skip), (r.id, p)
            assert (p["child_tiles"], p["layers"], p["norm"], p["table_stride"]) == ((A + 15) // 16, r.L, df.NORM[df.short(r)], (N + 3) & ~3), (r.id, p)
            assert p["fuse_head"] == int(image and df.has_image(r)) and 0 < p["lds_bytes"] <= 160 * 1024, (r.id, p)
            assert p["workgroups_per_cu"] == (2 if 2 * p["lds_bytes"] <= 160 * 1024 else 1), (r.id, p)
            # T4: three layers, softmax, f32, NT >= 2, at most four valid nodes in the last node tile
            t4 = r.L == 3 and df.family(r) == "soft" and N > 16 and N - 16 * ((N + 15) // 16 - 1) <= 4
            assert p["inst"][3] == t4, (r.id, p)
            if r.flavour == "trained" and r.contraction != "bf16x6":
                reached.setdefault(p["inst"], []).append(r.id)
    missing = sorted(set(df.INSTANTIATIONS) - set(reached))
    assert not missing and set(reached) == set(df.INSTANTIATIONS), (missing, sorted(set(reached) - set(df.INSTANTIATIONS)))


def test_the_planner_reports_no_instantiation_outside_the_thirty():
    """Every answer of the planner over the kernel's whole envelope is one of the thirty the table reaches: an instantiation added to
    the launcher shows here as a form without a run."""
    seen = set()
    for L in (2, 3):
        for sim in df.SIMS.values():
            for skip in (True, False):
                for mode in ("f32", "f16", "bf16x6"):
                    pl = df.planner(L, sim, skip, 17, mode)
                    for N in range(2, 65):
                        p = df.plan_of(pl, 3, N - 1, mode != "bf16x6")
                        if p["covered"]:
                            seen.add(p["inst"])
    assert seen == set(df.INSTANTIATIONS), sorted(seen ^ set(df.INSTANTIATIONS))


def test_similarities_layers_and_child_tiles_at_every_node_tile_count():
    pl = plans()
    for nt in (1, 2, 3, 4):
        mine = [r for r in df.COVERED if pl[r.id]["node_tiles"] == nt and r.flavour == "trained" and r.contraction != "bf16x6"]
        assert {df.short(r) for r in mine} == set(df.SIMS), (nt, sorted({df.short(r) for r in mine}))
        for fam in ("soft", "plain", "f16"):
            assert {r.skip for r in mine if df.family(r) == fam} == {True, False}, (nt, fam)
        assert {df.short(r) for r in mine if r.contraction == "f16"} == {"eg", "ga"}, nt
        assert any(r.flavour == "rand" and pl[r.id]["node_tiles"] == nt for r in df.COVERED), nt
        assert any(r.dense and pl[r.id]["node_tiles"] == nt for r in df.COVERED), nt
        assert sum(r.kind == "walk" and pl[r.id]["node_tiles"] == nt for r in df.RUNS) == 1, nt
        # 1, 4, 5 and 16 valid nodes in the last node tile, with three layers; with two where two layers reach the kernel
        for L in (3,) if nt < 3 else (2, 3):
            last = {r.H + 1 - 16 * (nt - 1) for r in mine if r.kind == "edge" and r.L == L}
            # (N = 1 has no human: two nodes at NT = 1; the planner's largest N at A = 81 with three layers is 60: twelve nodes)
            assert {2 if nt == 1 else 1, 4, 5, 12 if (nt, L) == (4, 3) else 16} <= last, (nt, L, sorted(last))
    # the crowd waves join the child tiles of phases A and B when CT > 8 - NT: at NT = 3 and NT = 4, and not at NT = 1, 2
    joined = {pl[r.id]["node_tiles"] for r in df.COVERED if pl[r.id]["child_tiles"] > 8 - pl[r.id]["node_tiles"]}
    assert joined == {3, 4}, joined
    assert {pl[r.id]["child_tiles"] for r in df.COVERED} >= {1, 2, 4, 6}
    A = {df.num_actions(r) for r in df.COVERED}
    assert {2, 16, 17, 81, 96} <= A, sorted(A)
    assert all(r.L == 3 for r in df.COVERED if r.contraction == "f16")
    assert {(r.L, pl[r.id]["node_tiles"]) for r in df.COVERED if r.contraction == "bf16x6"} >= {(3, 2), (3, 4), (2, 3)}


def test_both_sides_of_every_lds_limit():
    """The largest N the planner covers per (A, L), from the planner; the table has a run on it and one on the first N beyond."""
    for A, L, n_max in df.LIMITS:
        covered = [N for N in range(2, 67) if df.plan_of(df.planner(L, "embedded_gaussian", True, A, "f32"), 3, N - 1, True)["covered"]]
        assert covered == list(range(2 if L == 3 else 33, n_max + 1)), (A, L, covered)
        inside = [r for r in df.COVERED if (df.num_actions(r), r.L, r.H + 1) == (A, L, n_max) and r.contraction == "f32"]
        beyond = [r for r in df.BEYOND if (df.num_actions(r), r.L, r.H + 1) == (A, L, n_max + 1) and r.expect == "other"]
        assert inside and beyond, (A, L, n_max)
    # f16 has no kernel beyond the limit, nor at two layers: both refusals are in the table
    err = {(r.L, r.H + 1) for r in df.BEYOND if r.expect == "error"}
    assert err == {(3, 61), (2, 40)} and all(r.contraction == "f16" for r in df.BEYOND if r.expect == "error")
    assert df.plan(df.RUN["N60-L3-ga-skip-f16-40x2"])["covered"] == 1


def test_walking_runs_walk():
    assert len(df.WALK) == 4 and sorted(r.P for r in df.WALK) == [257, 300, 300, 300]
    for r in df.WALK:
        fused, unfused = df.plan(r, True), df.plan(r, False)
        assert fused["fuse_head"] == 1 and fused["parents_per_wg"] >= 2 and fused["grid"] == -(-r.P // fused["parents_per_wg"]), (r.id, fused)
        assert unfused["fuse_head"] == 0 and unfused["parents_per_wg"] == 1 and unfused["grid"] < r.P, (r.id, unfused)
        sample = df.walk_sample(r.P)
        k, g = fused["parents_per_wg"], unfused["grid"]
        assert len(sample) >= 32 and r.P - 1 in sample and 0 in sample
        assert any(p % k == 0 for p in sample) and any(p % k == k - 1 for p in sample)          # first and last parent of a workgroup
        assert any(p >= g for p in sample) and g - 1 in sample and g in sample                  # both turns of the stride
        # a smaller table of the list would not walk at this NT: two workgroups per CU, a slot for every parent (NT = 4 walks with any)
        smaller = [a for a in sorted(df.TABLES) if a < df.num_actions(r)]
        if fused["node_tiles"] < 4:
            s, t = df.TABLES[smaller[-1]]
            q = df.plan(r._replace(speeds=s, rots=t), True)
            assert q["parents_per_wg"] == 1 and q["grid"] == r.P, (r.id, smaller[-1], q)
    last = [r for r in df.WALK if r.P == 257][0]
    assert 257 % df.plan(last, True)["parents_per_wg"] == 1              # the last workgroup owns fewer parents


def lds_floats(N, A, L):
    """plan_deep's layout restated: every region rounded up to four floats (W1LD = 80, WLD = XLD = 36, HID = 64, XD = 32)."""
    W1LD, WLD, XLD, HID, XD = 80, 36, 36, 64, 32
    NT, TLD = (N + 15) // 16, (N + 3) & ~3
    take = lambda n: (n + 3) & ~3
    w = take(8 * W1LD) + take(HID) + take(HID * WLD) + take(XD) + take(XD * WLD) + take(12 * W1LD) + take(HID) + take(HID * WLD) + \
        take(XD) + take(XD * WLD) + (take(XD * WLD) if L == 3 else 0)
    crowd = 3 * take(16 * NT * XLD) + 2 * take(16 * NT)
    child = 3 * take(A * XLD) + take(A) + 2 * take(A * TLD) + take(max(A * TLD, NT * NT * 256))
    return w + crowd + child


def test_planner_against_a_restatement_of_the_lds_arithmetic():
    HEAD_LDS = 74176                # HeadLds<32, 100, 100>::total floats x 4: what stage 2 inside the launch needs at least
    for L in (2, 3):
        for A in (2, 16, 17, 81, 96):
            pl = df.planner(L, "embedded_gaussian", True, A, "f32")
            for H in range(1, 64):
                N = H + 1
                want = 4 * lds_floats(N, A, L)
                ok = want <= 160 * 1024 and (L == 3 or N > 32)
                for image in (False, True):
                    p = df.plan_of(pl, 300, H, image)
                    assert p["covered"] == int(ok), (L, A, H, p, want)
                    if not ok:
                        continue
                    lds = max(want, HEAD_LDS) if image else want
                    per_cu = 2 if 2 * lds <= 160 * 1024 else 1
                    k = -(-300 // (256 * per_cu)) if image else 1
                    assert (p["lds_bytes"], p["workgroups_per_cu"], p["parents_per_wg"]) == (lds, per_cu, k), (L, A, H, image, p, want)
                    assert p["grid"] == (-(-300 // k) if image else min(300, 256 * per_cu)), (L, A, H, image, p)
                    assert (p["node_tiles"], p["child_tiles"], p["table_stride"]) == ((N + 15) // 16, (A + 15) // 16, (N + 3) & ~3)


def test_plan_export_checks_its_arguments_and_modes():
    lib, ref = nat.lib(), ctypes.byref
    pl, p = df.planner(3, "embedded_gaussian", True, 81, "f32"), nat.RglDeepChildrenPlan()
    assert ctypes.sizeof(nat.RglDeepChildrenPlan) == 14 * 4 + 8
    assert lib.rgl_plan_deep_children(None, 3, 49, 1, ref(p)) == -3 and lib.rgl_plan_deep_children(ref(pl), 3, 49, 1, None) == -3
    for P, H in ((0, 49), (3, 0)):
        assert lib.rgl_plan_deep_children(ref(pl), P, H, 1, ref(p)) == -1, (P, H)
    # no pointer of the planner is read: they are NULL here
    assert lib.rgl_plan_deep_children(ref(pl), 3, 49, 1, ref(p)) == 0 and (p.covered, p.node_tiles, p.t4, p.fuse_head, p.grid) == (1, 4, 1, 1, 3)
    for change, why in ((lambda q: setattr(q, "num_actions", 97), "97 children"), (lambda q: setattr(q.value_graph, "layerwise_graph", 1), "layerwise"),
                        (lambda q: setattr(q.value_graph, "similarity", nat.SIMILARITY["cosine"]), "cosine"),
                        (lambda q: setattr(q.value_graph, "num_layer", 4), "four layers"), (lambda q: setattr(q.value_graph, "x_dim", 64), "x_dim 64"),
                        (lambda q: setattr(q, "contraction_dtype", 2), "the mode ABI 8 removed")):
        q = df.planner(3, "embedded_gaussian", True, 81, "f32")
        change(q)
        assert lib.rgl_plan_deep_children(ref(q), 3, 49, 1, ref(p)) == 0 and p.covered == 0 and p.grid == 0 and p.lds_bytes == 0, why
    # two layers and at most 32 nodes: the rank-1 (or the fused) kernel's; f16 there and with a plain-weight similarity: refused
    assert df.plan_of(df.planner(2, "embedded_gaussian", True, 81, "f32"), 3, 31, True)["covered"] == 0
    assert df.plan_of(df.planner(2, "embedded_gaussian", True, 81, "f32"), 3, 32, True)["covered"] == 1
    assert df.plan_of(df.planner(2, "embedded_gaussian", True, 81, "f16"), 3, 40, True)["covered"] == 0
    assert df.plan_of(df.planner(3, "squared", True, 81, "f16"), 3, 40, True)["covered"] == 0
    # a head without the shipped widths: stage 2 stays outside the launch
    q = df.planner(3, "embedded_gaussian", True, 81, "f32")
    q.value_head = df._mlp((32, 150, 100, 100, 1), False)
    assert df.plan_of(q, 3, 49, True)["fuse_head"] == 0 and df.plan_of(q, 3, 49, True)["covered"] == 1


def test_bounds_are_the_projects():
    """deep_forms holds the bounds without importing the GPU suite: the same numbers as tests/test_gpu_parity.py's."""
    import re
    src = open(df.__file__.replace("deep_forms.py", "test_gpu_parity.py")).read()
    got = {k: float(re.search(r"^%s = (\S+)" % k, src, flags=re.M).group(1)) for k in ("TOL", "REG_F32", "REG_F16", "F16_TOL")}
    assert got == {"TOL": df.TOL, "REG_F32": df.REG_F32, "REG_F16": df.REG_F16, "F16_TOL": df.F16_TOL}
    assert re.search(r"def seeded_scenes\(seed, B, H\):\n(.*?)\n\n\n", src, flags=re.S).group(1) == \
        re.search(r"def seeded_scenes\(seed, B, H\):\n    \"\"\".*?\"\"\"\n(.*?)\n\n\n", open(df.__file__).read(), flags=re.S).group(1)


@pytest.mark.parametrize("run_id", ["N50-L3-ga-noskip-f32-1x1", "N21-L3-eg-skip-f32-40x2", "N64-L2-ga-skip-f32-40x2", "N37-L3-di-skip-f32-40x2",
                                    "N5-L3-eg-skip-f32-40x2-rand"])
def test_reference64_is_the_oracle(run_id):
    """reference64 within 1e-6 of gio.oracle_params evaluated through the existing float32 path (relative to max(1, max|want|))."""
    r = df.RUN[run_id]
    cr, humans = df.inputs(run_id)
    P, A, H = cr.shape[0], cr.shape[1], r.H
    Pm = gio.oracle_params(r.flavour, r.L, similarity=r.sim)
    with torch.no_grad():
        want = orc.value_estimator_forward(cr.reshape(P * A, 1, 9), humans[:, None].expand(P, A, H, 5).reshape(P * A, H, 5), Pm.ve_graph,
                                           Pm.value_network, orc.OracleConfig(num_layer=r.L, similarity=r.sim, skip_connection=r.skip))
    want = want.numpy().reshape(P, A)
    assert df.reference64(run_id).dtype == np.float64 and df.reference64(run_id).shape == (r.P, df.num_actions(r))
    assert df.error(want, df.reference64(run_id)) <= 1e-6, run_id
    assert np.array_equal(want.astype(np.float64), df.reference32(run_id))
    with pytest.raises(ValueError):
        df.reference64(run_id)[0, 0] = 0.0              # shared among the tests: read-only


@pytest.mark.parametrize("run_id", [r.id for r in df.EDGE])
def test_the_edge_runs_have_teeth(run_id):
    """A kernel that drops the last human, the first human of the last node tile, or gives the last child its neighbour's robot state
    moves at least one value by 10 x the run's regression bound.  `diagonal` (A = I) never reads a human on the robot's row: a
    kernel that drops a node is right there, and only the child condition applies."""
    r = df.RUN[run_id]
    reg = df.bounds(r)[1]
    assert reg is not None and reg >= (df.REG_F16 if r.contraction == "f16" else df.REG_F32)
    moved = df.teeth(r)
    if r.sim == "diagonal":
        assert moved["last human"] == 0.0 and moved["tile human"] == 0.0
        moved = {"last child": moved["last child"]}
    for what, by in moved.items():
        assert by >= 10 * reg, (run_id, what, by, reg)


def test_f16_rounding_leaves_room_under_the_f16_bound():
    """What rounding layer 1's operands to f16 costs on each f16 run's inputs (reference_f16 against reference64, both float64 on the
    CPU) stays below REG_F16 by an f32 form's bound, so that the kernel can be asked for REG_F16 there; and the restatement without
    any rounding is reference64."""
    runs = [r for r in df.COVERED if r.contraction == "f16"]
    assert len(runs) >= 20
    for r in runs:
        cost = df.error(df.reference_f16(r.id), df.reference64(r.id))
        assert 1e-7 < cost <= df.REG_F16 - max(df.REG_F32, 8 * df.yardstick(r)), (r.id, cost)
    half = torch.Tensor.half
    try:
        torch.Tensor.half = lambda t: t
        df.reference_f16.cache_clear()
        for r in runs[:6]:
            assert df.error(df.reference_f16(r.id), df.reference64(r.id)) <= 1e-12, r.id
    finally:
        torch.Tensor.half = half
        df.reference_f16.cache_clear()


def test_parents_have_crowds_of_their_own_and_the_float32_yardstick_is_small():
    for r in df.COVERED:
        cr, humans = df.inputs(r.id)
        assert cr.shape == (r.P, df.num_actions(r), 9) and humans.shape == (r.P, r.H, 5) and cr.dtype == humans.dtype == torch.float32
        flat = humans.reshape(r.P, -1).numpy()
        assert len({row.tobytes() for row in flat}) == r.P, r.id
        tol, reg = df.bounds(r)
        if reg is not None and r.contraction != "f16":
            # the float32 oracle's own deviation: what the regression bound is a multiple of; far below the north-star bound
            assert df.REG_F32 <= reg <= tol / 4, (r.id, reg)
