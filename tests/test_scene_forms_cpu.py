"""CPU half of the scene graph kernel's form tests (-m "not gpu"): the conditions on the run table of tests/scene_forms.py, held
against the library's own planner (rgl_plan_scene_forward: host only) in a fresh process without switches and in one per forced
environment, the planner against a Python restatement of include/rgl_hip.h's description, the float64 reference against the oracle,
and the conditions on the inputs that give the GPU tests their teeth.  Each coverage condition fails when the run that meets it is
taken out of the table."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import rgl_oracle as orc
from relationalgraphlearning_amd import _native as nat
from tests import golden_io as gio
from tests import scene_forms as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_plans = {}


def plans(env):
    """{run id: the planner's answer} of a child process under `env`'s switches (asked once); `default`: no switch at all, and the
    walking runs' scene counts derived by that process's own planner."""
    if env not in _plans:
        code = ("import json\nfrom tests import scene_forms as sf\n"
                "print('PLANS' + json.dumps({r.id: sf.plan(r) for r in sf.RUNS if r.kind != 'beyond'}))\n")
        e = sf.child_environment(sf.SCENE_ENVS[env])
        if env == "default":
            del e[sf.WALK_SCENES]
        res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr[-3000:]
        _plans[env] = json.loads([l for l in res.stdout.splitlines() if l.startswith("PLANS")][0][5:])
    return _plans[env]


def test_every_run_takes_the_instantiation_it_names_and_every_instantiation_has_a_run():
    assert len(sf.INSTANTIATIONS) == 28 == len(set(sf.INSTANTIATIONS)) and sf.VALID in sf.RUN
    got = plans("default")
    assert set(got) == {r.id for r in sf.ANSWERED}          # the child built the same table: its walking counts are this table's
    reached, riding = set(), set()
    for r in sf.ANSWERED:
        p = got[r.id]
        assert p["covered"] == 1 and tuple(p["inst"]) == r.expect == sf.expected(r), (r.id, p, r.expect)
        assert p["bx"] == 0 and p["embed_launch"] == 1 - p["embed_inside"], (r.id, p)
        if r.flavour == "trained":
            reached.add(r.expect[:5])
        if r.expect[5]:
            riding.add(r.expect[:5])
    assert reached == set(sf.INSTANTIATIONS), (sorted(set(sf.INSTANTIATIONS) - reached), sorted(reached - set(sf.INSTANTIATIONS)))
    # the reward work rides (CH) in every instantiation fewer than 3072 scenes reach: all but the unsplit SK 0..2 forms of NT 2 | 4,
    # which ride in the `unsplit` environment (below)
    want = {i for i in sf.INSTANTIATIONS if not (i[0] in (2, 4) and i[1] != 3 and not i[3])}
    assert riding == want and len(want) == 22, (sorted(want - riding), sorted(riding - want))


@pytest.mark.parametrize("env", [e for e in sf.SCENE_ENVS if e != "default"])
def test_the_planner_under_each_forced_environment(env):
    got = plans(env)
    insts = set()
    for r in sf.ANSWERED:
        p = got[r.id]
        assert p["covered"] == 1 and tuple(p["inst"]) == sf.expected(r, env), (env, r.id, p, sf.expected(r, env))
        insts.add(tuple(p["inst"]))
    nt24 = [i for i in insts if i[0] in (2, 4) and i[1] != 3]
    if env == "unsplit":
        assert nt24 and not any(i[3] or i[4] for i in nt24)
        assert {i[:5] for i in insts if i[5]} >= {(nt, k, w, 0, 0) for nt, w in ((2, 8), (4, 4)) for k in range(3)}         # CH on the unsplit forms
    if env == "split":
        assert nt24 and all(i[3] for i in nt24)
    if env == "noembed":
        assert not any(i[4] for i in insts) and {(1, 0, 8, 0, 0), (2, 0, 8, 1, 0), (4, 0, 8, 1, 0)} <= {i[:5] for i in insts}
    if env in ("ride0", "ride1"):
        assert {i[5] for i in (tuple(got[r.id]["inst"]) for r in sf.EXPAND)} == {int(env == "ride1")}
        # the same scene instantiation but for CH wherever the embeddings are not inside (with them inside, ride0 moves them out)
        for r in sf.EXPAND:
            a, b = sf.expected(r, "ride0"), sf.expected(r, "ride1")
            assert a[:4] == b[:4] and (a[4] == b[4] or b[4] == 1), r.id


def test_the_edge_set_of_every_node_tile_count_is_complete():
    for nt, sks in sf.SK_OF_NT.items():
        for sk in sks:
            mine = [r for r in sf.EDGE if r.expect[0] == nt and sf.FAMILY[sf.SHORT[r.sim]] == sk]
            last = {r.H + 1 - 16 * (nt - 1 if nt < 8 else 7) for r in mine}
            assert last == set(sf.RESIDUES) - ({1} if nt == 1 else set()) | ({2} if nt == 1 else set()), (nt, sk, sorted(last))
            assert {r.L for r in mine} == {1, 2, 3, 4} and {r.skip for r in mine} == {True, False}, (nt, sk)
            assert {r.head for r in mine} == {"value", "motion"} and {r.spc for r in mine} == {1, 3}, (nt, sk)
            assert {sf.SHORT[r.sim] for r in mine} == set(sf.FAMILIES[sk]), (nt, sk)
            assert any(r.lw for r in mine), (nt, sk)
            # dealing: fewer scenes than a workgroup's slots (where it has more than one), one more than a multiple of them,
            # scenes_per_crowd 3 with a crowd boundary inside a workgroup and a crowd across two
            slots = {r.id: sf.plan(r)["slots"] for r in mine}
            assert any(r.P < slots[r.id] for r in mine) or nt == 8, (nt, sk)
            assert any(r.P > slots[r.id] and r.P % slots[r.id] == 1 % slots[r.id] for r in mine), (nt, sk)
            for r in mine:
                if r.spc == 3:
                    s = slots[r.id]
                    assert r.P > s and (s == 1 or (s % 3 != 0 or s > 3)), r.id
                    assert any((k * s) % 3 != 0 for k in range(1, -(-r.P // s))) or s == 1, (r.id, "no crowd across two workgroups")
        gaussians = [r for r in sf.ANSWERED if r.expect[0] == nt and r.sim == "gaussian"]
        assert {r.head for r in gaussians} == {"value", "motion"} and {r.L for r in gaussians} >= {1, 4}, nt          # Wa = I; value rows without a motion head
        assert any(r.flavour == "rand" and r.expect[0] == nt for r in sf.RUNS) and any(r.route == "pathg" and r.expect[0] == nt for r in sf.RUNS), nt
        assert any(r.route == "children" and r.expect[0] == nt for r in sf.RUNS) and any(r.route == "expand" and r.expect[0] == nt for r in sf.RUNS), nt
    assert {r.H + 1 for r in sf.RUNS if r.kind == "wide"} == {65, 68, 80, 96, 112}
    assert {sf.SHORT[r.sim] for r in sf.RUNS if r.route == "children"} >= {"co", "cs", "cc"} and any(r.lw for r in sf.RUNS if r.route == "children")


def test_walking_runs_walk_and_the_others_do_not():
    want = {(1, 0, 0), (2, 0, 0), (2, 1, 0), (3, 0, 0), (4, 1, 0), (4, 0, 0), (8, 1, 0)}           # (NT, split, embeddings inside)
    assert {(r.expect[0], r.expect[3], r.expect[4]) for r in sf.WALK} == want
    for r in sf.WALK:
        p = sf.plan(r)
        S = sf.n_scenes(r)
        assert p["grid"] == p["grid_cap"] and p["grid"] * p["slots"] < S <= p["grid"] * p["slots"] + p["slots"] + 3, (r.id, p)
        assert r.H + 1 == {1: 2, 2: 17, 3: 33, 4: 49, 8: 65}[r.expect[0]], r.id
        sample = sf.walk_sample(r, p)
        turn = p["grid"] * p["slots"]
        assert len(sample) >= 32 and 0 in sample and S - 1 in sample and any(s >= turn for s in sample) and any(s < turn for s in sample)
        assert {s % p["slots"] for s in sample} == set(range(p["slots"])), r.id
        spc = sf.scenes_per_crowd(r)
        assert all(sample[i] // spc == sample[i + spc - 1] // spc for i in range(0, len(sample), spc)) and S % spc == 0
        # a launch of the sample alone takes the same instantiation without switches -- or in the `unsplit` environment
        alone = sf.expected(r, "default", len(sample))
        assert alone == r.expect or sf.expected(r, "unsplit", len(sample)) == sf.expected(r, "unsplit") == r.expect, r.id
    assert any(sf.scenes_per_crowd(r) == 3 for r in sf.WALK)
    for r in sf.ANSWERED:
        if r.kind != "walk":
            p = sf.plan(r)
            assert sf.n_scenes(r) <= p["grid"] * p["slots"] and p["grid"] <= p["grid_cap"], (r.id, p)


def restated(N, L, sk, P, path_g=False, motion=False):
    """include/rgl_hip.h's description of rgl_plan_scene_forward restated (no switches, no reward work, no image)."""
    take = lambda n: (n + 3) & ~3
    NT = sf.node_tiles(N)
    below = 3072 if NT == 2 else 4096
    emb = (not path_g) and sk == 0 and NT in (1, 2, 4) and P <= 512 and (NT == 1 or P < below)
    split = NT == 8 or emb and NT != 1 or (sk != 3 and NT in (2, 4) and P < below)
    waves = 8 if split or NT <= 2 else 4
    slots = waves // NT if split else waves
    floats = take(32 * 36) + take(L * 32 * 36) + take(32 * 80) + take(64) + take(64 * 20) + take(16)
    if sk == 3:
        floats += take(64 * 80) + take(64) + take(64)
    if emb:
        floats += 2 * take(3168)
    region = 8 // NT if emb and NT in (2, 4) else (8 if NT <= 2 else (4 if NT <= 4 else 1))
    floats += take(region * 16 * NT * 36)
    lds = 4 * floats
    cap = 256 * (2 if 2 * lds <= 160 * 1024 else 1) * (2 if waves == 4 else 1)
    steps = 4 if sk == 3 else max(0, (N - 16 * (NT - 1) + 3) >> 2)
    return dict(node_tiles=NT, family=sk, waves=waves, split=int(split), embed_inside=int(emb), slots=slots, grid=min(-(-P // slots), cap),
                grid_cap=cap, last_steps=steps, lds_bytes=lds, embed_launch=int(not emb), children_riding=0, bx=0, covered=1)


def test_planner_against_a_restatement_of_the_header():
    seen = set()
    for sk, sim in enumerate(("embedded_gaussian", "squared", "cosine_softmax", "concatenation")):
        for L in (1, 2, 3, 4):
            for path_g in (False, True):
                g = sf.graph_of(sim, L, path_g=path_g)
                for N in list(range(2, 70)) + [79, 80, 81, 96, 111, 112, 113, 116, 117, 120, 124, 125, 127, 128]:
                    for P in (1, 7, 8, 9, 511, 512, 513, 2048, 2049, 3071, 3072, 4095, 4096, 4097, 9000):
                        p = sf.plan_of(g, False, P, 1, N - 1)
                        if sk == 3 and N > 64:
                            assert p["covered"] == 0 and p["inst"] is None and p["lds_bytes"] == 0, (sim, N)
                            continue
                        want = restated(N, L, sk, P, path_g)
                        assert {k: p[k] for k in want} == want, (sim, L, N, P, path_g, p, want)
                        assert p["lds_bytes"] <= 160 * 1024
                        seen.add(p["inst"][:5])
    # every answer over the envelope is one of the 28 the table reaches: an instantiation added to the launcher shows here
    assert seen == set(sf.INSTANTIATIONS), sorted(seen ^ set(sf.INSTANTIATIONS))


def test_the_planner_reports_the_bf16x6_instantiations_and_the_reward_work():
    g = sf.graph_of("embedded_gaussian", 2)
    got = set()
    for P in (5, 600, 3000, 3072, 5000):
        p = sf.plan_of(g, True, P, 1, 19, image=True)
        assert p["bx"] == 1 and p["covered"] == 1, p
        got.add(p["inst"][:5])
    assert got == set(sf.BF16X6_INSTANTIATIONS), got
    for H, sim in ((5, "embedded_gaussian"), (40, "embedded_gaussian"), (19, "squared"), (19, "cosine")):        # the image serves softmax at NT 2 only
        assert sf.plan_of(sf.graph_of(sim, 2), True, 600, 1, H, image=True)["bx"] == 0
    # offered reward work: in this launch below 3072 scenes (1100 in the bf16x6 mode), else in the embedding launch -- never embedded inside
    for P, image, riding in ((3071, False, 1), (3072, False, 0), (1099, True, 1), (1100, True, 0), (100, False, 1)):
        p = sf.plan_of(g, True, P, 1, 19, image=image, reward=True)
        assert p["children_riding"] == riding and (riding or (p["embed_launch"] == 1 and p["embed_inside"] == 0)), (P, image, p)
    assert sf.plan_of(g, True, 100, 1, 19, reward=True)["embed_inside"] == 1


def test_plan_export_checks_its_arguments():
    lib, ref = nat.lib(), ctypes.byref
    g, p = sf.graph_of("embedded_gaussian", 2), nat.RglSceneForwardPlan()
    assert ctypes.sizeof(nat.RglSceneForwardPlan) == 14 * 4 + 8
    assert lib.rgl_plan_scene_forward(None, 0, 3, 1, 5, 0, 0, ref(p)) == -3 and lib.rgl_plan_scene_forward(ref(g), 0, 3, 1, 5, 0, 0, None) == -3
    for S, spc, H in ((0, 1, 5), (3, 0, 5), (3, 1, 0), (4, 3, 5), (3, 1, 128)):
        assert lib.rgl_plan_scene_forward(ref(g), 0, S, spc, H, 0, 0, ref(p)) == -1, (S, spc, H)
    # no pointer of the graph is read: they are NULL here
    assert lib.rgl_plan_scene_forward(ref(g), 0, 3, 1, 127, 0, 0, ref(p)) == 0 and (p.covered, p.node_tiles, p.slots, p.last_steps) == (1, 8, 1, 4)
    for change, why in ((lambda q: setattr(q, "num_layer", 5), "five layers"), (lambda q: setattr(q, "x_dim", 64), "x_dim 64"),
                        (lambda q: setattr(q, "similarity", 99), "an unknown similarity"), (lambda q: setattr(q, "w_r", sf._mlp((9, 64, 64, 32), True)), "a deeper w_r"),
                        (lambda q: setattr(q, "w_h", sf._mlp((7, 64, 32), True)), "w_h of path G beside w_r of path M")):
        q = sf.graph_of("embedded_gaussian", 2)
        change(q)
        assert lib.rgl_plan_scene_forward(ref(q), 0, 3, 1, 5, 0, 0, ref(p)) == 0 and p.covered == 0 and p.grid == 0 and p.lds_bytes == 0, why


@pytest.mark.parametrize("run_id", [r.id for r in sf.EDGE])
def test_the_edge_runs_have_teeth(run_id):
    """A kernel that drops the last human, the first human of the last node tile or the last k-step group of the last tile, or that
    gives a scene its neighbour's crowd, moves at least one output by 10 x the run's regression bound -- for every tooth that applies
    (scene_forms' docstring says which do not, and why)."""
    r = sf.RUN[run_id]
    reg = sf.bounds(r)[1]
    assert reg is not None and sf.REG_F32 <= reg <= sf.TOL / 4
    moved = sf.teeth(r)
    N, sk = r.H + 1, sf.FAMILY[sf.SHORT[r.sim]]
    want = set()
    if r.sim != "diagonal" and r.H >= 2:
        want |= {"last human", "tile human"} | ({"step group"} if sk != 3 and N > 4 else set())
    if r.P > r.spc and not (r.sim == "diagonal" and r.head == "value"):
        want.add("next crowd")
    assert set(moved) == want and want, (run_id, sorted(moved), sorted(want))
    assert not (r.sim == "diagonal" and r.head == "value"), "diagonal runs have the motion head: every row is an output"
    for what, by in moved.items():
        assert by >= 10 * reg, (run_id, what, by, reg)


def test_the_float32_yardstick_is_small():
    """reference32 against reference64 stays below REG_F32 / 8 on every trained run with the value head, so REG_F32 itself is the
    regression bound there; with the motion head (outputs of several metres, five per human) the 8 x yardstick term governs on some
    runs and stays below 1e-5."""
    for r in sf.ANSWERED:
        out = sf.reference64(r.id)
        assert out.dtype == np.float64 and np.isfinite(out).all(), r.id
        if r.flavour != "trained":
            assert sf.bounds(r) == (sf.TOL, None) and sf.yardstick(r) <= sf.TOL / 100, r.id
            continue
        y = sf.yardstick(r)
        assert y <= (sf.REG_F32 / 8 if r.head == "value" else 1.25e-6), (r.id, y)
        assert sf.bounds(r)[1] == max(sf.REG_F32, 8 * y)


@pytest.mark.parametrize("run_id", [sf.VALID, "forward-N65-L2-eg-motion-P2", "expand-N13-L2-cc-motion-P4", "children-N20-L3-cs-value-P2",
                                    "forward-N5-L2-eg-value-P5-rand"])
def test_reference64_is_the_oracle(run_id):
    """reference64 within 1e-6 of gio.oracle_params evaluated through the existing float32 path (relative to max(1, max|want|))."""
    r = sf.RUN[run_id]
    a, humans = sf.inputs(run_id)
    Pm = gio.oracle_params(r.flavour, r.L, similarity=r.sim)
    cfg = sf.config(r)
    H = r.H
    with torch.no_grad():
        if r.route == "children":
            P, A = a.shape[0], a.shape[1]
            want = orc.value_estimator_forward(a.reshape(P * A, 1, 9), humans[:, None].expand(P, A, H, 5).reshape(P * A, H, 5), Pm.ve_graph,
                                               Pm.value_network, cfg).numpy().reshape(P, A)
        else:
            S = a.shape[0]
            hum = humans[:, None].expand(humans.shape[0], S // humans.shape[0], H, 5).reshape(S, H, 5)
            want = (orc.state_predictor_humans(a.reshape(S, 1, 9), hum, Pm.sp_graph, Pm.motion_predictor, cfg) if r.head == "motion" else
                    orc.value_estimator_forward(a.reshape(S, 1, 9), hum, Pm.ve_graph, Pm.value_network, cfg)).numpy()
    assert sf.error(want, sf.reference64(run_id)) <= 2e-6, run_id
    assert np.array_equal(want.astype(np.float64), sf.reference32(run_id))
    with pytest.raises(ValueError):
        sf.reference64(run_id)[0, 0] = 0.0              # shared among the tests: read-only


def test_scenes_have_crowds_of_their_own():
    for r in sf.ANSWERED:
        a, humans = sf.inputs(r.id)
        assert humans.shape[1:] == (r.H, 5) and a.dtype == humans.dtype == torch.float32
        assert humans.shape[0] * (r.spc if r.route == "forward" else 1) == r.P
        assert len({row.tobytes() for row in humans.reshape(humans.shape[0], -1).numpy()}) == humans.shape[0], r.id
