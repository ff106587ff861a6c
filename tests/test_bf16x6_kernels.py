"""The six-term bf16 kernels (RGL_CONTRACT_BF16X6) against float64, in every form they launch.

bench.py reports the two-layer workloads with N <= 32 in this mode, and whole-search values hide kernel errors behind selections
and maxima: here each kernel form is held directly against a float64 evaluation of the same operation on the same inputs.

Every bf16x6 comparison asserts (a) the f32 kernels' bounds against the float64 reference (`close(got, want64, reg=REG_F32)`; the
north-star bound alone for the raw random-init weights, as the f32 kernels are held there), (b) err_bx <= 1.5 err_f32 + 2^-23
max(1, max|want64|) -- err_f32 the f32 mode's deviation from float64 on the same inputs in the same launch form, plus one f32 rounding
at the scale `close` measures against -- and (c) the bf16x6 output is not bit-identical to the f32 one (the mode ran).  Outside a
kernel's bf16x6 window the two modes must agree bit for bit.  Switches read once per process (`static`) are set in child processes,
one after another: a child evaluates the kernels in both modes and hands its outputs back as a file; the float64 references and
every assertion stay in this process.

A: the state predictor's scene kernel and the level's reward step (TreeSearch.expand -> expand_level), and path G's value rows.
B: the fused children kernel under every dealing plan (RGL_FUSED_G, RGL_FUSED_INLINE_PARTIAL).
C: the strong-scaling slices of the 8-GPU shares; the share rows and forced families live in tests/test_gpu_parity.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import relationalgraphlearning_amd as rga
from oracle import rgl_oracle as orc
from tests import golden_io as gio
from tests.helpers import make_mprl_policy, make_gcn_policy, dense_scenes
from tests.test_gpu_parity import (TOL, REG_F32, close, report, seeded_scenes, check_decisions, compare_trees, _oracle_at_size,
                                   _bench_policy)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -23
MODES = ("f32", "bf16x6")
# RGL_CONTRACT_F32_AS=bf16x6 turns every f32 search into the bf16x6 one (admission runs of the whole suite): (c) cannot hold there
F32_IS_F32 = not os.environ.get("RGL_CONTRACT_F32_AS")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def params64(flavour, L, similarity="embedded_gaussian", ck=None):
    ck = gio.checkpoint(flavour, L, "separate", similarity) if ck is None else ck
    return orc.MprlParams.from_checkpoint({k: {kk: vv.double() for kk, vv in v.items()} for k, v in ck.items()})


class Worst(object):
    """Worst deviation from float64 per mode over a part (relative to max(1, max|want|), as `close` measures it)."""

    def __init__(self):
        self.bx, self.f32, self.n, self.rms = 0.0, 0.0, 0, 0.0

    def line(self):
        return ("worst deviation from float64 over %d comparisons: bf16x6 %.2e, f32 %.2e" % (self.n, self.bx, self.f32) +
                (" (largest rms ratio bf16x6 / f32 %.2f)" % self.rms if self.rms else ""))


def admit(tag, got_bx, got_32, want64, worst, reg=REG_F32):
    """(a), (b), (c) of the module docstring for one output of one launch form.  `reg` = None for the raw random-init weights
    (hidden features of 10..100): the f32 kernels are held to the north-star bound only there (test_gpu_parity), and (b) ties
    the mode to their deviation on the same inputs."""
    got_bx = np.asarray(got_bx, np.float64)
    got_32 = np.asarray(got_32, np.float64)
    want64 = np.asarray(want64, np.float64)
    scale = max(1.0, float(np.abs(want64).max()))          # the scale `close` measures against
    e6 = float(np.abs(got_bx - want64).max())
    e32 = float(np.abs(got_32 - want64).max())
    assert e6 <= close(got_bx, want64, reg=reg), tag                                                        # (a)
    assert e6 <= 1.5 * e32 + EPS32 * scale, (tag, "bf16x6 vs float64", e6, "f32 vs float64", e32)          # (b)
    if want64.size >= 256:          # (b) on the rms as well, where there are enough values for it to be stable: a lost low-order term
        r6 = float(np.sqrt(np.mean((got_bx - want64) ** 2)))                   # moves every value a little, the maximum hardly
        r32 = float(np.sqrt(np.mean((got_32 - want64) ** 2)))
        assert r6 <= 1.25 * r32 + 1e-9 * scale, (tag, "rms: bf16x6 vs float64", r6, "f32 vs float64", r32)
        worst.rms = max(worst.rms, r6 / max(r32, 1e-30))
    if F32_IS_F32:
        assert not np.array_equal(got_bx, got_32), (tag, "bit-identical to the f32 kernels: the bf16x6 form did not run")   # (c)
    worst.bx, worst.f32, worst.n = max(worst.bx, e6 / scale), max(worst.f32, e32 / scale), worst.n + 1
    return e6, e32


def run_child(kind, cases, env_add, tmp_path, tag, timeout=600):
    """`kind`'s cases evaluated in both modes in a child process under `env_add`; returns the outputs it saved."""
    spec, out = str(tmp_path / ("%s.json" % tag)), str(tmp_path / ("%s.npz" % tag))
    with open(spec, "w") as f:
        json.dump({"kind": kind, "cases": cases}, f)
    code = "import sys\nfrom tests.test_bf16x6_kernels import child_main\nchild_main(sys.argv[1], sys.argv[2])\n"
    env = dict(os.environ, **env_add)
    res = subprocess.run([sys.executable, "-c", code, spec, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0 and "OK" in res.stdout, (env_add, res.stdout[-2000:] + res.stderr[-3000:])
    return dict(np.load(out))


def child_main(spec, out):
    """Entry point of the child processes (see run_child)."""
    with open(spec) as f:
        s = json.load(f)
    dev = torch.device("cuda:0")
    fn = {"expand": expand_outputs, "children": children_outputs}[s["kind"]]
    res = {}
    for i, c in enumerate(s["cases"]):
        for k, v in fn(c, dev).items():
            res["%d/%s" % (i, k)] = v
    np.savez(out, **res)
    print("OK")


# ---------------------------------------------------------------------------------------------------
# A: the state predictor's scene kernel and the reward step, through TreeSearch.expand; path G's value rows
# ---------------------------------------------------------------------------------------------------
def expand_inputs(c):
    if c.get("dense"):
        return dense_scenes(np.random.RandomState(c["seed"]), c["P"], c["H"])
    return seeded_scenes(c["seed"], c["P"], c["H"])


def expand_outputs(c, dev):
    """TreeSearch.expand in both modes (and, with c["reward"], estimate_reward on its own) -> {"<mode>/<output>": array}."""
    robot, humans = expand_inputs(c)
    r, h = robot.to(dev), humans.to(dev)
    joint = bool(c.get("joint", True))
    out = {}
    for mode in MODES:
        pol = make_mprl_policy(c["flavour"], 1, L=c["L"], skip=c["skip"], device=dev)
        pol.contraction_dtype = mode
        pol.build_action_space(1.0)
        ts = pol.tree_search()
        ex = ts.expand(r, h, parents_are_joint_states=joint)
        for k in ("humans_next", "child_robot", "reward", "child_value"):
            out["%s/%s" % (mode, k)] = ex[k].cpu().numpy()
        if c.get("reward"):
            child, reward = ts.estimate_reward(r, h, parents_are_joint_states=joint)
            out["%s/est_child" % mode] = child.cpu().numpy()
            out["%s/est_reward" % mode] = reward.cpu().numpy()
    torch.cuda.synchronize()
    return out


def humans_next64(c):
    robot, humans = expand_inputs(c)
    P64 = params64(c["flavour"], c["L"])
    cfg = orc.OracleConfig(num_layer=c["L"], skip_connection=c["skip"])
    with torch.no_grad():
        return orc.state_predictor_humans(robot.double()[:, None, :], humans.double(), P64.sp_graph, P64.motion_predictor, cfg).numpy()


def check_humans_next(tag, c, got, worst):
    want = humans_next64(c)
    admit("%s: humans_next H=%d L=%d P=%d %s" % (tag, c["H"], c["L"], c["P"], c["flavour"]), got["bf16x6/humans_next"],
          got["f32/humans_next"], want, worst, reg=REG_F32 if c["flavour"] == "trained" else None)


def check_reward_step(tag, c, got, worst, n_parents=48):
    """The reward step of the expand launch (riding in the scene or the embedding launch) bit for bit against estimate_reward on
    its own; children's values on a spread of parents against float64 on each mode's own inputs (its child rows and predicted
    humans: the children kernel's operation alone)."""
    P, H, L = c["P"], c["H"], c["L"]
    for mode in MODES:
        assert np.array_equal(got["%s/child_robot" % mode], got["%s/est_child" % mode]), (tag, mode, P)
        assert np.array_equal(got["%s/reward" % mode], got["%s/est_reward" % mode]), (tag, mode, P)
    rew = got["bf16x6/reward"]
    counts = (int((rew == -0.25).sum()), int(((rew < 0) & (rew > -0.25)).sum()), int((rew == 1.0).sum()))
    idx = np.unique(np.linspace(0, P - 1, n_parents).astype(np.int64))
    P64 = params64(c["flavour"], L)
    cfg = orc.OracleConfig(num_layer=L, skip_connection=c["skip"])
    want = {}
    for mode in MODES:
        cr = torch.tensor(got["%s/child_robot" % mode][idx]).double()
        hn = torch.tensor(got["%s/humans_next" % mode][idx]).double()
        n, A = cr.shape[0], cr.shape[1]
        with torch.no_grad():
            want[mode] = orc.value_estimator_forward(cr.reshape(n * A, 1, 9), hn[:, None].expand(n, A, H, 5).reshape(n * A, H, 5),
                                                     P64.ve_graph, P64.value_network, cfg).reshape(n, A).numpy()
    bx, f32 = got["bf16x6/child_value"][idx].astype(np.float64), got["f32/child_value"][idx].astype(np.float64)
    e6, e32 = float(np.abs(bx - want["bf16x6"]).max()), float(np.abs(f32 - want["f32"]).max())
    close(bx, want["bf16x6"], reg=REG_F32)
    close(f32, want["f32"], reg=REG_F32)
    assert e6 <= 1.5 * e32 + EPS32 * max(1.0, float(np.abs(want["bf16x6"]).max())), (tag, P, e6, e32)
    if F32_IS_F32:
        assert not np.array_equal(bx, f32), (tag, P)
    worst.bx, worst.f32, worst.n = max(worst.bx, e6), max(worst.f32, e32), worst.n + 1
    return counts


# (H, L, skip, flavour, P): N = 17..32 (two node tiles), L = 1..4; P picks the launch form of the bf16x6 scene kernel --
# split with the embeddings inside (P <= 512), split without (P < 3072), unsplit
A1_CASES = [(16, 1, True, "trained", 3), (17, 2, True, "rand", 512), (24, 3, False, "trained", 513), (31, 4, True, "trained", 1500),
            (17, 2, False, "trained", 3072), (24, 2, True, "rand", 4000), (31, 2, True, "trained", 3), (16, 4, False, "rand", 700)]
# (env, cases): each launch form forced for sizes the default dispatch gives another one
A1_FORCED = [({"RGL_SCENE_EMBED_INSIDE": "0"}, [(17, 2, True, "trained", 3), (31, 3, False, "rand", 512)]),
             ({"RGL_SCENE_SPLIT_BELOW": "0"}, [(24, 2, True, "trained", 3), (16, 4, True, "trained", 512), (31, 1, True, "rand", 1500)]),
             ({"RGL_SCENE_SPLIT_BELOW": "1000000"}, [(17, 3, True, "trained", 3072), (24, 2, False, "trained", 4000)])]


def a1_case(H, L, skip, flavour, P):
    return dict(H=H, L=L, skip=skip, flavour=flavour, P=P, seed=5100 + 7 * H + L + P)


def test_state_predictor_bf16x6_scene_kernel_forms_vs_float64(dev, tmp_path):
    """A1: the predicted humans of expand (rgl_scene.hip, scene_graph_kernel<2, 0, *, *, *, BX = true>) in every launch form
    against float64 StatePredictor arithmetic; the crowds the form does not cover (N = 16: one node tile, N = 33: three) run the
    f32 kernel bit for bit."""
    worst = Worst()
    for args in A1_CASES:
        c = a1_case(*args)
        check_humans_next("default dispatch", c, expand_outputs(c, dev), worst)
    for env_add, cases in A1_FORCED:
        cs = [a1_case(*args) for args in cases]
        tag = "_".join("%s%s" % kv for kv in env_add.items())
        got = run_child("expand", cs, env_add, tmp_path, tag)
        for i, c in enumerate(cs):
            check_humans_next(tag, c, {k.split("/", 1)[1]: v for k, v in got.items() if k.startswith("%d/" % i)}, worst)
    for H in (15, 32):
        for P in (3, 1500):
            got = expand_outputs(a1_case(H, 2, True, "trained", P), dev)
            assert np.array_equal(got["bf16x6/humans_next"], got["f32/humans_next"]), (H, P)
    report("A1 bf16x6 scene kernel (predicted humans; H 16..31, L 1..4, split with / without embedded rows, unsplit, and each forced "
           "in a child process): " + worst.line() + "; H = 15 / 32 bit-identical to f32")


def test_reward_step_inside_and_outside_the_bf16x6_scene_launch(dev, tmp_path):
    """A2: the level's reward step rides in the scene launch below 1100 scenes in bf16x6 (3072 in f32), in the embedding launch
    above (rgl_scene.hip, launch_predict_humans): on dense crowds (collisions, discomfort, goals) the rewards and child rows of
    expand equal estimate_reward's on its own bit for bit (holonomic) on both sides of both cut-offs and with the cut-off forced;
    the children's values of the same launches against float64."""
    worst = Worst()
    counts = np.zeros(3, np.int64)
    cases = [dict(H=19, L=2, skip=True, flavour="trained", P=P, seed=6200 + P, dense=True, reward=True, joint=bool(P % 2))
             for P in (1099, 1100, 3071, 3072)]
    for c in cases:
        counts += check_reward_step("default dispatch", c, expand_outputs(c, dev), worst)
    for below in ("0", "1000000"):
        cs = [dict(H=H, L=2, skip=True, flavour="trained", P=P, seed=6300 + P + H, dense=True, reward=True, joint=bool(H % 2))
              for H, P in ((19, 600), (31, 37))]
        got = run_child("expand", cs, {"RGL_SCENE_CHILDREN_BELOW": below}, tmp_path, "below" + below)
        for i, c in enumerate(cs):
            counts += check_reward_step("RGL_SCENE_CHILDREN_BELOW=" + below, c,
                                        {k.split("/", 1)[1]: v for k, v in got.items() if k.startswith("%d/" % i)}, worst)
    assert counts.min() > 100, counts                      # every branch of the reward occurs
    report("A2 reward step in / beside the bf16x6 scene launch (P = 1099 / 1100 / 3071 / 3072 and forced): rewards and child rows bit "
           "for bit (%d collisions, %d discomfort values, %d goals); children's values: %s" % (tuple(counts) + (worst.line(),)))


def test_path_g_bf16x6_value_rows_split_and_unsplit_vs_float64(dev):
    """A3: path G's value rows in bf16x6 (B x 81 scenes: split below 3072, unsplit above) against the batched oracle in float64;
    decisions as in test_path_g_bf16x6_weight_products_at_size."""
    import bench
    sd64 = {k: v.double() for k, v in gio.path_g_sd().items()}
    worst = Worst()
    for H, B in ((16, 4), (31, 37), (16, 64), (31, 64), (16, 37)):
        robot, humans = bench.synth_scenes(7300 + H + B, B, H)
        ob, ov = orc.gcn_predict_batched(robot.numpy(), humans.numpy(), sd64, orc.OracleConfig(), dtype=torch.float64)
        out = {}
        for mode in MODES:
            pol = make_gcn_policy(device=dev)
            pol.contraction_dtype = mode
            pol.build_action_space(1.0)
            vals, best = pol.gcn_search().search(robot.to(dev), humans.to(dev))
            out[mode] = (vals.cpu().numpy().astype(np.float64), best.cpu().numpy().astype(np.int64))
        assert out["bf16x6"][0].shape == (B, 81)
        admit("path G H=%d B=%d (%d scenes)" % (H, B, 81 * B), out["bf16x6"][0], out["f32"][0], ov, worst)
        for b in np.nonzero(out["bf16x6"][1] != ob)[0]:
            assert ov[b, ob[b]] - ov[b, out["bf16x6"][1][b]] <= TOL, (H, B, b)
    report("A3 path G bf16x6 value rows (H 16 / 31, 324..5184 scenes: split and unsplit): " + worst.line())


# ---------------------------------------------------------------------------------------------------
# B: the fused children kernel under every dealing plan
# ---------------------------------------------------------------------------------------------------
TABLES = {9: (1, 8), 16: (3, 5), 25: (3, 8), 81: (5, 16), 96: (5, 19), 97: (6, 16)}       # A -> (speed, rotation samples)


def forced_plan(P, A, G, inline, n_cu):
    """plan_items (rgl_fused.hip) restated for a forced cut: RGL_FUSED_G = G (clamped to the tiles that run their own head),
    RGL_FUSED_INLINE_PARTIAL = inline; one parent per unit (no tail).  -> dict(G, ipp, rot, k, inline, n_full, rem)."""
    n_full, rem = divmod(A, 16)
    k = max(1, -(-P // n_cu))
    inl = 1 if (inline and rem) else 0
    n_tiles = n_full + inl
    CT = max(n_tiles, 1)
    G = min(G, CT)
    ipp = -(-CT // G)
    last = n_tiles - (ipp - 1) * G
    c_full = 0.45 + G
    c_last = 0.45 + max(last, 0) + (0.45 if rem and not inl else 0.0)
    rot = ipp - 1 if ipp > 1 and c_last > c_full else 0
    return dict(G=G, ipp=ipp, rot=rot, k=k, inline=inl, n_full=n_full, rem=rem)


def plan_allowed(plan):
    """Forced plans the cost model can itself return: an inline partial tile only where k * rem <= 8."""
    return not plan["inline"] or plan["k"] * plan["rem"] <= 8


# (RGL_FUSED_G, RGL_FUSED_INLINE_PARTIAL): None = the cost model's own choice
FUSED_SETTINGS = [(None, None), (1, 0), (2, 0), (3, 0), (99, 0), (1, 1), (2, 1), (4, 1)]


def fused_cases(C):
    """(A, P, H, similarity, skip, flavour) over partial-only / full-only / mixed tables, k = 1, 2, 3 and 10 parents per workgroup,
    both sides of every register bucket edge (N = 8 / 9, 16 / 17, 20 / 21) and the non-softmax instantiations <8,1>, <20,1>, <20,2>."""
    eg = "embedded_gaussian"
    return [(9, 1, 1, eg, True, "trained"), (16, 7, 7, eg, False, "trained"), (25, C, 8, eg, True, "rand"),
            (81, C + 1, 15, eg, True, "trained"), (96, 7, 16, eg, False, "trained"), (97, 2 * C + 3, 19, eg, True, "trained"),
            (9, 9 * C + 5, 7, eg, True, "trained"), (97, 1, 16, eg, True, "rand"), (16, 9 * C + 5, 8, eg, False, "trained"),
            (81, 7, 20, eg, True, "trained"), (97, C, 31, eg, False, "rand"),
            (25, 2 * C + 3, 19, "squared", True, "trained"), (16, C + 1, 7, "diagonal", False, "trained"),
            (81, 7, 15, "squared", True, "trained"), (96, 2 * C + 3, 1, "diagonal", True, "trained")]


def fused_bx_live(H, sim):
    """The fused kernel's bf16x6 forms that fit a CU's LDS: <8,1> and <20,1> for every similarity, <20,2> (N = 17..20) for the
    softmax one only; the others (N = 17..20 with a plain-weight similarity, N = 21..32) run the f32 form on an image of their own.
    (rgl_fused.h states the same window in static_asserts on fused_form_fits, and no kernel is compiled outside it.)"""
    N = H + 1
    return N <= 16 or (N <= 20 and sim == "embedded_gaussian")


def children_inputs(c):
    s, r = TABLES[c["A"]]
    robot, humans = seeded_scenes(8100 + c["A"] + c["H"], c["P"], c["H"])
    acts, _ = orc.mprl_action_space(orc.OracleConfig(speed_samples=s, rotation_samples=r), 1.0)
    return orc._children_robot(robot, acts, orc.OracleConfig()), humans


def children_outputs(c, dev):
    cr, humans = children_inputs(c)
    s, r = TABLES[c["A"]]
    out = {}
    for mode in MODES:
        pol = make_mprl_policy(c["flavour"], 1, L=2, skip=c["skip"], similarity=c["sim"], device=dev)
        pol.contraction_dtype = mode
        pol.speed_samples, pol.rotation_samples = s, r
        pol.build_action_space(1.0)
        ts = pol.tree_search()
        assert ts.num_actions == c["A"], (ts.num_actions, c["A"])
        out[mode] = ts.value_children(cr.to(dev), humans.to(dev)).cpu().numpy()
    torch.cuda.synchronize()
    return out


def test_fused_children_kernel_every_dealing_plan_both_modes(dev, tmp_path):
    """B: the fused children kernel (rgl_fused_kernel.hip) under each forced dealing plan -- tiles per item G, the inline partial tile --
    and the cost model's own, in child processes with RGL_CHILDREN_FUSED=1 (so that f32 takes the small launches too): f32 and
    bf16x6 against float64 ValueEstimator arithmetic.  N <= 20: (a)-(c); N = 21..32: the bf16x6 request runs the f32 kernel on an
    image of its own (the larger image does not fit a CU), bit for bit."""
    C = torch.cuda.get_device_properties(dev).multi_processor_count
    cases = [dict(A=A, P=P, H=H, sim=sim, skip=skip, flavour=fl) for A, P, H, sim, skip, fl in fused_cases(C)]
    want = []
    for c in cases:
        cr, humans = children_inputs(c)
        P, A, H = c["P"], c["A"], c["H"]
        P64 = params64(c["flavour"], 2, c["sim"])
        with torch.no_grad():
            want.append(orc.value_estimator_forward(cr.double().reshape(P * A, 1, 9),
                                                    humans.double()[:, None].expand(P, A, H, 5).reshape(P * A, H, 5),
                                                    P64.ve_graph, P64.value_network,
                                                    orc.OracleConfig(skip_connection=c["skip"], similarity=c["sim"])).reshape(P, A).numpy())
    worst, worst_f32_wide = Worst(), 0.0
    reached = set()
    labels = []
    for G, inline in FUSED_SETTINGS:
        env_add = {"RGL_CHILDREN_FUSED": "1"}
        if G is not None:
            env_add["RGL_FUSED_G"] = str(G)
            env_add["RGL_FUSED_INLINE_PARTIAL"] = str(inline)
        plans = [forced_plan(c["P"], c["A"], G, inline, C) if G is not None else None for c in cases]
        idx = [i for i, p in enumerate(plans) if p is None or plan_allowed(p)]
        tag = "G%s_inline%s" % (G, inline)
        got = run_child("children", [cases[i] for i in idx], env_add, tmp_path, tag)
        for j, i in enumerate(idx):
            c, p = cases[i], plans[i]
            bx, f32 = got["%d/bf16x6" % j], got["%d/f32" % j]
            label = "A=%d P=%d H=%d %s skip=%d, %s" % (c["A"], c["P"], c["H"], c["sim"], c["skip"],
                                                       "cost model" if p is None else
                                                       "G=%d ipp=%d rot=%d k=%d inline=%d" % (p["G"], p["ipp"], p["rot"], p["k"], p["inline"]))
            if fused_bx_live(c["H"], c["sim"]):
                admit(label, bx, f32, want[i], worst, reg=REG_F32 if c["flavour"] == "trained" else None)
            else:
                assert np.array_equal(bx, f32), (label, "outside the bf16x6 window: the f32 kernel, bit for bit")
                e = close(f32, want[i], reg=REG_F32 if c["flavour"] == "trained" else None)
                worst_f32_wide = max(worst_f32_wide, e)
            if p is not None:
                reached |= {"rot != 0"} if p["rot"] else set()
                reached |= {"ipp >= 3"} if p["ipp"] >= 3 else set()
                reached |= {"inline partial, k >= 2"} if p["inline"] and p["k"] >= 2 else set()
                reached |= {"k >= 9"} if p["k"] >= 9 else set()
                reached |= {"partial tile only"} if p["n_full"] == 0 else set()
                reached |= {"full tiles only"} if p["rem"] == 0 else set()
                labels.append("G=%d/ipp=%d/rot=%d/k=%d/inl=%d" % (p["G"], p["ipp"], p["rot"], p["k"], p["inline"]))
    need = {"rot != 0", "ipp >= 3", "inline partial, k >= 2", "k >= 9", "partial tile only", "full tiles only"}
    assert need <= reached, need - reached
    report("B fused children kernel, %d dealing settings x %d shapes (C = %d CUs): %s; outside the bf16x6 window bit-identical to f32, "
           "%.2e; %d distinct forced plans covered (%s)" % (len(FUSED_SETTINGS), len(cases), C, worst.line(), worst_f32_wide,
                                                            len(set(labels)), ", ".join(sorted(reached))))


# ---------------------------------------------------------------------------------------------------
# C: the strong-scaling slices of the 8-GPU runs in bf16x6
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B", [(2, 2048), (3, 4096)])
def test_last_rank_slice_of_the_strong_scaling_sets_in_bf16x6(D, B, dev):
    """The last rank's share (rga.shard_bounds(B, 8, 7)) of bench.py's scenes searched alone in bf16x6 -- the tail's back-up
    chain over `unit` > 1 parents (P / u >= CUs / 2), a dealing of its own -- against the memoised full-size oracle, sliced (the
    levels are root-major: level l holds parents [lo w^l, hi w^l)), and against the same roots inside the full batch; repeated runs
    and a root permutation bit-exact.  (bench.synth_scenes(1000, 256) is not a slice of the 2048-root set: hence this test.)"""
    import bench
    H, L, w = 19, 2, 2
    robot, humans = bench.synth_scenes(1000, B, H)
    lo, hi = rga.shard_bounds(B, 8, 7)
    oracle_out, v1, levels = _oracle_at_size(H, L, D, B, robot, humans)
    o_sl = [x[lo:hi] for x in oracle_out]
    lv_sl = [{"value1": lv["value1"][lo * w ** l:hi * w ** l], "keep": lv["keep"][lo * w ** l:hi * w ** l]} for l, lv in enumerate(levels)]
    tag = "last rank of 8 (roots %d..%d of %d, depth %d), bf16x6" % (lo, hi, B, D)
    pol = _bench_policy(L, D, H, "bf16x6", dev)
    r, h = robot[lo:hi].contiguous().to(dev), humans[lo:hi].contiguous().to(dev)
    act, val = pol.predict_batch(r, h, roots_are_joint_states=True)
    act, val = act.clone(), val.clone()
    _, n_div, _ = compare_trees(tag, pol.tree_search(), val, o_sl, lv_sl, TOL, REG_F32)
    err = close(val.cpu().numpy(), o_sl[1].numpy(), reg=None if n_div else REG_F32)
    check_decisions(tag, act, val, o_sl, [{"value1": v1[lo:hi]}], TOL)
    a2, v2 = pol.predict_batch(r, h, roots_are_joint_states=True)
    assert torch.equal(a2, act) and torch.equal(v2, val)
    perm = torch.randperm(hi - lo, generator=torch.Generator().manual_seed(7)).to(dev)
    a3, v3 = pol.predict_batch(r[perm].contiguous(), h[perm].contiguous(), roots_are_joint_states=True)
    assert torch.equal(a3, act[perm]) and torch.equal(v3, val[perm])
    af, vf = _bench_policy(L, D, H, "bf16x6", dev).predict_batch(robot.to(dev), humans.to(dev), roots_are_joint_states=True)
    dv = float((vf[lo:hi] - val).abs().max())
    differ = int((af[lo:hi] != act).sum())
    assert dv <= REG_F32 and differ <= 2, (dv, differ)
    report("%s: max |dV| vs the oracle %.2e; vs the same roots inside the full batch %.1e, %d decisions differ; repeat and root "
           "permutation bit-exact" % (tag, err, dv, differ))
