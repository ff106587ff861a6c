"""The level prologue of the fused children kernel (RGL_LEVEL_PROLOGUE): a tree level as ONE launch, whose workgroups run the state
predictor and the reward / next-state pairs of the parents they own before scoring those parents' children, against the
three-launch form (RGL_LEVEL_PROLOGUE=0) in separate processes.  Both forms run the same device code on the same inputs, so every
per-level array (humans_next, child_robot, reward, child_value) and every output must be bit-identical."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import relationalgraphlearning_amd as rga
from tests.helpers import make_mprl_policy
from tests.test_gpu_parity import report, seeded_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (humans, roots, depth, width, seed): configs[2] at 2048 and 256 roots (the latter below the prologue's parent count: both runs take
# the three launches), configs[3]'s 512-root share at depth 3 (its second and third levels fold), a root count that is not a multiple
# of the CU count, N = 17 (the smallest crowd of the form)
CASES = [(19, 2048, 2, 2, 5), (19, 256, 2, 2, 6), (19, 512, 3, 2, 7), (19, 1000, 2, 2, 8), (16, 512, 2, 2, 9)]
CAPTURED = (19, 1024, 2, 2, 10)
LEVEL_KEYS = ("humans_next", "child_robot", "reward", "child_value")


def make_search(H, D, w, dev):
    pol = make_mprl_policy("trained", D, w, True, device=dev)
    pol.build_action_space(1.0)
    return rga.TreeSearch(pol.value_estimator, pol.state_predictor, rga.actions.as_array(pol.action_space), None, pol.kinematics,
                          pol.time_step, pol.get_normalized_gamma(), D, w, True, False, contraction_dtype="bf16x6")


def search_outputs(case, dev):
    H, B, D, w, seed = case
    robot, humans = seeded_scenes(seed, B, H)
    ts = make_search(H, D, w, dev)
    o = ts.search(robot.to(dev), humans.to(dev), True)
    torch.cuda.synchronize()
    res = {k: o[k].cpu().numpy() for k in ("best_action", "best_value", "root_values", "root_kept")}
    for l in range(D):
        lv = ts.level_arrays(l)
        for k in LEVEL_KEYS + ("reward_clip",):
            if k in lv:
                res["L%d/%s" % (l, k)] = lv[k].cpu().numpy()
    return res


def captured_outputs(case, dev):
    H, B, D, w, seed = case
    robot, humans = seeded_scenes(seed, B, H)
    ts = make_search(H, D, w, dev)
    r, h = robot.to(dev), humans.to(dev)
    direct = ts.search(r, h, True)
    direct = {k: direct[k].clone() for k in ("best_action", "best_value")}
    graph, out = ts.capture(r.clone(), h.clone(), True, private_workspace=True)
    graph.replay()
    torch.cuda.synchronize()
    res = {"direct/" + k: v.cpu().numpy() for k, v in direct.items()}
    res.update({"graph/" + k: out[k].cpu().numpy() for k in ("best_action", "best_value")})
    return res


def child_main(spec, out):
    """Entry point of the child processes (run_child)."""
    with open(spec) as f:
        s = json.load(f)
    dev = torch.device("cuda:0")
    res = {}
    for i, c in enumerate(s["cases"]):
        for k, v in search_outputs(c, dev).items():
            res["%d/%s" % (i, k)] = v
    for k, v in captured_outputs(s["captured"], dev).items():
        res["cap/" + k] = v
    np.savez(out, **res)
    print("OK")


def run_child(prologue, tmp_path):
    spec, out = str(tmp_path / ("p%s.json" % prologue)), str(tmp_path / ("p%s.npz" % prologue))
    with open(spec, "w") as f:
        json.dump({"cases": CASES, "captured": CAPTURED}, f)
    code = "import sys\nfrom tests.test_level_prologue import child_main\nchild_main(sys.argv[1], sys.argv[2])\n"
    env = dict(os.environ, RGL_LEVEL_PROLOGUE=prologue)
    res = subprocess.run([sys.executable, "-c", code, spec, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "OK" in res.stdout, (prologue, res.stdout[-2000:] + res.stderr[-3000:])
    return dict(np.load(out))


@pytest.mark.gpu
def test_level_prologue_matches_three_launches(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    one = run_child("1", tmp_path)
    three = run_child("0", tmp_path)
    assert sorted(one) == sorted(three)
    for k in sorted(one):
        assert one[k].dtype == three[k].dtype and one[k].shape == three[k].shape, k
        assert one[k].tobytes() == three[k].tobytes(), (k, float(np.abs(one[k].astype(np.float64) - three[k]).max()))
    for k in ("best_action", "best_value"):                    # the captured search replays what the direct call computes
        assert one["cap/graph/" + k].tobytes() == one["cap/direct/" + k].tobytes(), k
    report("level prologue: %d arrays over %d searches + a captured one bit-identical to the three-launch form" % (len(one), len(CASES)))
