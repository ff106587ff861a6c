"""The workgroup-cooperative embeddings of the level prologue (children_fused_kernel's PRO form: each workgroup embeds the rows of the
parents it owns once per crowd, densely packed, into an LDS row buffer) against the three-launch form (RGL_LEVEL_PROLOGUE=0), in
separate processes.  The arithmetic per row is the same MFMA chain with the same weights and k order in both, so every per-level
array and every output must be byte-identical: no tolerance anywhere.  The same again with poisoned workspaces, and between two
runs in one process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import prologue_embedding as pe
from tests.test_gpu_parity import report, seeded_scenes
from tests.test_level_prologue import make_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(pe.CASES)
LEVEL_KEYS = ("humans_next", "child_robot", "reward", "reward_clip", "child_value")
OUTPUT_KEYS = ("best_action", "best_value", "root_values", "root_kept")


def search_outputs(case, dev):
    H, B, D, w, seed = case
    robot, humans = seeded_scenes(seed, B, H)
    ts = make_search(H, D, w, dev)
    r, h = robot.to(dev), humans.to(dev)
    res = {}
    for run in ("", "again/"):
        o = ts.search(r, h, True)
        torch.cuda.synchronize()
        res.update({run + k: o[k].cpu().numpy() for k in OUTPUT_KEYS})
        for l in range(D):
            lv = ts.level_arrays(l)
            for k in LEVEL_KEYS:
                if k in lv:
                    res["%sL%d/%s" % (run, l, k)] = lv[k].cpu().numpy()
    return res


def child_main(spec, out):
    """Entry point of the child processes (run_child)."""
    with open(spec) as f:
        cases = [tuple(c) for c in json.load(f)]
    dev = torch.device("cuda:0")
    res = {}
    for i, c in enumerate(cases):
        for k, v in search_outputs(c, dev).items():
            res["%d/%s" % (i, k)] = v
    np.savez(out, **res)
    print("OK")


def run_child(prologue, poison, tmp_path):
    tag = "p%s_x%s" % (prologue, poison)
    spec, out = str(tmp_path / (tag + ".json")), str(tmp_path / (tag + ".npz"))
    with open(spec, "w") as f:
        json.dump(CASES, f)
    code = "import sys\nfrom tests.test_prologue_embedding import child_main\nchild_main(sys.argv[1], sys.argv[2])\n"
    env = dict(os.environ, RGL_LEVEL_PROLOGUE=prologue, RGL_DEBUG_POISON_WORKSPACES=poison)
    res = subprocess.run([sys.executable, "-c", code, spec, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "OK" in res.stdout, (tag, res.stdout[-2000:] + res.stderr[-3000:])
    return dict(np.load(out))


def same_bytes(a, b, k):
    assert a.dtype == b.dtype and a.shape == b.shape, k
    assert a.tobytes() == b.tobytes(), (k, float(np.nanmax(np.abs(a.astype(np.float64) - b))))


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["0", "1"])
def test_cooperative_embeddings_match_the_three_launch_form(poison, tmp_path):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    one = run_child("1", poison, tmp_path)
    three = run_child("0", poison, tmp_path)
    assert sorted(one) == sorted(three)
    for i, case in enumerate(CASES):                      # every level's arrays and every output are there, both runs
        D = case[2]
        for run in ("", "again/"):
            for k in OUTPUT_KEYS + tuple("L%d/%s" % (l, k) for l in range(D) for k in LEVEL_KEYS if k != "reward_clip"):
                assert "%d/%s%s" % (i, run, k) in one, (case, run, k)
            assert "%d/%sL0/reward_clip" % (i, run) in one, case
    for k in sorted(one):
        same_bytes(one[k], three[k], k)
        if "/again/" in k:                                # two runs in one process
            same_bytes(one[k], one[k.replace("/again/", "/", 1)], k)
    report("prologue embeddings (poisoned workspaces: %s): %d arrays over %d searches, each run twice, byte-identical to the "
           "three-launch form" % (poison, len(one), len(CASES)))
