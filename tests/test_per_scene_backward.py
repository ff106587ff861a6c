"""rgl_scene_backward_kernel of csrc/rgl_backward.hip in the configurations no other kernel takes (tests/per_scene_backward.py: the
runs, the launch each takes by the library's own planners -- held on the CPU by tests/test_per_scene_backward_cpu.py -- and the
references).  The harness is tests/test_graph_forms.py's.

  a. forward and every parameter gradient of every run against torch autograd over the oracle in FLOAT64 (test_row_forms.
     against_float64: the project's bounds, 1e-4 / 2e-4, and max(REG_F32 | REG_GRAD, 8 x the float32 oracle's deviation) beside them),
     two calls bit-identical; the state predictor with detach False and True, the detached graph model without a gradient and the head
     gradients bit-identical to the attached run's.  Without a GCN layer the similarity block's parameters receive exact zeros.
  b. the default environment and the per-scene switches (RGL_BACKWARD_MFMA=0, RGL_TILES_FORWARD=0) agree bit for bit on every run: the
     tile pipeline has declined, so the switch must not matter.
  c. the walking run (S = 4101: five workgroups take a second scene) with an upstream gradient that is zero for scenes 0 to 4095 is
     bit-identical to a launch of scenes 4096 to 4100 alone.
  d. one human more than fits the LDS of a CU raises RGL_ERR_LDS, and a valid run right after is still right.
  e. the whole module once more with poisoned workspaces: every slab element is written exactly once.

One child process per environment, started once per session, each under its own time limit; a child that fails -- by an assertion, a
signal, an abort or its time limit -- fails every test that needs it and is not started again.  profiles/per_scene_backward.txt holds
the parity-report lines of a run of this module.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from relationalgraphlearning_amd import _native as nat
from tests import per_scene_backward as psb
from tests import test_row_forms as trf
from tests.test_gpu_parity import report

pytestmark = pytest.mark.gpu
ROOT = trf.ROOT
WHAT = "per-scene backward"
TABLE = "scene_backward"
ENVS = {
    "default": {},
    "scene": {"RGL_BACKWARD_MFMA": "0", "RGL_TILES_FORWARD": "0"},
}
SWITCHES = ("RGL_BACKWARD_MFMA", "RGL_BACKWARD_MFMA_MIN", "RGL_TILES_FORWARD", "RGL_HEAD_ROWS_DIRECT", "RGL_REQUIRE_MFMA_FORWARD")


def launch(run):
    p = psb.plan(run)
    return "%d workgroups of up to %d scenes, %d bytes of LDS" % (p["grid"], p["scenes_per_wg"], p["lds_bytes"])


# ---------------------------------------------------------------------------------------------------------------------------
# the child processes
# ---------------------------------------------------------------------------------------------------------------------------
def child_main(name, out):
    """Entry point of the child of environment `name`: every run, then the refusals, each followed by the valid run."""
    dev = torch.device("cuda:0")
    res = {}
    for run in psb.RUNS:
        for detach in ((False, True) if run.module == "motion" else (False,)):
            prefix = run.id + ("/detach" if detach else "")
            for k, v in trf.measure(run, dev, detach).items():
                res["%s/%s" % (prefix, k)] = v
        print("done", run.id, flush=True)
    valid = psb.RUN[psb.VALID]
    for run in psb.REFUSALS:
        trf.attempt(res, run.id + "/backward", lambda: trf.measure(run, dev))
        trf.attempt(res, run.id + "/after", lambda: trf.measure(valid, dev))
        print("done refusal of", run.id, flush=True)
    torch.cuda.synchronize()
    np.savez(out, **res)
    print("OK")


_children = {}


def child(name, tmp_path_factory):
    """The arrays of environment `name`'s child, started ONCE per session, one child at a time; a failure is kept and raised again."""
    if name not in _children:
        out = str(tmp_path_factory.mktemp("per_scene_backward") / (name + ".npz"))
        code = "import sys\nfrom tests.test_per_scene_backward import child_main\nchild_main(sys.argv[1], sys.argv[2])\n"
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(ENVS[name])
        try:
            res = subprocess.run([sys.executable, "-c", code, name, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
            if res.returncode != 0 or "OK" not in res.stdout:
                raise AssertionError("child ended with %s\n%s" % (res.returncode, res.stdout[-2000:] + res.stderr[-4000:]))
            _children[name] = dict(np.load(out))
        except Exception as e:              # also the time limit: remembered, not retried
            _children[name] = e
    if isinstance(_children[name], Exception):
        raise AssertionError("the child process of environment %s failed (started once): %s" % (name, _children[name]))
    return _children[name]


def arrays(got, run_id):
    return sorted(k for k in got if k.startswith(run_id + "/") and ("/g/" in k or k.endswith("/out")))


# ---------------------------------------------------------------------------------------------------------------------------
# a. against float64
# ---------------------------------------------------------------------------------------------------------------------------
CASES_A = [(env, run.id) for env in ENVS for run in psb.RUNS]


@pytest.mark.parametrize("env,run_id", CASES_A, ids=["%s-%s" % c for c in CASES_A])
def test_forward_and_gradients_against_float64(env, run_id, tmp_path_factory):
    run = psb.RUN[run_id]
    got = child(env, tmp_path_factory)
    tag = "%s S=%d N=%d x_dim=%d L=%d %s %s%s under %s (%s)" % (run.id, run.S, run.H + 1, run.X, run.L, run.sim, "layerwise " if run.lw else "",
                                                               "skip" if run.skip else "no skip", env, launch(run))
    graph = [k for k in got if k.startswith(run.id + "/g/graph.")]
    assert len(graph) == len(run.wr) * 2 + len(run.wh) * 2 + len(psb.block_parameters(run)) + run.L, (tag, graph)
    if run.L == 0:                          # torch: the block received no gradient at all; the kernel: zeros, and exact ones
        unused = [run.id + "/g/" + k for k in psb.block_parameters(run)]
        assert all(k in got and not got[k].any() for k in unused), (tag, unused)
        got = {k: v for k, v in got.items() if k not in unused}
    trf.against_float64(got, run.id, run, False, tag, TABLE, WHAT)
    assert bool(got[run.id + "/repeat_ok"]), (tag, "two runs differ")
    if run.module == "motion":
        pre = run.id + "/detach"
        trf.against_float64(got, pre, run, True, tag + ", detached", TABLE, WHAT)
        assert bool(got[pre + "/graph_absent"]), (tag, "a detached graph model received a gradient")
        assert bool(got[pre + "/repeat_ok"]), (tag, "two detached runs differ")
        heads = [k for k in got if k.startswith(pre + "/g/")]
        assert heads and all(k.startswith(pre + "/g/motion.") for k in heads)
        for k in heads:                     # the motion head's gradients do not depend on what happens behind it
            assert np.array_equal(got[k], got[run.id + k[len(pre):]]), (tag, k)
        assert np.array_equal(got[pre + "/out"], got[run.id + "/out"]), tag


# ---------------------------------------------------------------------------------------------------------------------------
# b. the switches do not matter
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_id", [r.id for r in psb.RUNS])
def test_default_and_per_scene_switches_agree_bit_for_bit(run_id, tmp_path_factory):
    run = psb.RUN[run_id]
    base, got = child("scene", tmp_path_factory), child("default", tmp_path_factory)
    keys = arrays(got, run.id)
    assert keys and keys == arrays(base, run.id), (run.id, keys)
    assert any("/g/" in k for k in keys) and run.id + "/out" in keys
    for k in keys:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], base[k]), (run.id, k)
    report("%s, %s: the default environment and RGL_BACKWARD_MFMA=0 RGL_TILES_FORWARD=0 agree bit for bit on %d arrays"
           % (WHAT, run.id, len(keys)))


# ---------------------------------------------------------------------------------------------------------------------------
# c. a workgroup's second scene owes nothing to its first
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", list(ENVS))
def test_walking_run_matches_its_tail_alone(env, tmp_path_factory):
    walk, tail = psb.RUN[psb.WALK], psb.RUN[psb.WALK_TAIL]
    got = child(env, tmp_path_factory)
    grads = [k[len(walk.id):] for k in arrays(got, walk.id) if "/g/" in k]
    assert grads and sorted(grads) == sorted(k[len(tail.id):] for k in arrays(got, tail.id) if "/g/" in k)
    for k in grads:
        assert np.array_equal(got[walk.id + k], got[tail.id + k]) and got[tail.id + k].any(), (env, k)
    assert np.array_equal(got[walk.id + "/out"][walk.dark:], got[tail.id + "/out"]), env
    report("%s, %s under %s (%s): %d gradients bit-identical to scenes %d to %d launched alone" %
           (WHAT, walk.id, env, launch(walk), len(grads), walk.dark, walk.S - 1))


# ---------------------------------------------------------------------------------------------------------------------------
# d. the LDS limit
# ---------------------------------------------------------------------------------------------------------------------------
CASES_D = [(env, run.id) for env in ENVS for run in psb.REFUSALS]


@pytest.mark.parametrize("env,run_id", CASES_D, ids=["%s-%s" % c for c in CASES_D])
def test_one_human_more_than_fits_is_refused_loudly(env, run_id, tmp_path_factory):
    run, valid = [r for r in psb.REFUSALS if r.id == run_id][0], psb.RUN[psb.VALID]
    got = child(env, tmp_path_factory)
    err = str(got.get(run.id + "/backward/error"))
    assert "RGL_ERR_LDS" in err and "rgl_graph_backward_f32" in err, (run.id, err)
    assert not [k for k in got if k.startswith(run.id + "/backward/") and not k.endswith("/error")], run.id
    trf.against_float64(got, run.id + "/after", valid, False, "%s after the refusal of %s under %s" % (valid.id, run.id, env), TABLE, WHAT)
    report("%s, %s under %s: N = %d raises RGL_ERR_LDS (%d bytes; N = %d fits with %d); the valid run that follows is right"
           % (WHAT, run.id, env, run.H + 1, psb.plan(run)["lds_bytes"], run.H, psb.plan(run, H=run.H - 1)["lds_bytes"]))


# ---------------------------------------------------------------------------------------------------------------------------
# e. poisoned workspaces
# ---------------------------------------------------------------------------------------------------------------------------
def test_whole_module_with_poisoned_workspaces():
    """Every test above once more with workspaces and outputs filled with NaN patterns before the kernels run: a slab element that a
    scene does not write, or adds to before writing it (`first`), turns a gradient into NaN."""
    if nat.poison_workspaces():
        return                              # this IS the poisoned run
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_per_scene_backward.py"), "-q", "-m", "gpu", "-x",
                          "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, RGL_DEBUG_POISON_WORKSPACES="1"),
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and " passed" in res.stdout, res.stdout[-6000:] + res.stderr[-2000:]
    report("%s with poisoned workspaces: %s" % (WHAT, res.stdout.strip().splitlines()[-1].strip("= ")))
