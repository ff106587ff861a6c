"""graph_kernel<NT, XT, L, BWD, COS, LW> of csrc/rgl_graph_kernel.h in every instantiation it launches, with workgroups that walk
several scenes (tests/graph_forms.py: the runs, the instantiation and the grid each takes by the library's own planner -- held on
the CPU by tests/test_graph_forms_cpu.py -- and the references).  The harness is tests/test_row_forms.py's.

  a. forward and every parameter gradient of every run against torch autograd over the oracle in FLOAT64 -- w_a and each Ws.l
     scaled on their own -- under the project's bounds (1e-4 of max(1, largest entry); 2e-4 of the gradient's largest entry) and a
     regression-level bound beside each: max(REG_F32 | REG_GRAD, 8 x the deviation of the same oracle evaluated in float32 on the
     CPU).  The state predictor with detach False and True.  Forward-only runs (hl_row0, all rows, sibling scenes) the same way.
  b. the tile pipeline within 5e-5 of the per-scene kernel where that holds a scene (its refusal is RGL_ERR_LDS where it does not),
     two runs of one form bit-identical.
  c. the configurations the pipeline refuses are loud in the backward (RGL_ERR_BAD_MODE under RGL_BACKWARD_MFMA=2), loud or correct
     in the forward, and a valid run right after each is still correct.
  d. the whole module once more with poisoned workspaces.

One child process per environment, started once per session, each under its own time limit; a child that fails -- by an assertion, a
signal, an abort or its time limit -- fails every test that needs it and is not started again.  profiles/graph_kernel_forms.txt
holds the parity-report lines of a run of this module.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd.nets import graph_forward
from tests import graph_forms as gf
from tests import row_forms as rf
from tests import test_row_forms as trf
from tests.test_gpu_parity import REG_F32, TOL, report

pytestmark = pytest.mark.gpu
ROOT = trf.ROOT
FORMS_TOL = trf.FORMS_TOL
WHAT = "graph kernel forms"
ENVS = {
    "tiles": {"RGL_BACKWARD_MFMA": "2", "RGL_TILES_FORWARD": "2", "RGL_REQUIRE_MFMA_FORWARD": "1"},
    "scene": {"RGL_BACKWARD_MFMA": "0", "RGL_TILES_FORWARD": "0"},      # the per-scene kernels
}
REFUSED = [gf.refused_run(e) for e in gf.REFUSED]


def walked(run):
    """"<instantiation>, <grid> workgroups of <fewest>-<most> scenes" of the run's backward (forward-only runs: forward) launch."""
    cap = 2048 if run.forward_only else gf.backward_cap(run)[0]
    p = gf.plan(run, not run.forward_only, cap)
    return "%s, %d workgroups of %d-%d scenes" % ((run.inst, p["grid"]) + gf.scenes_walked(run, p["grid"]))


# ---------------------------------------------------------------------------------------------------------------------------
# the child processes
# ---------------------------------------------------------------------------------------------------------------------------
def forward_only(run, dev):
    """The forward without autograd, twice: the value head reads the robot row alone (hl_row0), the motion head all rows; `spc`
    sibling scenes share a crowd."""
    mod, g, head = rf.build(run)
    mod.to(dev)
    robot, humans = rf.scenes(run)
    r, h = robot.to(dev), humans.to(dev)

    def once():
        with torch.no_grad():
            if run.module == "value":
                return graph_forward(g.descriptor(), mod.head_descriptor(), None, r, h, scenes_per_crowd=run.spc)["value"].cpu().numpy()
            return graph_forward(g.descriptor(), None, mod.head_descriptor(), r, h, scenes_per_crowd=run.spc)["humans_next"].cpu().numpy()
    first, again = once(), once()
    return {"out": first, "repeat_ok": np.array(np.array_equal(first, again))}


def child_main(name, out):
    """Entry point of the child of environment `name`: every run; in `tiles`, section c after them."""
    dev = torch.device("cuda:0")
    res = {}
    for run in gf.RUNS:
        for detach in ((False, True) if run.module == "motion" and not run.forward_only else (False,)):
            prefix = run.id + ("/detach" if detach else "")
            fn = (lambda: forward_only(run, dev)) if run.forward_only else (lambda: trf.measure(run, dev, detach))
            if name == "scene":
                trf.attempt(res, prefix, fn)                    # a scene may not fit the per-scene kernel
            else:
                for k, v in fn().items():
                    res["%s/%s" % (prefix, k)] = v
        print("done", run.id, flush=True)
    if name == "tiles":
        valid = gf.RUN[gf.VALID]
        for run in REFUSED:
            trf.attempt(res, run.id + "/backward", lambda: trf.measure(run, dev))
            trf.attempt(res, run.id + "/after_backward", lambda: trf.measure(valid, dev))
            trf.attempt(res, run.id + "/forward", lambda: forward_only(run, dev))
            trf.attempt(res, run.id + "/after_forward", lambda: forward_only(valid, dev))
            print("done refusals of", run.id, flush=True)
    torch.cuda.synchronize()
    np.savez(out, **res)
    print("OK")


_children = {}


def child(name, tmp_path_factory):
    """The arrays of environment `name`'s child, started ONCE per session, one child at a time; a failure is kept and raised again."""
    if name not in _children:
        out = str(tmp_path_factory.mktemp("graph_forms") / (name + ".npz"))
        code = "import sys\nfrom tests.test_graph_forms import child_main\nchild_main(sys.argv[1], sys.argv[2])\n"
        env = {k: v for k, v in os.environ.items() if k not in ("RGL_HEAD_ROWS_DIRECT", "RGL_REQUIRE_MFMA_FORWARD", "RGL_BACKWARD_MFMA_MIN")}
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


def forward_against_float64(out, run, tag):
    """A forward-only result against the float64 oracle, under TOL and the regression-level bound."""
    ref = gf.reference(run)
    assert ref["masks_agree"] and ref["n_masks"] > 0 and ref["margin"] >= 8, (run.id, "a wrong seed", ref["margin"])
    assert out.shape == ref["out"].shape and out.dtype == np.float32 and np.isfinite(out).all(), tag
    e_f, reg_f = rf.forward_error(out, ref["out"]), max(REG_F32, 8 * ref["yard_fwd"])
    print("%s: forward %.2e (float32 oracle %.2e, bounds %.0e and %.2e)" % (tag, e_f, ref["yard_fwd"], TOL, reg_f))
    assert e_f <= TOL, (tag, e_f)
    assert e_f <= reg_f, ("regression-level bound", tag, e_f, reg_f)
    return e_f, ref["yard_fwd"], reg_f


# ---------------------------------------------------------------------------------------------------------------------------
# a. against float64
# ---------------------------------------------------------------------------------------------------------------------------
CASES_A = [(env, run.id) for env in ENVS for run in gf.RUNS]


@pytest.mark.parametrize("env,run_id", CASES_A, ids=["%s-%s" % c for c in CASES_A])
def test_forward_and_gradients_against_float64(env, run_id, tmp_path_factory):
    run = gf.RUN[run_id]
    got = child(env, tmp_path_factory)
    tag = "%s S=%d N=%d %s %s%s under %s (%s)" % (run.id, run.S, run.H + 1, run.sim, "layerwise " if run.lw else "",
                                                 "skip" if run.skip else "no skip", env, walked(run) if env == "tiles" else "per-scene kernel")
    if run.id + "/error" in got:            # only the per-scene kernel may decline, and only for a scene that does not fit one CU
        assert env == "scene" and "RGL_ERR_LDS" in str(got[run.id + "/error"]), (tag, got[run.id + "/error"])
        report("%s, %s: the per-scene kernel cannot hold the scene (RGL_ERR_LDS)" % (WHAT, tag))
        return
    if run.forward_only:
        e_f, yard, reg_f = forward_against_float64(got[run.id + "/out"], run, tag)
        assert bool(got[run.id + "/repeat_ok"]), (tag, "two runs differ")
        report("%s, %s, forward only, %s, %d scenes per crowd: forward %.2e of the float64 oracle (float32 oracle on the CPU %.2e; "
               "asserted %.0e and %.2e)" % (WHAT, tag, "robot row (hl_row0)" if run.module == "value" else "all rows", run.spc, e_f,
                                           yard, TOL, reg_f))
        return
    trf.against_float64(got, run.id, run, False, tag, "graph", WHAT)
    assert bool(got[run.id + "/repeat_ok"]), (tag, "two runs differ")
    graph = [k for k in got if k.startswith(run.id + "/g/graph.")]
    assert len(graph) == len(run.wr) * 2 + len(run.wh) * 2 + (1 if run.sim == "embedded_gaussian" else 0) + run.L, (tag, graph)
    if run.module == "motion":
        pre = run.id + "/detach"
        trf.against_float64(got, pre, run, True, tag + ", detached", "graph", WHAT)
        assert bool(got[pre + "/graph_absent"]), (tag, "a detached graph model received a gradient")
        assert bool(got[pre + "/repeat_ok"]), (tag, "two detached runs differ")
        heads = [k for k in got if k.startswith(pre + "/g/")]
        assert heads and all(k.startswith(pre + "/g/motion.") for k in heads)
        for k in heads:                     # the motion head's gradients do not depend on what happens behind it
            assert np.array_equal(got[k], got[run.id + k[len(pre):]]), (tag, k)
        assert np.array_equal(got[pre + "/out"], got[run.id + "/out"]), tag


# ---------------------------------------------------------------------------------------------------------------------------
# b. the tile pipeline against the per-scene kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_id", [r.id for r in gf.RUNS])
def test_tile_pipeline_agrees_with_the_per_scene_kernel(run_id, tmp_path_factory):
    run = gf.RUN[run_id]
    base, got = child("scene", tmp_path_factory), child("tiles", tmp_path_factory)
    assert bool(got[run.id + "/repeat_ok"]), run.id
    if run.id + "/error" in base:
        assert "RGL_ERR_LDS" in str(base[run.id + "/error"]), (run.id, base[run.id + "/error"])
        report("%s, %s (%s): the per-scene kernel refuses the scene (RGL_ERR_LDS); the tile pipeline bit-identical between two runs"
               % (WHAT, run.id, walked(run)))
        return
    want = lambda d: sorted(k for k in d if k.startswith(run.id + "/") and ("/g/" in k or k.endswith("/out")))
    keys = want(got)
    assert keys and keys == want(base)
    worst = 0.0
    for k in keys:
        err = rf.grad_error(got[k], base[k].astype(np.float64)) if "/g/" in k else rf.forward_error(got[k], base[k].astype(np.float64))
        assert err <= FORMS_TOL, (run.id, k, err)
        worst = max(worst, err)
    report("%s, %s (%s): within %.1e of the per-scene kernel (asserted %.0e), bit-identical between two runs"
           % (WHAT, run.id, walked(run), worst, FORMS_TOL))


# ---------------------------------------------------------------------------------------------------------------------------
# c. refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_id", [r.id for r in REFUSED])
def test_refused_configurations_are_loud(run_id, tmp_path_factory):
    run, valid = [r for r in REFUSED if r.id == run_id][0], gf.RUN[gf.VALID]
    got = child("tiles", tmp_path_factory)
    err = str(got.get(run.id + "/backward/error"))
    assert "RGL_ERR_BAD_MODE" in err and ("rgl_graph_backward_f32" in err or "rgl_graph_forward_f32" in err), (run.id, err)
    trf.against_float64(got, run.id + "/after_backward", valid, False, "%s after the refusal of %s" % (valid.id, run.id), "graph", WHAT)
    # the forward with the general kernel forbidden: refused, or the one-wave-per-scene kernel's (right) result
    if run.id + "/forward/error" in got:
        assert "RGL_ERR_BAD_MODE" in str(got[run.id + "/forward/error"]), (run.id, got[run.id + "/forward/error"])
        fwd = "refused"
    else:
        fwd = "%.2e of the float64 oracle" % forward_against_float64(got[run.id + "/forward/out"], run, run.id + ", forward")[0]
    forward_against_float64(got[run.id + "/after_forward/out"], valid, "%s forward after %s" % (valid.id, run.id))
    report("%s, %s: the backward raises RGL_ERR_BAD_MODE, the forward is %s; the valid runs that follow are right" % (WHAT, run.id, fwd))


# ---------------------------------------------------------------------------------------------------------------------------
# d. poisoned workspaces
# ---------------------------------------------------------------------------------------------------------------------------
def test_whole_module_with_poisoned_workspaces():
    """Every test above once more with workspaces and outputs filled with NaN patterns before the kernels run: every padding row a
    product reads and every slab a workgroup writes after its last scene was written first."""
    if nat.poison_workspaces():
        return                              # this IS the poisoned run
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_graph_forms.py"), "-q", "-m", "gpu", "-x",
                          "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, RGL_DEBUG_POISON_WORKSPACES="1"),
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and " passed" in res.stdout, res.stdout[-6000:] + res.stderr[-2000:]
    report("%s with poisoned workspaces: %s" % (WHAT, res.stdout.strip().splitlines()[-1].strip("= ")))
