"""The MLP row kernels of csrc/rgl_rows.hip, forward and backward, in every form they launch (tests/row_forms.py: the
runs, the form each takes by the library's own planner -- held on the CPU by tests/test_row_forms_cpu.py -- and the references).

  a. forward and every parameter gradient of every run against torch autograd over the oracle in FLOAT64, under the project's
     bounds (1e-4 of max(1, largest entry); 2e-4 of the gradient's largest entry) and a regression-level bound beside each:
     max(REG_F32 | REG_GRAD, 8 x the deviation of the same oracle evaluated in float32 on the CPU), the yardstick being the
     reference at the kernel's precision, never the kernel.  The state predictor with detach False and True.
  b. the forms against each other: one child process per environment (RGL_HEAD_ROWS_DIRECT is read once), started once per
     session; the tile forms within 5e-5 of the per-scene kernel, two runs of one form bit-identical.
  c. runs the pipeline cannot take ("not mine": a job without waves) are loud or correct, never wrong, and leave nothing behind.
  d. the whole module once more with poisoned workspaces.

A child that fails -- by an assertion, a signal, an abort or its time limit -- fails every test that needs it with its output; it is
not started again.  profiles/mlp_row_forms.txt holds the parity-report lines of a run of this module.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from relationalgraphlearning_amd import _native as nat
from tests import row_forms as rf
from tests.test_gpu_parity import REG_F32, REG_GRAD, TOL, report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 2e-4                     # test_gpu_parity._grad_close
FORMS_TOL = 5e-5                    # test_mfma_backward_at_size: the tile pipeline against the per-scene kernel

TILES = {"RGL_BACKWARD_MFMA": "2", "RGL_TILES_FORWARD": "2"}
ENVS = {
    "direct": dict(TILES),
    "staged": dict(TILES, RGL_HEAD_ROWS_DIRECT="0"),
    "scene": {"RGL_BACKWARD_MFMA": "0", "RGL_TILES_FORWARD": "0"},      # the per-scene kernels
}
VALID = "V1-37"                     # the call that must still be right after a refusal


def refused(run, env):
    """By the table (held against the planner on the CPU): the tile pipeline does not take the run in this environment."""
    return env != "scene" and any(e[0 if env == "direct" else 1] == "waves0" for e in run.jobs.values())


def forms(run, env):
    if env == "scene":
        return "per-scene kernel"
    return ", ".join("%s %s" % (job, e[0 if env == "direct" else 1]) for job, e in run.jobs.items())


# ---------------------------------------------------------------------------------------------------------------------------
# the child processes
# ---------------------------------------------------------------------------------------------------------------------------
def measure(run, dev, detach=False):
    """Forward and backward of a run on the device, twice: {"out", "g/<parameter>", "repeat_ok", "graph_absent"}."""
    mod, g, head = rf.build(run)
    mod.to(dev)
    robot, humans = rf.scenes(run)
    r, h, up = robot.unsqueeze(1).to(dev), humans.to(dev), rf.upstream(run).to(dev)

    def once():
        for p_ in mod.parameters():
            p_.grad = None
        out = mod((r, h)) if run.module != "motion" else mod((r, h), None, detach=detach)[1]     # "rgl": the graph model alone
        (out * up).sum().backward()
        res = {"out": out.detach().cpu().numpy()}
        absent = True
        for k, v in g.named_parameters():
            if detach:
                absent = absent and (v.grad is None or float(v.grad.abs().max()) == 0.0)
            else:
                res["g/graph." + k] = v.grad.detach().cpu().numpy()
        for k, v in (head.named_parameters() if head is not None else ()):
            res["g/%s.%s" % (run.module, k)] = v.grad.detach().cpu().numpy()
        res["graph_absent"] = np.array(absent and detach)
        return res
    first, again = once(), once()
    first["repeat_ok"] = np.array(all(np.array_equal(first[k], again[k]) for k in first))
    return first


def forward_only(run, dev):
    mod, _, _ = rf.build(run)
    mod.to(dev)
    robot, humans = rf.scenes(run)
    with torch.no_grad():
        out = mod((robot.unsqueeze(1).to(dev), humans.to(dev))) if run.module == "value" else \
            mod((robot.unsqueeze(1).to(dev), humans.to(dev)), None)[1]
    return out.cpu().numpy()


def attempt(res, prefix, fn):
    """fn()'s arrays under `prefix`, or the library's refusal as `prefix`/error."""
    try:
        got = fn()
        for k, v in (got.items() if isinstance(got, dict) else [("out", got)]):
            res["%s/%s" % (prefix, k)] = v
    except nat.NativeLibraryError as e:
        res[prefix + "/error"] = np.array(str(e))


def child_main(name, out):
    """Entry point of the child of environment `name`: every run the environment takes; for the runs it refuses, section c."""
    dev = torch.device("cuda:0")
    res = {}
    for run in rf.RUNS:
        assert rf.not_mine(run) == refused(run, name) or name == "scene", run.id
        if refused(run, name):
            continue
        for detach in ((False, True) if run.module == "motion" else (False,)):
            prefix = run.id + ("/detach" if detach else "")
            if name == "scene":
                attempt(res, prefix, lambda: measure(run, dev, detach))       # a scene may not fit the per-scene kernel
            else:
                for k, v in measure(run, dev, detach).items():
                    res["%s/%s" % (prefix, k)] = v
        print("done", run.id, flush=True)
    valid = rf.RUN[VALID]
    for run in [r for r in rf.RUNS if refused(r, name)]:
        pre = "refused/%s/" % run.id
        # backward: must-run mode raises; mode 1 hands the scene to the per-scene kernel (or raises that kernel's own error)
        os.environ["RGL_BACKWARD_MFMA"] = "2"
        attempt(res, pre + "mfma2", lambda: measure(run, dev))
        attempt(res, pre + "after_mfma2", lambda: measure(valid, dev))
        os.environ["RGL_BACKWARD_MFMA"] = "1"
        attempt(res, pre + "mfma1", lambda: measure(run, dev))
        attempt(res, pre + "after_mfma1", lambda: measure(valid, dev))
        os.environ["RGL_BACKWARD_MFMA"] = ENVS[name]["RGL_BACKWARD_MFMA"]
        # forward: with the general kernel refused, and by default
        os.environ["RGL_REQUIRE_MFMA_FORWARD"] = "1"
        attempt(res, pre + "forward_required", lambda: forward_only(run, dev))
        attempt(res, pre + "after_forward_required", lambda: forward_only(valid, dev))
        del os.environ["RGL_REQUIRE_MFMA_FORWARD"]
        attempt(res, pre + "forward_default", lambda: forward_only(run, dev))
        print("done refusals of", run.id, flush=True)
    torch.cuda.synchronize()
    np.savez(out, **res)
    print("OK")


_children = {}


def child(name, tmp_path_factory):
    """The arrays of environment `name`'s child, started ONCE per session, one child at a time; a failure is kept and raised again."""
    if name not in _children:
        out = str(tmp_path_factory.mktemp("row_forms") / (name + ".npz"))
        code = "import sys\nfrom tests.test_row_forms import child_main\nchild_main(sys.argv[1], sys.argv[2])\n"
        env = {k: v for k, v in os.environ.items() if k not in ("RGL_HEAD_ROWS_DIRECT", "RGL_REQUIRE_MFMA_FORWARD")}
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


# ---------------------------------------------------------------------------------------------------------------------------
# a. against float64
# ---------------------------------------------------------------------------------------------------------------------------
def against_float64(got, prefix, run, detach, tag, table="rows", what="mlp row forms"):
    """Section a for the arrays under `prefix`; returns (forward deviation, worst gradient deviation).  `table`, `what`: the case
    table the run is of and the parity report's heading (tests/test_graph_forms.py runs its own table through here)."""
    ref = rf.reference(run.id, detach, table)
    assert ref["masks_agree"] and ref["n_masks"] > 0, (run.id, "the float32 and float64 oracles differ in a ReLU mask: a wrong seed")
    assert ref["margin"] >= 8, (run.id, "a pre-activation within 8 float32 errors of zero: a wrong seed", ref["margin"])
    names = sorted(k[len(prefix) + 3:] for k in got if k.startswith(prefix + "/g/"))
    assert names == sorted(ref["grads"]), (tag, names, sorted(ref["grads"]))            # no parameter is left out
    reg_f, reg_g = max(REG_F32, 8 * ref["yard_fwd"]), max(REG_GRAD, 8 * ref["yard_grad"])
    out = got[prefix + "/out"]
    assert out.shape == ref["out"].shape and out.dtype == np.float32
    e_f = rf.forward_error(out, ref["out"])
    errs = {k: rf.grad_error(got["%s/g/%s" % (prefix, k)], ref["grads"][k]) for k in names}
    worst = max(errs, key=errs.get)
    print("%s: forward %.2e (float32 oracle %.2e, bounds %.0e and %.2e); gradients %.2e at %s (float32 oracle %.2e, bounds %.0e and %.2e)"
          % (tag, e_f, ref["yard_fwd"], TOL, reg_f, errs[worst], worst, ref["yard_grad"], GRAD_TOL, reg_g))
    assert np.isfinite(out).all() and all(np.isfinite(got["%s/g/%s" % (prefix, k)]).all() for k in names), tag
    assert e_f <= TOL, (tag, e_f)
    assert e_f <= reg_f, ("regression-level bound", tag, e_f, reg_f)
    for k in names:
        assert got["%s/g/%s" % (prefix, k)].shape == ref["grads"][k].shape, (tag, k)
        assert errs[k] <= GRAD_TOL, (tag, k, errs[k])
        assert errs[k] <= reg_g, ("regression-level bound", tag, k, errs[k], reg_g)
    report("%s, %s: forward %.2e of the float64 oracle (float32 oracle on the CPU %.2e; asserted %.0e and %.2e), gradients %.2e "
           "at %s (float32 oracle %.2e; asserted %.0e and %.2e)"
           % (what, tag, e_f, ref["yard_fwd"], TOL, reg_f, errs[worst], worst, ref["yard_grad"], GRAD_TOL, reg_g))
    return e_f, errs[worst]


CASES_A = [(env, run.id) for env in ENVS for run in rf.RUNS if not refused(run, env)]


@pytest.mark.parametrize("env,run_id", CASES_A, ids=["%s-%s" % c for c in CASES_A])
def test_forward_and_gradients_against_float64(env, run_id, tmp_path_factory):
    run = rf.RUN[run_id]
    got = child(env, tmp_path_factory)
    tag = "%s S=%d H=%d under %s (%s)" % (run.id, run.S, run.H, env, forms(run, env))
    if run.id + "/error" in got:            # only the per-scene kernel may decline, and only for a scene that does not fit one CU
        assert env == "scene" and "RGL_ERR_LDS" in str(got[run.id + "/error"]), (tag, got[run.id + "/error"])
        assert run.H >= 49, tag
        report("mlp row forms, %s: the per-scene kernel cannot hold the scene (RGL_ERR_LDS)" % tag)
        return
    against_float64(got, run.id, run, False, tag)
    assert bool(got[run.id + "/repeat_ok"]), (tag, "two runs differ")
    if run.module == "motion":
        pre = run.id + "/detach"
        against_float64(got, pre, run, True, tag + ", detached")
        assert bool(got[pre + "/graph_absent"]), (tag, "a detached graph model received a gradient")
        assert bool(got[pre + "/repeat_ok"]), (tag, "two detached runs differ")
        heads = [k for k in got if k.startswith(pre + "/g/")]
        assert heads and all(k.startswith(pre + "/g/motion.") for k in heads)
        for k in heads:                     # the motion head's gradients do not depend on what happens behind it
            assert np.array_equal(got[k], got[run.id + k[len(pre):]]), (tag, k)
        assert np.array_equal(got[pre + "/out"], got[run.id + "/out"]), tag


# ---------------------------------------------------------------------------------------------------------------------------
# b. the forms against each other
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_id", [r.id for r in rf.RUNS])
def test_tile_forms_agree_with_the_per_scene_kernel(run_id, tmp_path_factory):
    run = rf.RUN[run_id]
    base = child("scene", tmp_path_factory)
    tiles = [env for env in ("direct", "staged") if not refused(run, env)]
    if run.id + "/error" in base:
        assert run.H >= 49 and "RGL_ERR_LDS" in str(base[run.id + "/error"]) and len(tiles) == 2     # then the tile forms are all there is
        base = child("direct", tmp_path_factory)
    worst = 0.0
    for env in tiles:
        got = child(env, tmp_path_factory)
        keys = sorted(k for k in got if k.startswith(run.id + "/") and ("/g/" in k or k.endswith("/out")))
        assert keys and keys == sorted(k for k in base if k.startswith(run.id + "/") and ("/g/" in k or k.endswith("/out")))
        for k in keys:
            err = rf.grad_error(got[k], base[k].astype(np.float64)) if "/g/" in k else rf.forward_error(got[k], base[k].astype(np.float64))
            assert err <= FORMS_TOL, (run.id, env, k, err)
            worst = max(worst, err)
        assert bool(got[run.id + "/repeat_ok"]), (run.id, env)
    report("mlp row forms, %s: %s within %.1e of the per-scene kernel (asserted %.0e), each bit-identical between two runs"
           % (run.id, " and ".join("%s (%s)" % (e, forms(run, e)) for e in tiles) or "no tile form", worst, FORMS_TOL))


# ---------------------------------------------------------------------------------------------------------------------------
# c. "not mine" is loud or correct, never wrong
# ---------------------------------------------------------------------------------------------------------------------------
CASES_C = [(env, run.id) for env in ("direct", "staged") for run in rf.RUNS if refused(run, env)]


@pytest.mark.parametrize("env,run_id", CASES_C, ids=["%s-%s" % c for c in CASES_C])
def test_not_mine_is_loud_or_correct(env, run_id, tmp_path_factory):
    run, valid = rf.RUN[run_id], rf.RUN[VALID]
    got = child(env, tmp_path_factory)
    pre = "refused/%s/" % run.id
    tag = "%s under %s (%s)" % (run.id, env, forms(run, env))
    # RGL_BACKWARD_MFMA=2: the backward raises, and the next valid call is right
    assert "RGL_ERR_BAD_MODE" in str(got.get(pre + "mfma2/error")) and "rgl_graph_backward_f32" in str(got[pre + "mfma2/error"]), tag
    against_float64(got, pre + "after_mfma2", valid, False, "%s after the refusal of %s" % (valid.id, tag))
    # RGL_BACKWARD_MFMA=1: the per-scene kernel's gradients, or its own error
    if pre + "mfma1/error" in got:
        assert "RGL_ERR_LDS" in str(got[pre + "mfma1/error"]), (tag, got[pre + "mfma1/error"])
        how = "raises the per-scene kernel's RGL_ERR_LDS"
    else:
        against_float64(got, pre + "mfma1", run, False, tag + ", RGL_BACKWARD_MFMA=1")
        how = "is computed by the per-scene kernel"
    against_float64(got, pre + "after_mfma1", valid, False, "%s after RGL_BACKWARD_MFMA=1 on %s" % (valid.id, tag))
    # the forward: refused or right with the general kernel forbidden, right by default
    ref = rf.reference(run.id)
    fwd = []
    for mode in ("forward_required", "forward_default"):
        if pre + mode + "/error" in got:
            assert mode == "forward_required" and "RGL_ERR_BAD_MODE" in str(got[pre + mode + "/error"]), (tag, mode, got[pre + mode + "/error"])
            fwd.append("refused")
        else:
            e_f = rf.forward_error(got[pre + mode + "/out"], ref["out"])
            assert e_f <= TOL and e_f <= max(REG_F32, 8 * ref["yard_fwd"]), (tag, mode, e_f)
            fwd.append("%.2e" % e_f)
    e_v = rf.forward_error(got[pre + "after_forward_required/out"], rf.reference(valid.id)["out"])
    assert e_v <= TOL and e_v <= max(REG_F32, 8 * rf.reference(valid.id)["yard_fwd"]), (tag, e_v)
    report("mlp row forms, %s: RGL_BACKWARD_MFMA=2 raises, =1 %s; forward with RGL_REQUIRE_MFMA_FORWARD=1 %s, by default %s; the "
           "valid calls that follow are right" % (tag, how, fwd[0], fwd[1]))


# ---------------------------------------------------------------------------------------------------------------------------
# d. poisoned workspaces
# ---------------------------------------------------------------------------------------------------------------------------
def test_whole_module_with_poisoned_workspaces():
    """Every test above once more with workspaces and outputs filled with NaN patterns before the kernels run: every padded column a
    product reads and every slab element a wave's later tiles add to was written first."""
    if nat.poison_workspaces():
        return                              # this IS the poisoned run
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_row_forms.py"), "-q", "-m", "gpu", "-x",
                          "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, RGL_DEBUG_POISON_WORKSPACES="1"),
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and " passed" in res.stdout, res.stdout[-6000:] + res.stderr[-2000:]
    report("mlp row forms with poisoned workspaces: " + res.stdout.strip().splitlines()[-1].strip("= "))
