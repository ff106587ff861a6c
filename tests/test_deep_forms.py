"""children_deep_kernel<NT, F16, SKIP, SOFT, T4> of csrc/rgl_deep.hip in every form it launches (tests/deep_forms.py: the runs, the
form each takes by the library's own planner -- held on the CPU by tests/test_deep_forms_cpu.py -- and the references).  The
harness is tests/test_graph_forms.py's.

Every run goes through TreeSearch.value_children.  By the planner, that stand-alone call has the packed value-estimator image at
hand in the f32 and f16 modes (the Python layer packs it for every shape this kernel serves), so it IS the call that runs stage 2
inside the launch: no run needs expand or predict_batch to reach that form.  Stage 2 runs outside -- robot_head_kernel -- in the
bf16x6 runs (that image is the fused kernel's) and in the environment RGL_DEEP_FUSE_HEAD=0.  Each child records its own planner's
answers beside its outputs, and the tests hold the path each form took against them.

  a. every run in every environment against reference64, relative to max(1, max|want|): f32 forms under TOL and max(REG_F32, 8 x the
     float32 oracle's deviation); f16 forms under F16_TOL and REG_F16, and not bit-identical to the f32 form; the bf16x6 mode (the f32
     form with stage 2 outside) under the f32 bounds; raw random-init weights under the north-star bound only; two calls bit-identical.
  b. the three deep environments differ in bits from the tile-kernel environment and agree with it within twice the bounds of a.
  c. T4 on and off agree within the bounds of a, differ in bits where the planner chose T4 and are bit-identical where it did not;
     stage 2 inside and outside the launch are bit-identical: head_rows_and_tail is the body of robot_head_kernel too, both read the
     same packed fragments, and a child's value is one column of its 16-row MFMA tile whichever rows share the tile.
  d. walking runs: the value of parent p in the launch of 300 (257) parents equals, bit for bit, that of a launch of p alone.
  e. beyond each LDS limit another MFMA kernel answers correctly; f16 there and at two layers raises; the next covered run is right.
  f. the whole module once more with poisoned workspaces.

One child process per environment, started once per session, each under its own time limit; a child that fails -- by an assertion, a
signal, an abort or its time limit -- fails every test that needs it and is not started again.  profiles/deep_kernel_forms.txt
holds the parity-report lines of a run of this module.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import relationalgraphlearning_amd as rga
from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd.config import policy_config
from tests import deep_forms as df
from tests import golden_io as gio
from tests.test_gpu_parity import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHAT = "deep kernel forms"
ENVS = {
    "default": {},
    "t4off": {"RGL_DEEP_T4": "0"},
    "nofuse": {"RGL_DEEP_FUSE_HEAD": "0"},
    "tile": {"RGL_CHILDREN_TILE_KERNEL": "1"},          # the tile kernel (plain-weight similarities: the one-wave-per-child kernel)
}
DEEP_ENVS = ("default", "t4off", "nofuse")
# switches read once per process that would change which kernel a child runs
STRIPPED = ("RGL_DEEP_T4", "RGL_DEEP_FUSE_HEAD", "RGL_CHILDREN_TILE_KERNEL", "RGL_FORCE_GENERIC", "RGL_CONTRACT_F32_AS", "RGL_FUSED",
            "RGL_FUSED_MIN_TILES")
PLAN_FIELDS = ("covered", "t4", "fuse_head", "grid", "parents_per_wg", "f16")
CHILD_TIMEOUT = 120                 # measured: 3 to 4 s per child, 31 s for the module with its poisoned rerun


# ---------------------------------------------------------------------------------------------------------------------------
# the child processes
# ---------------------------------------------------------------------------------------------------------------------------
_policies = {}


def policy(run, dev):
    key = (run.L, run.sim, run.skip, run.flavour, run.speeds, run.rots)
    if key not in _policies:
        cfg = policy_config("model_predictive_rl", gcn__num_layer=run.L, gcn__similarity_function=run.sim, gcn__skip_connection=run.skip,
                            action_space__speed_samples=run.speeds, action_space__rotation_samples=run.rots)
        pol = rga.ModelPredictiveRL()
        pol.time_step = 0.25
        pol.configure(cfg)
        pol.load_state_dict(gio.checkpoint(run.flavour, run.L, "separate", run.sim))
        pol.set_time_step(0.25)
        pol.set_phase("test")
        pol.set_device(dev)
        pol.build_action_space(1.0)
        _policies[key] = pol
    return _policies[key]


def attempt(res, prefix, fn):
    """fn()'s array under `prefix`, or the library's refusal as `prefix`/error."""
    try:
        res[prefix] = fn()
    except nat.NativeLibraryError as e:
        res[prefix + "/error"] = np.array(str(e))


def measure(run, dev, env, res):
    """The run's children valued twice (and, for an f16 run, once by the f32 form; for a walking run, the sampled parents alone)."""
    pol = policy(run, dev)
    cr, humans = (t.to(dev) for t in df.inputs(run.id))

    def call(dt, c=cr, h=humans):
        pol.contraction_dtype = dt
        ts = pol.tree_search()
        assert ts.num_actions == df.num_actions(run), run.id
        return ts.value_children(c, h).cpu().numpy()
    # the tile kernel has no f16 form: the second opinion on an f16 run is its f32 value
    dt = "f32" if env == "tile" and run.contraction == "f16" and run.expect == "deep" else run.contraction
    pol.contraction_dtype = dt
    p = df.plan(run._replace(contraction=dt))              # this process's planner, under this process's switches
    res[run.id + "/plan"] = np.array([p[k] for k in PLAN_FIELDS])
    res[run.id + "/image"] = np.array(pol.tree_search().planner(dev).children_image is not None)
    attempt(res, run.id + "/out", lambda: call(dt))
    if run.id + "/out" not in res:
        return
    res[run.id + "/repeat_ok"] = np.array(np.array_equal(res[run.id + "/out"], call(dt)))
    if dt == "f16":
        res[run.id + "/out_f32"] = call("f32")
    if run.kind == "walk" and env != "tile":
        res[run.id + "/solo"] = np.stack([call(dt, cr[q:q + 1], humans[q:q + 1])[0] for q in df.walk_sample(run.P)])


def child_main(name, out):
    """Entry point of the child of environment `name`: every run; after each run beyond a limit, the valid run once more."""
    dev = torch.device("cuda:0")
    res = {}
    for run in df.RUNS:
        measure(run, dev, name, res)
        if run.kind == "beyond":
            after = {}
            measure(df.RUN[df.VALID], dev, name, after)
            res[run.id + "/after"] = after[df.VALID + "/out"]
        print("done", run.id, flush=True)
    torch.cuda.synchronize()
    np.savez(out, **res)
    print("OK")


_children = {}


def child(name, tmp_path_factory):
    """The arrays of environment `name`'s child, started ONCE per session, one child at a time; a failure is kept and raised again."""
    if name not in _children:
        out = str(tmp_path_factory.mktemp("deep_forms") / (name + ".npz"))
        code = "import sys\nfrom tests.test_deep_forms import child_main\nchild_main(sys.argv[1], sys.argv[2])\n"
        env = {k: v for k, v in os.environ.items() if k not in STRIPPED}
        env.update(ENVS[name], RGL_REQUIRE_MFMA_CHILDREN="1")
        try:
            res = subprocess.run([sys.executable, "-c", code, name, out], cwd=ROOT, env=env, capture_output=True, text=True,
                                 timeout=CHILD_TIMEOUT)
            if res.returncode != 0 or "OK" not in res.stdout:
                raise AssertionError("child ended with %s\n%s" % (res.returncode, res.stdout[-2000:] + res.stderr[-4000:]))
            _children[name] = dict(np.load(out))
        except Exception as e:              # also the time limit: remembered, not retried
            _children[name] = e
    if isinstance(_children[name], Exception):
        raise AssertionError("the child process of environment %s failed (started once): %s" % (name, _children[name]))
    return _children[name]


def child_plan(got, run):
    return dict(zip(PLAN_FIELDS, (int(v) for v in got[run.id + "/plan"])))


def held(tag, out, run, f16):
    """`out` against reference64 under the bounds of the form that computed it; returns (error, float32 yardstick, tol, reg)."""
    want = df.reference64(run.id)
    tol, reg = df.bounds(run._replace(contraction="f16" if f16 else "f32"))
    assert out.shape == want.shape and out.dtype == np.float32 and np.isfinite(out).all(), tag
    err, yard = df.error(out, want), df.yardstick(run)
    print("%s: %.2e of float64 (float32 oracle on the CPU %.2e; bounds %.0e and %s)" % (tag, err, yard, tol, "%.2e" % reg if reg else "none"))
    assert err <= tol, (tag, err, tol)
    if reg is not None:
        assert err <= reg, ("regression-level bound", tag, err, reg, "float32 oracle", yard)
    return err, yard, tol, reg


# ---------------------------------------------------------------------------------------------------------------------------
# a. against float64
# ---------------------------------------------------------------------------------------------------------------------------
ANSWERED = [r for r in df.RUNS if r.expect != "error"]
CASES_A = [(env, run.id) for env in ENVS for run in ANSWERED]
WORST = {}


@pytest.mark.parametrize("env,run_id", CASES_A, ids=["%s-%s" % c for c in CASES_A])
def test_values_against_float64(env, run_id, tmp_path_factory):
    run = df.RUN[run_id]
    got = child(env, tmp_path_factory)
    assert run.id + "/out" in got, (env, run.id, got.get(run.id + "/out/error"))
    p = child_plan(got, run)
    deep = env != "tile" and run.expect == "deep"
    f16 = deep and run.contraction == "f16"
    # the path the form took, by the child's own planner: the deep kernel (with T4, stage 2 inside as the environment says) or not
    assert p["covered"] == int(deep) and p["f16"] == int(f16), (env, run.id, p)
    if run.contraction != "bf16x6":         # (a two-layer bf16x6 planner carries the fused kernel's image, which this call does not take)
        assert bool(got[run.id + "/image"]) and df.has_image(run), (env, run.id, "the stand-alone call has no image at hand")
    if deep:
        here = df.plan(run)
        assert p["fuse_head"] == (here["fuse_head"] if env != "nofuse" else 0) and p["t4"] == (here["t4"] if env != "t4off" else 0), (env, p, here)
    tag = "%s, %s under %s (%s)" % (WHAT, run.id, env, df.form(run, df.plan(run, p["fuse_head"] == 1)) if deep else "not the deep kernel")
    err, yard, tol, reg = held(tag, got[run.id + "/out"], run, f16)
    assert bool(got[run.id + "/repeat_ok"]), (tag, "two calls differ")
    if f16:
        assert not np.array_equal(got[run.id + "/out"], got[run.id + "/out_f32"]), (tag, "bit-identical to the f32 form: the f16 form did not run")
        held(tag + ", its f32 form", got[run.id + "/out_f32"], run, False)
        # what the f16 inputs cost is rounding, not a defect: the float64 restatement that rounds the same operands explains the
        # kernel's deviation to within an f32 form's bound -- or half of that cost: the kernel rounds f32 values where the restatement
        # rounds float64 ones, and an operand that falls the other way moves by a whole f16 ulp, twice what its rounding contributes
        # to the cost, which is the sum of 64 N + N^2 such contributions and more (largest at N = 2: a fifth of the cost)
        cost, off = df.error(df.reference_f16(run.id), df.reference64(run.id)), df.error(got[run.id + "/out"], df.reference_f16(run.id))
        print("%s: f16 operands cost %.2e in float64; the kernel is %.2e from that restatement" % (tag, cost, off))
        assert off <= max(df.bounds(run._replace(contraction="f32"))[1], cost / 2), (tag, "beyond the rounding of its f16 operands", off, cost)
        tag += "; f16 operands cost %.2e in a float64 restatement, from which the kernel is %.2e" % (cost, off)
    fam = ("f16" if f16 else df.family(run._replace(contraction="f32"))) + (" rand" if run.flavour == "rand" else "")
    w = WORST.setdefault((env, fam), [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], err), max(w[1], yard), w[2] + 1
    report("%s: %.2e of the float64 oracle (float32 oracle on the CPU %.2e; asserted %.0e and %s)"
           % (tag, err, yard, tol, "%.2e" % reg if reg else "the north-star bound only"))


def test_worst_deviation_per_family():
    """The report's summary: per environment and family the worst deviation from float64 next to the float32 oracle's."""
    assert WORST, "section a did not run"
    for (env, fam), (err, yard, n) in sorted(WORST.items()):
        report("%s, worst over %d runs under %s, %s: %.2e of the float64 oracle (float32 oracle on the CPU: %.2e)" % (WHAT, n, env, fam, err, yard))


# ---------------------------------------------------------------------------------------------------------------------------
# b. proof of run and cross-check against the tile kernel;  c. the environments against each other
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_id", [r.id for r in df.COVERED])
def test_deep_kernel_against_the_tile_kernel_and_its_own_forms(run_id, tmp_path_factory):
    run = df.RUN[run_id]
    base = child("tile", tmp_path_factory)[run.id + "/out"].astype(np.float64)
    outs = {env: child(env, tmp_path_factory)[run.id + "/out"] for env in DEEP_ENVS}
    tol, reg = df.bounds(run)
    worst = 0.0
    for env, out in outs.items():
        assert not np.array_equal(out.astype(np.float64), base), (run.id, env, "bit-identical to the tile kernel's values")
        err = df.error(out, base)
        assert err <= 2 * tol and (reg is None or err <= 2 * reg), (run.id, env, err, tol, reg)
        worst = max(worst, err)
    # T4 on and off
    t4 = bool(df.plan(run)["t4"])
    err = df.error(outs["t4off"], outs["default"].astype(np.float64))
    assert err <= tol and (reg is None or err <= reg), (run.id, "T4 on / off", err)
    assert np.array_equal(outs["t4off"], outs["default"]) == (not t4), (run.id, "T4 chosen" if t4 else "T4 not chosen")
    # stage 2 inside and outside the launch
    assert np.array_equal(outs["nofuse"], outs["default"]), (run.id, "stage 2 inside / outside the launch")
    report("%s, %s: within %.2e of the tile-kernel environment (asserted %s), never bit-identical to it; RGL_DEEP_T4=0 %s; "
           "RGL_DEEP_FUSE_HEAD=0 bit-identical" % (WHAT, run.id, worst, "%.2e" % (2 * (reg or tol)), "differs in bits, within %.2e" % err if t4 else "bit-identical"))


# ---------------------------------------------------------------------------------------------------------------------------
# d. walking runs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", DEEP_ENVS)
@pytest.mark.parametrize("run_id", [r.id for r in df.WALK])
def test_a_walked_parent_equals_the_parent_alone(run_id, env, tmp_path_factory):
    run, got = df.RUN[run_id], child(env, tmp_path_factory)
    sample = df.walk_sample(run.P)
    p = child_plan(got, run)
    assert (p["parents_per_wg"] >= 2 and p["grid"] * p["parents_per_wg"] >= run.P > p["grid"]) if p["fuse_head"] else p["grid"] < run.P, p
    together, alone = got[run.id + "/out"][sample], got[run.id + "/solo"]
    assert alone.shape == together.shape and len(sample) >= 32
    differ = [q for q, a, b in zip(sample, together, alone) if not np.array_equal(a, b)]
    assert not differ, (run.id, env, "parents whose values depend on the launch they are in", differ)
    report("%s, %s under %s (%s): %d sampled parents bit-identical to launches of their own"
           % (WHAT, run.id, env, df.form(run, df.plan(run, p["fuse_head"] == 1)), len(sample)))


# ---------------------------------------------------------------------------------------------------------------------------
# e. refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("run_id", [r.id for r in df.BEYOND])
def test_beyond_the_limits(run_id, env, tmp_path_factory):
    run, valid, got = df.RUN[run_id], df.RUN[df.VALID], child(env, tmp_path_factory)
    assert child_plan(got, run)["covered"] == 0, run.id
    if run.expect == "error":
        err = str(got.get(run.id + "/out/error"))
        assert run.id + "/out" not in got and "RGL_ERR_BAD_MODE" in err and "mprl_value_children_f32" in err, (run.id, env, err)
        what = "raises RGL_ERR_BAD_MODE"
    else:
        assert run.id + "/out" in got, (run.id, env, got.get(run.id + "/out/error"))            # held to the bounds in section a
        what = "another MFMA kernel answers"
    after = got[run.id + "/after"]
    held("%s after %s under %s" % (valid.id, run.id, env), after, valid, False)
    assert np.array_equal(after, got[valid.id + "/out"]), (run.id, env, "the valid run changed after the refusal")
    report("%s, %s under %s: %s; %s right after it is bit-identical to its first run" % (WHAT, run.id, env, what, valid.id))


# ---------------------------------------------------------------------------------------------------------------------------
# f. poisoned workspaces
# ---------------------------------------------------------------------------------------------------------------------------
def test_whole_module_with_poisoned_workspaces():
    """Every test above once more with workspaces and outputs filled with NaN patterns before the kernels run: the rows stage 2 reads
    were written by stage 1 of the same parents, whichever workgroup owns them."""
    if nat.poison_workspaces():
        return                              # this IS the poisoned run
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_deep_forms.py"), "-q", "-m", "gpu", "-x",
                          "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, RGL_DEBUG_POISON_WORKSPACES="1"),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and " passed" in res.stdout, res.stdout[-6000:] + res.stderr[-2000:]
    report("%s with poisoned workspaces: %s" % (WHAT, res.stdout.strip().splitlines()[-1].strip("= ")))
