"""The two-stage pair -- children_rank1_kernel<HR, NT, SKIP, SOFT> of csrc/rgl_rank1.hip, then robot_head_kernel<32,100,100>,
robot_head_kernel<150,100,100> or robot_head_any_kernel of csrc/rgl_head.hip -- in every form it launches (tests/two_stage_forms.py:
the runs, the form each takes by the library's own planner -- held on the CPU by tests/test_two_stage_forms_cpu.py -- and the
references).  The harness is tests/test_deep_forms.py's.

Every run goes through TreeSearch.value_children, in three environments: `default`, `twostage` (RGL_CHILDREN_TWO_STAGE=1: the
shipped head's pair at every size) and `tile` (RGL_CHILDREN_TILE_KERNEL=1: the tile kernel, or the one-wave-per-child kernel for
the plain-weight similarities -- never the pair).  Each child records its own planner's answers beside its outputs, and the tests
hold the form each run took against the CPU table.

  a. every run in `default` and `twostage` against reference64, relative to max(1, max|want|): under TOL and max(REG_F32, 8 x the
     float32 oracle's deviation on the same inputs); raw random-init weights under the north-star bound only; two calls bit-identical.
  b. where an environment runs the pair, its values differ in bits from the `tile` environment's and agree within twice the bounds of a.
  c. walking and striding runs: the values of sampled parents equal, bit for bit, those of a launch of that parent alone.  Stage 1
     computes a parent from its own rows and crowd whichever workgroup walks it and whichever half of the double buffer holds the
     crowd block; in stage 2 a child's value is one column of its 16-row MFMA tile, whichever rows share the tile and whichever
     wave walks it.  The code gives no reason for different bits, and none is allowed.
  d. with and without the packed image: a bf16x6-mode run (stage 1 gathers its weights matrix by matrix, Wa = I built for gaussian;
     stage 2 builds its fragments from the raw matrices) against the f32-mode run of the same shape and weights (both copy the packed
     image).  The image holds the same f32 matrices, padded with the same zeros, and fragments of the same f32 elements
     (pack_images_kernel rounds nothing in the f32 layout), so the two are asked to be bit-identical.
  e. beyond the envelope (33 nodes, 97 children, three layers, a layerwise graph) another kernel answers within the bounds of a, and
     the next covered run is right and unchanged.
  f. the whole module once more with poisoned workspaces.

The tail of robot_head_kernel (select, back-up chain, root decision) is tests/test_search_bookkeeping.py's, bit for bit.

One child process per environment, started once per session, each under its own time limit; a child that fails -- by an assertion, a
signal, an abort or its time limit -- fails every test that needs it and is not started again.  profiles/two_stage_forms.txt
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
from tests import two_stage_forms as ts
from tests.test_gpu_parity import report

pytestmark = pytest.mark.gpu
ROOT = ts.ROOT
WHAT = "two-stage pair forms"
ENVS = ts.ENVS
PLAN_FIELDS = ("pair", "hr", "node_tiles", "child_tiles", "norm", "skip", "image", "grid", "parents_per_wg", "head_variant", "head_grid",
               "head_tiles", "head_tiles_per_wave", "family")
CHILD_TIMEOUT = 120                 # measured: 2.7 s per child, 26 s for the module with its poisoned rerun


# ---------------------------------------------------------------------------------------------------------------------------
# the child processes
# ---------------------------------------------------------------------------------------------------------------------------
_policies = {}


def policy(run, dev):
    key = (run.L, run.sim, run.skip, run.flavour, run.speeds, run.rots, run.head, run.layerwise)
    if key not in _policies:
        more = {} if run.head == "ship" else {"model_predictive_rl__value_network_dims": list(ts.HEADS[run.head])}
        cfg = policy_config("model_predictive_rl", gcn__num_layer=run.L, gcn__similarity_function=run.sim, gcn__skip_connection=run.skip,
                            gcn__layerwise_graph=run.layerwise, action_space__speed_samples=run.speeds,
                            action_space__rotation_samples=run.rots, **more)
        pol = rga.ModelPredictiveRL()
        pol.time_step = 0.25
        pol.configure(cfg)
        pol.load_state_dict(ts.checkpoint(run))
        pol.set_time_step(0.25)
        pol.set_phase("test")
        pol.set_device(dev)
        pol.build_action_space(1.0)
        _policies[key] = pol
    return _policies[key]


def measure(run, dev, res):
    """The run's children valued twice (a bf16x6 run: once more in the f32 mode; a walking or striding run: the sampled parents alone)."""
    pol = policy(run, dev)
    cr, humans = (t.to(dev) for t in ts.inputs(run.id))

    def call(dt, c=cr, h=humans):
        pol.contraction_dtype = dt
        search = pol.tree_search()
        assert search.num_actions == ts.num_actions(run), run.id
        return search.value_children(c, h).cpu().numpy()
    pol.contraction_dtype = run.contraction
    p = ts.plan(run)                                        # this process's planner, under this process's switches
    res[run.id + "/plan"] = np.array([p[k] for k in PLAN_FIELDS])
    res[run.id + "/image"] = np.array(pol.tree_search().planner(dev).children_image is not None)
    res[run.id + "/out"] = call(run.contraction)
    res[run.id + "/repeat_ok"] = np.array(np.array_equal(res[run.id + "/out"], call(run.contraction)))
    if run.contraction == "bf16x6":
        q = ts.plan(run._replace(contraction="f32"))
        res[run.id + "/plan_f32"] = np.array([q[k] for k in PLAN_FIELDS])
        res[run.id + "/out_f32"] = call("f32")
    if run.kind in ("walk", "stride"):
        res[run.id + "/solo"] = np.stack([call(run.contraction, cr[q:q + 1], humans[q:q + 1])[0] for q in ts.walk_sample(run.P)])


def child_main(name, out):
    """Entry point of the child of environment `name`: every run; after each run beyond the envelope, the valid run once more."""
    dev = torch.device("cuda:0")
    res = {}
    for run in ts.RUNS:
        measure(run, dev, res)
        if run.kind == "beyond":
            after = {}
            measure(ts.RUN[ts.VALID], dev, after)
            res[run.id + "/after"] = after[ts.VALID + "/out"]
        print("done", run.id, flush=True)
    torch.cuda.synchronize()
    np.savez(out, **res)
    print("OK")


_children = {}


def child(name, tmp_path_factory):
    """The arrays of environment `name`'s child, started ONCE per session, one child at a time; a failure is kept and raised again."""
    if name not in _children:
        out = str(tmp_path_factory.mktemp("two_stage_forms") / (name + ".npz"))
        code = "import sys\nfrom tests.test_two_stage_forms import child_main\nchild_main(sys.argv[1], sys.argv[2])\n"
        env = {k: v for k, v in os.environ.items() if k not in ts.STRIPPED}
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


def child_plan(got, run, key="/plan"):
    return dict(zip(PLAN_FIELDS, (int(v) for v in got[run.id + key])))


def held(tag, out, run):
    """`out` against reference64 under the run's bounds; returns (error, float32 yardstick, tol, reg)."""
    want = ts.reference64(run.id)
    tol, reg = ts.bounds(run)
    assert out.shape == want.shape and out.dtype == np.float32 and np.isfinite(out).all(), tag
    err, yard = ts.error(out, want), ts.yardstick(run)
    print("%s: %.2e of float64 (float32 oracle on the CPU %.2e; bounds %.0e and %s)" % (tag, err, yard, tol, "%.2e" % reg if reg else "none"))
    assert err <= tol, (tag, err, tol)
    if reg is not None:
        assert err <= reg, ("regression-level bound", tag, err, reg, "float32 oracle", yard)
    return err, yard, tol, reg


def took_the_table_form(env, run, p):
    """The form the child's planner recorded is the one the CPU table expects of the run in this environment."""
    want = ts.expects_pair(run, env)
    assert p["pair"] == int(want) and (p["family"] == 2) == want, (env, run.id, p)
    if want:
        N, A = run.H + 1, ts.num_actions(run)
        hr, nt = [k for k, (lo, hi) in ts.BUCKETS.items() if lo <= N <= hi][0]
        assert (p["hr"], p["node_tiles"], p["skip"], p["norm"], p["child_tiles"]) == (hr, nt, int(run.skip), ts.NORM[ts.short(run)], (A + 15) // 16), (env, run.id, p)
        assert p["image"] == int(run.head == "ship" and run.contraction == "f32") and p["head_variant"] == ts.VARIANT[run.head], (env, run.id, p)
        assert p["grid"] == min(run.P, 256) and p["parents_per_wg"] == -(-run.P // 256), (env, run.id, p)
        here = ts.plan(run)                                 # (this process runs under the default environment or the suite's own)
        if here["pair"]:
            assert all(p[k] == here[k] for k in PLAN_FIELDS), (env, run.id, p, here)


# ---------------------------------------------------------------------------------------------------------------------------
# a. against float64
# ---------------------------------------------------------------------------------------------------------------------------
CASES_A = [(env, run.id) for env in ENVS for run in ts.COVERED]
WORST = {}


@pytest.mark.parametrize("env,run_id", CASES_A, ids=["%s-%s" % c for c in CASES_A])
def test_values_against_float64(env, run_id, tmp_path_factory):
    run = ts.RUN[run_id]
    got = child(env, tmp_path_factory)
    p = child_plan(got, run)
    took_the_table_form(env, run, p)
    # the Python layer's image, as the library sizes it (the bf16x6 image is the fused kernel's: gone with that kernel's switches)
    if run.contraction == "f32":
        assert bool(got[run.id + "/image"]) == (run.head == "ship"), (env, run.id)
    else:
        assert not p["image"], (env, run.id, p)
    tag = "%s, %s under %s (%s)" % (WHAT, run.id, env, ts.form(p))
    err, yard, tol, reg = held(tag, got[run.id + "/out"], run)
    assert bool(got[run.id + "/repeat_ok"]), (tag, "two calls differ")
    fam = ("not the pair" if not p["pair"] else "head %d %s" % (p["head_variant"], "softmax" if p["norm"] == 0 else "plain-weight")) + \
        (" rand" if run.flavour == "rand" else "")
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
# b. proof of run and cross-check against the tile-kernel environment
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_id", [r.id for r in ts.COVERED])
def test_pair_against_the_tile_environment(run_id, tmp_path_factory):
    run = ts.RUN[run_id]
    other = child("tile", tmp_path_factory)
    assert child_plan(other, run)["pair"] == 0, run.id
    base = other[run.id + "/out"].astype(np.float64)
    tol, reg = ts.bounds(run)
    envs = [env for env in ts.PAIR_ENVS if ts.expects_pair(run, env)]
    assert "twostage" in envs
    worst = 0.0
    for env in envs:
        got = child(env, tmp_path_factory)
        assert child_plan(got, run)["pair"] == 1, (run.id, env)
        out = got[run.id + "/out"]
        assert not np.array_equal(out.astype(np.float64), base), (run.id, env, "bit-identical to the tile environment's values")
        err = ts.error(out, base)
        assert err <= 2 * tol and (reg is None or err <= 2 * reg), (run.id, env, err, tol, reg)
        worst = max(worst, err)
    if len(envs) == 2:              # the same kernels on the same inputs, whichever switch left the call to them
        assert np.array_equal(child("default", tmp_path_factory)[run.id + "/out"], child("twostage", tmp_path_factory)[run.id + "/out"]), run.id
    report("%s, %s: the pair (%s) within %.2e of the tile-kernel environment (asserted %s), never bit-identical to it"
           % (WHAT, run.id, " and ".join(envs), worst, "%.2e" % (2 * (reg or tol))))


# ---------------------------------------------------------------------------------------------------------------------------
# c. walking and striding runs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ts.PAIR_ENVS)
@pytest.mark.parametrize("run_id", [r.id for r in ts.WALK + ts.STRIDE])
def test_a_walked_parent_equals_the_parent_alone(run_id, env, tmp_path_factory):
    run, got = ts.RUN[run_id], child(env, tmp_path_factory)
    sample = ts.walk_sample(run.P)
    p = child_plan(got, run)
    together, alone = got[run.id + "/out"][sample], got[run.id + "/solo"]
    assert alone.shape == together.shape and len(sample) >= 24
    if not ts.expects_pair(run, env):
        # the shipped head from 1200 child tiles in the default environment: the fused kernel's launch against the pair's of one
        # parent -- two kernels, held to section a's bounds of each other
        assert not p["pair"] and env == "default" and run.head == "ship", (run.id, env, p)
        tol, reg = ts.bounds(run)
        err = ts.error(together, alone.astype(np.float64))
        assert err <= 2 * reg, (run.id, env, err, reg)
        report("%s, %s under %s: not the pair (the fused kernel); %d sampled parents within %.2e of the pair's launches of their own"
               % (WHAT, run.id, env, len(sample), err))
        return
    if run.kind == "walk":
        assert p["grid"] == 256 and p["parents_per_wg"] == -(-run.P // 256) >= 2, (run.id, p)
    else:
        assert p["head_tiles_per_wave"] == 2, (run.id, p)
    differ = [q for q, a, b in zip(sample, together, alone) if not np.array_equal(a, b)]
    assert not differ, (run.id, env, "parents whose values depend on the launch they are in", differ)
    report("%s, %s under %s (%s): %d sampled parents bit-identical to launches of their own" % (WHAT, run.id, env, ts.form(p), len(sample)))


# ---------------------------------------------------------------------------------------------------------------------------
# d. with and without the packed image
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ts.PAIR_ENVS)
@pytest.mark.parametrize("run_id", [r.id for r in ts.B6])
def test_without_the_image_equals_with_it(run_id, env, tmp_path_factory):
    run, got = ts.RUN[run_id], child(env, tmp_path_factory)
    p, q = child_plan(got, run), child_plan(got, run, "/plan_f32")
    assert p["pair"] == q["pair"] == 1 and p["image"] == 0 and q["image"] == int(run.head == "ship"), (run.id, env, p, q)
    assert {k: v for k, v in p.items() if k != "image"} == {k: v for k, v in q.items() if k != "image"}, (run.id, env, p, q)
    held("%s, %s under %s, f32 mode" % (WHAT, run.id, env), got[run.id + "/out_f32"], run)
    assert np.array_equal(got[run.id + "/out"], got[run.id + "/out_f32"]), (run.id, env, "the weights gathered matrix by matrix and the packed image give different bits")
    report("%s, %s under %s: bit-identical to the f32 mode (%s)" % (WHAT, run.id, env, "the packed image" if q["image"] else "no image either"))


# ---------------------------------------------------------------------------------------------------------------------------
# e. beyond the envelope
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("run_id", [r.id for r in ts.BEYOND])
def test_beyond_the_envelope(run_id, env, tmp_path_factory):
    run, valid, got = ts.RUN[run_id], ts.RUN[ts.VALID], child(env, tmp_path_factory)
    p = child_plan(got, run)
    assert p["pair"] == 0 and p["family"] in (3, 4, 5), (run.id, env, p)              # the deep, the tile or the one-wave-per-child kernel
    err = held("%s, %s under %s" % (WHAT, run.id, env), got[run.id + "/out"], run)[0]
    assert bool(got[run.id + "/repeat_ok"]), (run.id, env)
    after = got[run.id + "/after"]
    held("%s after %s under %s" % (valid.id, run.id, env), after, valid)
    assert np.array_equal(after, got[valid.id + "/out"]), (run.id, env, "the valid run changed after the run beyond the envelope")
    report("%s, %s under %s: kernel family %d answers, %.2e of the float64 oracle; %s right after it is bit-identical to its first run"
           % (WHAT, run.id, env, p["family"], err, valid.id))


# ---------------------------------------------------------------------------------------------------------------------------
# f. poisoned workspaces
# ---------------------------------------------------------------------------------------------------------------------------
def test_whole_module_with_poisoned_workspaces():
    """Every test above once more with workspaces and outputs filled with NaN patterns before the kernels run: the rows stage 2 reads
    were written by stage 1 of the same parents, whichever workgroup walked them."""
    if nat.poison_workspaces():
        return                              # this IS the poisoned run
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_two_stage_forms.py"), "-q", "-m", "gpu", "-x",
                          "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, RGL_DEBUG_POISON_WORKSPACES="1"),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and " passed" in res.stdout, res.stdout[-6000:] + res.stderr[-2000:]
    report("%s with poisoned workspaces: %s" % (WHAT, res.stdout.strip().splitlines()[-1].strip("= ")))
