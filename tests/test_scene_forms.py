"""scene_graph_kernel<NT, SK, WAVES, CH, SPLIT, EMB, BX> of csrc/rgl_scene.hip in every f32 form it launches (tests/scene_forms.py: the
runs, the form each takes by the library's own planner -- held on the CPU by tests/test_scene_forms_cpu.py -- and the references).
The harness is tests/test_deep_forms.py's.

Routes: nets.graph_forward with the value head (value rows + the head's row kernel) or the motion head, TreeSearch.expand (the state
predictor, the level's reward work offered to the launch), TreeSearch.value_children of cosine / concatenation / layerwise graphs
(crowds_per = A) and gcn_search().search (path G's 6 / 7-wide rows).  The scene environments run under RGL_REQUIRE_MFMA_FORWARD=1,
RGL_REQUIRE_MFMA_CHILDREN=1 and RGL_TILES_FORWARD=0: no general kernel and no tile kernel can answer for this one, and each child
records its own planner's answer beside its outputs.

  a. every answered run in every scene environment against reference64, relative to max(1, max|want|), under TOL and max(REG_F32, 8 x
     the float32 oracle's deviation) (raw random-init weights and path G: TOL only); finite, shape, dtype; two calls bit-identical;
     the child's plan names the instantiation the environment implies.
  b. the scene environments against the general kernel (`generic`) and the tile kernels (`tiles`, forward runs they cover): within
     twice the bounds, and different in bits on every run.  Split against unsplit and embeddings inside against rows from the
     embedding launch: within the bounds; bit-identical where both plans name the same instantiation.
  c. expand: humans_next of `ride0` and `ride1` bit-identical where they differ in CH alone; reward / child_robot bit-identical to
     estimate_reward on its own in every environment.
  d. walking runs: a sample of scenes over the first pass, the turn into the second, the middle and the end, in whole crowds, equals
     bit for bit a launch of those scenes alone in every environment in which both take the same instantiation (at least one per
     run); within the bounds otherwise.
  e. beyond the envelope: concatenation at 65 nodes and five layers raise RGL_ERR_BAD_MODE (the general kernel answers in `generic`),
     129 nodes RGL_ERR_BAD_SHAPE; the valid run right after each is bit-identical to its first run.  (This section found the
     require switch silent for exactly these two: no MFMA kernel covers them, so the caller gets no workspace, and the refusal sat
     behind the workspace check of rgl_graph_forward_f32.)
  f. the whole module once more with poisoned workspaces.

One child process per environment, started once per session, each under its own time limit; a child that fails -- by an assertion, a
signal, an abort or its time limit -- fails every test that needs it and is not started again.  profiles/scene_kernel_forms.txt
holds the parity-report lines of a run of this module.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import relationalgraphlearning_amd as rga
from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd import nets
from relationalgraphlearning_amd.config import policy_config
from tests import graph_forms as gf
from tests import scene_forms as sf
from tests.helpers import make_gcn_policy
from tests.test_gpu_parity import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHAT = "scene kernel forms"
REQUIRE = {"RGL_REQUIRE_MFMA_FORWARD": "1", "RGL_REQUIRE_MFMA_CHILDREN": "1", "RGL_TILES_FORWARD": "0"}
ENVS = dict({name: dict(sw, **REQUIRE) for name, sw in sf.SCENE_ENVS.items()},
            tiles={"RGL_TILES_FORWARD": "2"}, generic={"RGL_FORCE_GENERIC": "1"})
FORWARD_ENVS = ("default", "unsplit", "split", "noembed")          # every run; ride0 / ride1: the expand runs; tiles: the forward runs
PLAN_FIELDS = ("covered", "node_tiles", "family", "waves", "split", "embed_inside", "children_riding", "slots", "grid", "grid_cap", "last_steps")
CHILD_TIMEOUT = 60                  # measured: 2.2 to 3.3 s per child process (0.2 to 0.7 s of it on its runs), 52 s for the module with its poisoned rerun


def runs_of(env):
    if env in ("ride0", "ride1"):
        return sf.EXPAND
    if env == "tiles":
        return [r for r in sf.RUNS if r.route == "forward"]
    return sf.RUNS


# ---------------------------------------------------------------------------------------------------------------------------
# the child processes
# ---------------------------------------------------------------------------------------------------------------------------
_built = {}


def modules(run, dev):
    """(graph, head descriptor or None, motion descriptor or None) of a forward run; the policy of the other routes."""
    key = (run.route, run.L, run.sim, run.lw, run.skip, run.flavour, run.head, run.table)
    if key in _built:
        return _built[key]
    ck = sf.checkpoint(run) if run.route != "pathg" else None
    if run.route == "forward":
        cfg = policy_config(gcn__num_layer=run.L, gcn__similarity_function=run.sim, gcn__layerwise_graph=run.lw, gcn__skip_connection=run.skip)
        g = rga.RGL(cfg, 9, 5)
        g.load_state_dict(ck["graph_model2" if run.head == "motion" else "graph_model1"])
        if run.head == "motion":
            top = rga.StatePredictor(cfg, g, 0.25)
            top.human_motion_predictor.load_state_dict(ck["motion_predictor"])
        else:
            top = rga.ValueEstimator(cfg, g)
            top.value_network.load_state_dict(ck["value_network"])
        _built[key] = top.to(dev)
    elif run.route == "pathg":
        pol = make_gcn_policy(device=dev)
        pol.build_action_space(1.0)
        _built[key] = pol
    else:
        cfg = policy_config("model_predictive_rl", gcn__num_layer=run.L, gcn__similarity_function=run.sim, gcn__layerwise_graph=run.lw,
                            gcn__skip_connection=run.skip, action_space__speed_samples=run.table[0], action_space__rotation_samples=run.table[1])
        pol = rga.ModelPredictiveRL()
        pol.time_step = 0.25
        pol.configure(cfg)
        pol.load_state_dict(ck)
        pol.set_time_step(0.25)
        pol.set_phase("test")
        pol.set_device(dev)
        pol.build_action_space(1.0)
        _built[key] = pol
    return _built[key]


def launch(run, dev, a, humans):
    """The run's route over (a, humans) -> {"out": array, and for expand "reward", "child_robot"}."""
    top = modules(run, dev)
    a, humans = a.to(dev), humans.to(dev)
    if run.route == "forward":
        head = top.head_descriptor()
        out = nets.graph_forward(top.graph_model.descriptor(), head if run.head == "value" else None, head if run.head == "motion" else None,
                                 a, humans, scenes_per_crowd=a.shape[0] // humans.shape[0])
        return {"out": out["value" if run.head == "value" else "humans_next"].cpu().numpy()}
    if run.route == "pathg":
        return {"out": top.gcn_search().search(a, humans)[0].cpu().numpy()}
    ts = top.tree_search()
    assert ts.num_actions == sf.actions_of(run), run.id
    if run.route == "children":
        return {"out": ts.value_children(a, humans).cpu().numpy()}
    got = ts.expand(a, humans, parents_are_joint_states=False)
    return {"out": got["humans_next"].cpu().numpy(), "reward": got["reward"].cpu().numpy(), "child_robot": got["child_robot"].cpu().numpy()}


def measure(run, dev, res):
    """The run twice; an expand run's reward step on its own; a walking run's sampled scenes alone."""
    p = sf.plan(run) if run.H + 1 <= 128 else {k: 0 for k in PLAN_FIELDS}            # this process's planner, under this process's switches
    res[run.id + "/plan"] = np.array([p[k] for k in PLAN_FIELDS])
    if run.route == "forward" and run.H + 1 <= 64:
        res[run.id + "/tiles"] = np.array(gf.plan(gf.Run(run.id, "value", 32, [64, 32], [64, 32], [], sf.n_scenes(run), run.H, 0, {}, run.L, run.sim,
                                                         run.lw, run.skip, run.spc, True, None, False), False)["covered"])
    a, humans = sf.inputs(run.id)
    try:
        first = launch(run, dev, a, humans)
    except nat.NativeLibraryError as e:
        res[run.id + "/error"] = np.array(str(e))
        return
    for k, v in first.items():
        res[run.id + "/" + k] = v
    again = launch(run, dev, a, humans)
    res[run.id + "/repeat_ok"] = np.array(all(np.array_equal(first[k], again[k]) for k in first))
    if run.route == "expand":
        cr, rew = modules(run, dev).tree_search().estimate_reward(a.to(dev), humans.to(dev), parents_are_joint_states=False)
        res[run.id + "/est_child_robot"], res[run.id + "/est_reward"] = cr.cpu().numpy(), rew.cpu().numpy()
    if run.kind == "walk" and p["covered"]:
        sample = sf.walk_sample(run, p)
        spc = sf.scenes_per_crowd(run)
        alone = sf.plan(run, len(sample))
        res[run.id + "/solo_plan"] = np.array([alone[k] for k in PLAN_FIELDS])
        res[run.id + "/solo"] = launch(run, dev, a[sample], humans[[s // spc for s in sample[::spc]]])["out"]
        res[run.id + "/sample"] = np.array(sample)


def child_main(name, out):
    """Entry point of the child of environment `name`: its runs; after each run beyond the envelope, the valid run once more."""
    dev = torch.device("cuda:0")
    res = {}
    t0 = time.time()
    for run in runs_of(name):
        measure(run, dev, res)
        if run.kind == "beyond":
            after = {}
            measure(sf.RUN[sf.VALID], dev, after)
            res[run.id + "/after"] = after[sf.VALID + "/out"]
        print("done", run.id, flush=True)
    torch.cuda.synchronize()
    res["seconds"] = np.array(time.time() - t0)
    np.savez(out, **res)
    print("OK")


_children = {}


def child(name, tmp_path_factory):
    """The arrays of environment `name`'s child, started ONCE per session, one child at a time; a failure is kept and raised again."""
    if name not in _children:
        out = str(tmp_path_factory.mktemp("scene_forms") / (name + ".npz"))
        code = "import sys\nfrom tests.test_scene_forms import child_main\nchild_main(sys.argv[1], sys.argv[2])\n"
        try:
            res = subprocess.run([sys.executable, "-c", code, name, out], cwd=ROOT, env=sf.child_environment(ENVS[name]), capture_output=True,
                                 text=True, timeout=CHILD_TIMEOUT)
            if res.returncode != 0 or "OK" not in res.stdout:
                raise AssertionError("child ended with %s\n%s" % (res.returncode, res.stdout[-2000:] + res.stderr[-4000:]))
            _children[name] = dict(np.load(out))
        except Exception as e:              # also the time limit: remembered, not retried
            _children[name] = e
    if isinstance(_children[name], Exception):
        raise AssertionError("the child process of environment %s failed (started once): %s" % (name, _children[name]))
    return _children[name]


def child_plan(got, run, key="/plan"):
    p = dict(zip(PLAN_FIELDS, (int(v) for v in got[run.id + key])))
    p["inst"] = tuple(p[k] for k in PLAN_FIELDS[1:7]) if p["covered"] else None
    return p


def held(tag, out, run, want=None, twice=1):
    """`out` against reference64 under the run's bounds; returns (error, float32 yardstick, tol, reg)."""
    want = sf.reference64(run.id) if want is None else want
    tol, reg = sf.bounds(run)
    assert out.shape == want.shape and out.dtype == np.float32 and np.isfinite(out).all(), (tag, out.shape, want.shape, out.dtype)
    err, yard = sf.error(out, want), sf.yardstick(run)
    print("%s: %.2e of float64 (float32 oracle on the CPU %.2e; bounds %.0e and %s)" % (tag, err, yard, tol, "%.2e" % reg if reg else "none"))
    assert err <= twice * tol, (tag, err, tol)
    if reg is not None:
        assert err <= twice * reg, ("regression-level bound", tag, err, reg, "float32 oracle", yard)
    return err, yard, tol, reg


# ---------------------------------------------------------------------------------------------------------------------------
# a. against float64
# ---------------------------------------------------------------------------------------------------------------------------
CASES_A = [(env, run.id) for env in sf.SCENE_ENVS for run in runs_of(env) if run.kind != "beyond"]
WORST = {}


@pytest.mark.parametrize("env,run_id", CASES_A, ids=["%s-%s" % c for c in CASES_A])
def test_outputs_against_float64(env, run_id, tmp_path_factory):
    run = sf.RUN[run_id]
    got = child(env, tmp_path_factory)
    assert run.id + "/out" in got, (env, run.id, got.get(run.id + "/error"))
    p = child_plan(got, run)
    assert p["covered"] == 1 and p["inst"] == sf.expected(run, env), (env, run.id, p, sf.expected(run, env))
    tag = "%s, %s under %s (%s)" % (WHAT, run.id, env, sf.form(p))
    err, yard, tol, reg = held(tag, got[run.id + "/out"], run)
    assert bool(got[run.id + "/repeat_ok"]), (tag, "two calls differ")
    w = WORST.setdefault((env, p["node_tiles"], p["family"]), [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], err), max(w[1], yard), w[2] + 1
    if env == "default" or run.kind == "walk":
        report("%s: %.2e of the float64 oracle (float32 oracle on the CPU %.2e; asserted %.0e and %s)"
               % (tag, err, yard, tol, "%.2e" % reg if reg else "the north-star bound only"))


def test_worst_deviation_per_environment_node_tiles_and_family():
    """The report's summary: per (environment, NT, SK) the worst deviation from float64 next to the float32 oracle's."""
    assert WORST, "section a did not run"
    for (env, nt, sk), (err, yard, n) in sorted(WORST.items()):
        report("%s, worst over %d runs under %s, NT=%d SK=%d: %.2e of the float64 oracle (float32 oracle on the CPU: %.2e)" % (WHAT, n, env, nt, sk, err, yard))


# ---------------------------------------------------------------------------------------------------------------------------
# b. proof of run and cross-checks
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_id", [r.id for r in sf.ANSWERED])
def test_scene_kernel_against_the_other_kernels_and_its_own_forms(run_id, tmp_path_factory):
    run = sf.RUN[run_id]
    envs = FORWARD_ENVS + (("ride0", "ride1") if run.route == "expand" else ())
    outs = {env: child(env, tmp_path_factory)[run.id + "/out"] for env in envs}
    plans = {env: child_plan(child(env, tmp_path_factory), run) for env in envs}
    tol, reg = sf.bounds(run)
    others = {"generic": child("generic", tmp_path_factory)}
    assert child_plan(others["generic"], run)["covered"] == 0
    if run.route == "forward" and run.id + "/tiles" in others["generic"] and int(child("tiles", tmp_path_factory)[run.id + "/tiles"]):
        others["tiles"] = child("tiles", tmp_path_factory)
    worst = 0.0
    for name, other in others.items():
        base = other[run.id + "/out"]
        held("%s, %s under %s" % (WHAT, run.id, name), base, run)
        for env, out in outs.items():
            err = sf.error(out, base.astype(np.float64))
            assert err <= 2 * tol and (reg is None or err <= 2 * reg), (run.id, env, name, err, tol, reg)
            worst = max(worst, err)
            assert not np.array_equal(out, base), (run.id, env, "bit-identical to the %s environment's output" % name)
    same = 0
    for a, b in (("unsplit", "split"), ("default", "noembed"), ("default", "split"), ("default", "unsplit"), ("ride0", "ride1")):
        if a in outs and b in outs:
            err = sf.error(outs[a], outs[b].astype(np.float64))
            assert err <= tol and (reg is None or err <= reg), (run.id, a, b, err)
            if plans[a]["inst"][:5] == plans[b]["inst"][:5]:          # the same scene instantiation (but for CH): the same bits
                assert np.array_equal(outs[a], outs[b]), (run.id, a, b, plans[a]["inst"])
                same += 1
    report("%s, %s: within %.2e of %s (asserted %s); its environments agree within the bounds, %d pairs of one instantiation bit-identical"
           % (WHAT, run.id, worst, " and ".join(sorted(others)), "%.2e" % (2 * (reg or tol)), same))


# ---------------------------------------------------------------------------------------------------------------------------
# c. the riding reward work
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_id", [r.id for r in sf.EXPAND])
def test_riding_reward_work(run_id, tmp_path_factory):
    run = sf.RUN[run_id]
    r0, r1 = child("ride0", tmp_path_factory), child("ride1", tmp_path_factory)
    p0, p1 = child_plan(r0, run), child_plan(r1, run)
    assert (p0["children_riding"], p1["children_riding"]) == (0, 1) and p0["inst"][:4] == p1["inst"][:4], (p0, p1)
    if p0["inst"][:5] == p1["inst"][:5]:
        assert np.array_equal(r0[run.id + "/out"], r1[run.id + "/out"]), (run.id, "humans_next with and without the riding reward work")
    for env in sf.SCENE_ENVS:
        got = child(env, tmp_path_factory)
        assert np.array_equal(got[run.id + "/reward"], got[run.id + "/est_reward"]), (run.id, env, "reward")
        assert np.array_equal(got[run.id + "/child_robot"], got[run.id + "/est_child_robot"]), (run.id, env, "child_robot")
        assert np.isfinite(got[run.id + "/reward"]).all() and got[run.id + "/reward"].shape == (run.P, sf.actions_of(run))
    report("%s, %s: humans_next %s with (%s) and without the riding reward work; reward and child_robot bit-identical to estimate_reward in %d environments"
           % (WHAT, run.id, "bit-identical" if p0["inst"][:5] == p1["inst"][:5] else "within the bounds (the embeddings move out of the launch)",
              sf.form(p1), len(sf.SCENE_ENVS)))


# ---------------------------------------------------------------------------------------------------------------------------
# d. walking runs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_id", [r.id for r in sf.WALK])
def test_a_walked_scene_equals_the_scene_alone(run_id, tmp_path_factory):
    run = sf.RUN[run_id]
    tol, reg = sf.bounds(run)
    exact = []
    for env in FORWARD_ENVS:
        got = child(env, tmp_path_factory)
        p, alone = child_plan(got, run), child_plan(got, run, "/solo_plan")
        sample = got[run.id + "/sample"]
        together, solo = got[run.id + "/out"][sample], got[run.id + "/solo"]
        assert solo.shape == together.shape and len(sample) >= 32
        if env == "default":
            assert p["grid"] == p["grid_cap"] and sf.n_scenes(run) > p["grid"] * p["slots"], (run.id, p)
        if p["inst"] == alone["inst"]:
            differ = [int(s) for s, x, y in zip(sample, together, solo) if not np.array_equal(x, y)]
            assert not differ, (run.id, env, "scenes whose outputs depend on the launch they are in", differ)
            exact.append(env)
        else:
            err = sf.error(together, solo.astype(np.float64))
            assert err <= tol and (reg is None or err <= reg), (run.id, env, err)
    assert exact, (run.id, "no environment in which the sample alone takes the walking launch's instantiation")
    report("%s, %s (%s): %d sampled scenes bit-identical to a launch of their own under %s; within the bounds under the others"
           % (WHAT, run.id, sf.form(sf.plan(run)), len(sample), ", ".join(exact)))


# ---------------------------------------------------------------------------------------------------------------------------
# e. beyond the envelope
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", FORWARD_ENVS + ("generic",))
@pytest.mark.parametrize("run_id", [r.id for r in sf.BEYOND])
def test_beyond_the_envelope(run_id, env, tmp_path_factory):
    run, valid, got = sf.RUN[run_id], sf.RUN[sf.VALID], child(env, tmp_path_factory)
    assert child_plan(got, run)["covered"] == 0, run.id
    what = sf.REFUSALS[run.id][env == "generic"]
    if what == "answers":
        assert run.id + "/out" in got, (run.id, env, got.get(run.id + "/error"))
        held("%s, %s under %s" % (WHAT, run.id, env), got[run.id + "/out"], run)
        assert bool(got[run.id + "/repeat_ok"])
        what = "the general kernel answers"
    else:
        err = str(got.get(run.id + "/error"))
        assert run.id + "/out" not in got and what in err and "rgl_graph_forward_f32" in err, (run.id, env, err)
        what = "raises " + what
    after = got[run.id + "/after"]
    held("%s after %s under %s" % (valid.id, run.id, env), after, valid)
    assert np.array_equal(after, got[valid.id + "/out"]), (run.id, env, "the valid run changed after the refusal")
    report("%s, %s under %s: %s; %s right after it is bit-identical to its first run" % (WHAT, run.id, env, what, valid.id))


def test_children_times(tmp_path_factory):
    """Seconds each child spent on its runs (its start, imports included, adds about two), for the report."""
    took = {name: float(child(name, tmp_path_factory)["seconds"]) for name in ENVS}
    report("%s, seconds per child: %s" % (WHAT, ", ".join("%s %.1f" % kv for kv in sorted(took.items()))))


# ---------------------------------------------------------------------------------------------------------------------------
# f. poisoned workspaces
# ---------------------------------------------------------------------------------------------------------------------------
def test_whole_module_with_poisoned_workspaces():
    """Every test above once more with workspaces and outputs filled with NaN patterns before the kernels run: the x0 / xh rows the
    scene kernel reads were written by the embedding launch before it, the value rows by the scene kernel before the head's."""
    if nat.poison_workspaces():
        return                              # this IS the poisoned run
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_scene_forms.py"), "-q", "-m", "gpu", "-x",
                          "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, RGL_DEBUG_POISON_WORKSPACES="1"),
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and " passed" in res.stdout, res.stdout[-6000:] + res.stderr[-2000:]
    report("%s with poisoned workspaces: %s" % (WHAT, res.stdout.strip().splitlines()[-1].strip("= ")))
