"""Generate tests/golden/explore.npz: the reference's own Explorer exploring in the `train` phase (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_explore.py [OUT.npz]

The setting of make_golden.py's gen_explorer_kats -- the reference Explorer, CrowdSim (linear humans, 1.5 m circle, 12 s limit)
and ModelPredictiveRL (weights_goal.npz, depth 1) -- with `set_epsilon(EPSILON)`: CrowdSim.reset seeds numpy per case, the
scene consumes doubles and every predict continues that stream with `np.random.random()` and, when it explores,
`np.random.choice(81)`.  Both calls are logged by wrapping the two functions on the numpy module while the episodes run, so
nothing in the reference changes.  Each case runs as one `run_k_episodes(1, "train", update_memory=True)` with the
environment's case counter set to it.

Cases: the first N_CASES training cases from 0 upwards none of whose GREEDY decisions rests on a near-tie: the top two root
values, evaluated by oracle/rgl_oracle.py on the recorded float64 states, are at least MIN_GAP = 1e-4 apart (the parity bound on
values), so that the product's float32 kernels take the same greedy action.  The smallest gap found is
stored.  The fixture must hold at least 10 explored decisions and one rejected draw of the masked rejection (asserted here
with tests/explore_cpu.py and again by tests/test_explore_cpu.py).

`ex.` arrays: cases, draws (doubles the scene took), epsilon, n_actions, per decision (all cases concatenated; steps_end =
cumulative decision count per case) actions, probability, choice (-1: not explored); per case outcome (2 collision, 3 goal,
4 timeout), time (global_time at the end), n_tuples (pushed into the ReplayMemory); min_gap, circle_radius, time_limit.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_loader  # noqa: E402

policy_factory = ref_loader.load_reference()

from crowd_sim.envs.utils.state import JointState  # noqa: E402

from oracle import rgl_oracle as orc  # noqa: E402
from tests import explore_cpu as xc  # noqa: E402
from tests import golden_io as gio  # noqa: E402

EPSILON = 0.3
N_CASES = 8
MIN_GAP = 1e-4
CIRCLE_RADIUS, TIME_LIMIT = 1.5, 12


def build(candidates=range(0, 200)):
    import gym
    from crowd_sim.envs.utils.robot import Robot
    from crowd_sim.envs.utils.info import ReachGoal, Collision
    from crowd_nav.utils.explorer import Explorer
    from crowd_nav.utils.memory import ReplayMemory
    JointState.self_state = property(lambda self_: self_.robot_state)       # the in-memory alias gen_explorer_kats uses
    mod = importlib.import_module("crowd_nav.configs.icra_benchmark.mp_separate")
    envc = mod.EnvConfig()
    envc.humans.policy = "linear"
    envc.sim.centralized_planning = False
    envc.sim.circle_radius, envc.env.time_limit = CIRCLE_RADIUS, TIME_LIMIT
    env = gym.make("CrowdSim-v0")
    env.configure(envc)
    robot = Robot(envc, "robot")
    robot.time_step = env.time_step
    pol = policy_factory["model_predictive_rl"]()
    pol.configure(mod.PolicyConfig())
    pol.load_state_dict(gio.checkpoint("goal"))
    pol.set_device(torch.device("cpu"))
    pol.set_time_step(env.time_step)
    pol.set_epsilon(EPSILON)
    ve_fwd = pol.value_estimator.forward
    pol.value_estimator.forward = lambda state: ve_fwd(state).reshape(())        # scalar-shape shim (make_golden.py's header)
    robot.set_policy(pol)
    env.set_robot(robot)
    memory = ReplayMemory(100000)
    explorer = Explorer(env, robot, torch.device("cpu"), None, memory, 0.9, target_policy=pol)
    params, ocfg = gio.oracle_params("goal"), orc.OracleConfig()

    log = {}
    act0, step0 = robot.act, env.step
    random0, choice0 = np.random.random, np.random.choice

    def act(ob):
        log["roots"].append((robot.get_full_state(), list(ob)))
        n_before = len(log["probability"])
        log["deciding"] = True
        a = act0(ob)
        log["deciding"] = False
        assert len(log["probability"]) == n_before + 1               # one decision, one draw
        table = [(x.vx, x.vy) for x in pol.action_space]
        index = table.index((a.vx, a.vy))
        if log["choice"][-1] >= 0:
            assert index == log["choice"][-1]
        log["actions"].append(index)
        return a

    def step(action, update=True):
        ob, reward, done, info = step0(action, update)
        if done and update:
            log["end"] = (3 if isinstance(info, ReachGoal) else (2 if isinstance(info, Collision) else 4), env.global_time)
        return ob, reward, done, info

    def random():
        p = random0()
        if log["deciding"]:
            log["probability"].append(p)
            log["choice"].append(-1)
        else:
            log["scene_draws"] += 1                  # generate_human's (the circle draws with np.random.random alone)
        return p

    def choice(n):
        c = choice0(n)
        log["choice"][-1] = int(c)
        return c

    def smallest_gap():
        greedy = [i for i, c in enumerate(log["choice"]) if c < 0]
        if not greedy:
            return np.inf
        r64 = np.array([[s.px, s.py, s.vx, s.vy, s.radius, s.gx, s.gy, s.v_pref, s.theta] for s, _ in log["roots"]])[greedy]
        h64 = np.array([[[h.px, h.py, h.vx, h.vy, h.radius] for h in ob] for _, ob in log["roots"]])[greedy]
        with torch.no_grad():
            best, _, values, _ = orc.mprl_predict_batched(torch.tensor(r64.astype(np.float32)), torch.tensor(h64.astype(np.float32)),
                                                          params, ocfg, roots64=(r64, h64))
        if [int(a) for a in best] != [log["actions"][i] for i in greedy]:        # a tie the oracle breaks the other way
            return 0.0
        top = np.sort(values.numpy().astype(np.float64), axis=1)
        return float((top[:, -1] - top[:, -2]).min())

    kept = []
    robot.act, env.step = act, step
    np.random.random, np.random.choice = random, choice
    try:
        with torch.no_grad():
            for case in candidates:
                log.update(roots=[], probability=[], choice=[], actions=[], end=None, deciding=False, scene_draws=0)
                env.case_counter["train"] = case
                n_before = len(memory.memory)
                explorer.run_k_episodes(1, "train", update_memory=True, episode=3)
                gap = smallest_gap()
                print("case %d: %d decisions, %d explored, outcome %d, %d tuples, smallest gap %.3e"
                      % (case, len(log["actions"]), sum(c >= 0 for c in log["choice"]), log["end"][0],
                         len(memory.memory) - n_before, gap))
                if gap >= MIN_GAP:
                    kept.append(dict(case=case, gap=gap, actions=list(log["actions"]), probability=list(log["probability"]),
                                     choice=list(log["choice"]), end=log["end"], scene_draws=log["scene_draws"], n_tuples=len(memory.memory) - n_before))
                if len(kept) == N_CASES:
                    break
    finally:
        robot.act, env.step = act0, step0
        np.random.random, np.random.choice = random0, choice0
        del JointState.self_state
    assert len(kept) == N_CASES

    # the draws of each scene and the fixture's counts, from the restatement
    from relationalgraphlearning_amd.sim import BASE_SEED, SimConfig, generate_scene_with_draws
    scfg = SimConfig(circle_radius=CIRCLE_RADIUS, time_limit=TIME_LIMIT)
    draws, rejections = [], 0
    n_actions = len(pol.action_space)
    for k in kept:
        d = generate_scene_with_draws(scfg, "train", k["case"])[4]
        assert d == k["scene_draws"]                 # the host generator's count is the reference's
        draws.append(d)
        st = xc.ExploreStream(BASE_SEED["train"] + k["case"], d)
        for a, p, c in zip(k["actions"], k["probability"], k["choice"]):
            chosen, explored = st.decide(a, n_actions, EPSILON)
            assert st.last_u == p and explored == int(c >= 0) and chosen == a
        rejections += st.rejections
    n_explored = sum(c >= 0 for k in kept for c in k["choice"])
    print("kept cases %s: %d decisions, %d explored, %d rejected draws" % ([k["case"] for k in kept],
                                                                           sum(len(k["actions"]) for k in kept), n_explored, rejections))
    assert n_explored >= 10 and rejections >= 1
    cat = lambda name, dtype: np.array([x for k in kept for x in k[name]], dtype)      # noqa: E731
    return {"ex.cases": np.array([k["case"] for k in kept], np.int64), "ex.draws": np.array(draws, np.int64),
            "ex.epsilon": np.array(EPSILON), "ex.n_actions": np.array(n_actions, np.int64),
            "ex.actions": cat("actions", np.int64), "ex.probability": cat("probability", np.float64),
            "ex.choice": cat("choice", np.int64), "ex.steps_end": np.cumsum([len(k["actions"]) for k in kept]).astype(np.int64),
            "ex.outcome": np.array([k["end"][0] for k in kept], np.int64), "ex.time": np.array([k["end"][1] for k in kept], np.float64),
            "ex.n_tuples": np.array([k["n_tuples"] for k in kept], np.int64), "ex.min_gap": np.array(min(k["gap"] for k in kept)),
            "ex.circle_radius": np.array(CIRCLE_RADIUS), "ex.time_limit": np.array(float(TIME_LIMIT))}


if __name__ == "__main__":
    target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "explore.npz")
    np.savez_compressed(target, **build())
    print("wrote", target, os.path.getsize(target), "bytes")
