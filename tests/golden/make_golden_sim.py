"""Generate tests/golden/sim_modes.npz: the reference's own CrowdSim.step in the modes sim.npz does not hold (build
container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sim.py [OUT.npz]

Unicycle robots (ActionRot over the reference's unicycle action table) under four scripts -- turn towards the goal, seeded
random, and turning one way with positive and with negative r so that theta passes the ends of [0, 2 pi) several times --;
non-default constants (all six of the reward ladder at once, and another time_step); 1, 5 and 19 humans and a
square_crossing scene; humans driven by scripted actions (`given`) and humans that keep their velocity
(`constant_velocity`), both by replacing `human.act` in memory; and CrowdSim.onestep_lookahead for every action of the table
at three steps of four trajectories (one of them unicycle; the steps are chosen so that the table meets collisions, goals,
discomfort and the time limit).  Same in-memory shim as make_golden.gen_sim_kats (JointState.self_state aliased to
robot_state for the reference's Linear.predict); nothing of the reference is changed on disk or copied: the file holds
states, actions, settings and outcomes only.

Per trajectory `modes.<tag>.`: robot (T+1, 9) and humans (T+1, H, 9) full states (px, py, vx, vy, radius, gx, gy, v_pref,
theta), actions (T,) indices into `modes.table.<kinematics>` ((v, r) rows for unicycle), reward / done / info / dmin (T,)
(dmin: Discomfort.min_dist, NaN otherwise), time (T+1,), human_actions (T, H, 2) (what every human did), constants (6,)
(time_step, time_limit, success_reward, collision_penalty, discomfort_dist, discomfort_penalty_factor); with lookaheads
also look_steps (L,), look_reward / look_done / look_info (L, A) and look_humans (L, A, H, 5).  `modes_cases` lists
"tag|kinematics|human policy|script|phase|case|scenario|H".

No recorded step or lookahead may have a margin (oracle/sim_oracle.py) below 1e-9 on the reference's own states: a case
that has one is replaced by the case 100 further on.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_loader  # noqa: E402

policy_factory = ref_loader.load_reference()

from crowd_sim.envs.utils.action import ActionXY, ActionRot  # noqa: E402
from crowd_sim.envs.utils.state import JointState  # noqa: E402
from oracle import sim_oracle as so  # noqa: E402

INFO_CODES = {"": 0, "Discomfort": 1, "Collision": 2, "Reaching goal": 3, "Timeout": 4}
MIN_MARGIN = 1e-9
MAX_STEPS = 140
DEFAULTS = (0.25, 30, 1, -0.25, 0.2, 0.5)
OTHER = (0.25, 10, 2.5, -0.6, 0.45, 0.8)          # a short clock, a wide discomfort zone, other rewards and factor
OTHER_DT = (0.2, 30, 1, -0.25, 0.2, 0.5)          # another time step alone
OTHER_ALL = (0.4, 12, 0.7, -1.5, 0.35, 0.25)      # all six at once
# 19 humans on the 4 m circle are placed with discomfort_dist as clearance: the default leaves room, 0.35 does not
OTHER_19 = (0.25, 12, 0.7, -1.5, 0.2, 0.25)
# tag, kinematics, human policy, script, case, scenario, H, constants, lookahead steps
CASES = [
    ("uni_turn0", "unicycle", "linear", "turn", 0, "circle_crossing", 5, DEFAULTS, (2, 8, 11)),
    ("uni_turn1", "unicycle", "linear", "turn", 1, "circle_crossing", 5, DEFAULTS, ()),
    ("uni_turn2", "unicycle", "linear", "turn", 2, "circle_crossing", 5, DEFAULTS, ()),
    ("uni_random0", "unicycle", "linear", "random", 0, "circle_crossing", 5, DEFAULTS, ()),
    ("uni_spin_pos", "unicycle", "linear", "spin+", 3, "circle_crossing", 5, OTHER, ()),
    ("uni_spin_neg", "unicycle", "given", "spin-", 4, "circle_crossing", 5, OTHER, ()),
    ("uni_late19", "unicycle", "constant_velocity", "late", 1, "circle_crossing", 19, OTHER_DT, ()),
    ("uni_square", "unicycle", "linear", "turn", 3, "square_crossing", 5, OTHER_ALL, ()),
    ("uni_one", "unicycle", "given", "turn", 5, "circle_crossing", 1, DEFAULTS, ()),
    ("holo_other", "holonomic", "linear", "greedy", 0, "circle_crossing", 5, OTHER_ALL, ()),
    ("holo_stop_other", "holonomic", "constant_velocity", "stop", 1, "circle_crossing", 5, OTHER, (1, 20, 36)),
    ("holo_dt", "holonomic", "linear", "late", 2, "circle_crossing", 5, OTHER_DT, (35, 60, 68)),
    ("holo_given19", "holonomic", "given", "greedy", 1, "circle_crossing", 19, OTHER_19, ()),
    ("holo_one", "holonomic", "linear", "greedy", 6, "circle_crossing", 1, DEFAULTS, (3, 10, 13)),
    ("holo_square_cv", "holonomic", "constant_velocity", "random", 4, "square_crossing", 5, DEFAULTS, ()),
]


def _full(agent):
    return [agent.px, agent.py, agent.vx, agent.vy, agent.radius, agent.gx, agent.gy, agent.v_pref, agent.theta]


def _make_env(kinematics, scenario, H, constants):
    import gym
    from crowd_sim.envs.utils.robot import Robot
    mod = importlib.import_module("crowd_nav.configs.icra_benchmark.mp_separate")
    envc = mod.EnvConfig()
    envc.humans.policy = "linear"
    envc.sim.centralized_planning = False
    envc.sim.test_scenario = envc.sim.train_val_scenario = scenario
    envc.sim.human_num = H
    envc.env.time_step, envc.env.time_limit = constants[0], constants[1]
    envc.reward.success_reward, envc.reward.collision_penalty = constants[2], constants[3]
    envc.reward.discomfort_dist, envc.reward.discomfort_penalty_factor = constants[4], constants[5]
    env = gym.make("CrowdSim-v0")
    env.configure(envc)
    robot = Robot(envc, "robot")
    robot.time_step = env.time_step
    pc = mod.PolicyConfig()
    pc.action_space.kinematics = kinematics
    pol = policy_factory["model_predictive_rl"]()
    pol.configure(pc)
    robot.set_policy(pol)
    env.set_robot(robot)
    pol.build_action_space(1.0)
    return env, robot, pol


def _table(pol, kinematics):
    if kinematics == "holonomic":
        return np.array([[a.vx, a.vy] for a in pol.action_space], np.float64)
    return np.array([[a.v, a.r] for a in pol.action_space], np.float64)


def _action(table, ai, kinematics):
    a0, a1 = np.float64(table[ai, 0]), np.float64(table[ai, 1])
    return ActionXY(a0, a1) if kinematics == "holonomic" else ActionRot(a0, a1)


def _choose(script, t, robot, table, kinematics, rng):
    goal = np.array([robot.gx - robot.px, robot.gy - robot.py])
    if script == "stop" or (script == "late" and t < 30):
        return 0
    if script == "random":
        return int(rng.randint(0, len(table)))
    if script in ("spin+", "spin-"):                 # the largest turn one way at the middle speed: theta leaves [0, 2 pi) often
        r = table[:, 1].max() if script == "spin+" else table[:, 1].min()
        return int(np.nonzero((table[:, 1] == r) & (table[:, 0] == np.sort(np.unique(table[:, 0]))[3]))[0][0])
    if kinematics == "holonomic":                    # greedy / late: the action that points most nearly at the goal
        return int(np.argmax(table @ goal))
    heading = robot.theta + table[:, 1]              # turn: the (v, r) whose new heading makes most progress towards the goal
    return int(np.argmax(table[:, 0] * (np.cos(heading) * goal[0] + np.sin(heading) * goal[1])))


def run_case(tag, kinematics, human_policy, script, case, scenario, H, constants, look_steps):
    """One trajectory, or None if some recorded step or lookahead has a margin below MIN_MARGIN."""
    env, robot, pol = _make_env(kinematics, scenario, H, constants)
    table = _table(pol, kinematics)
    env.reset("test", case)
    rng = np.random.RandomState(300 + case)
    if human_policy == "constant_velocity":          # the reference starts humans at rest: give them something to keep
        for h in env.humans:
            h.set_velocity(rng.uniform(-0.6, 0.6, 2))
    if human_policy != "linear":
        for h in env.humans:
            if human_policy == "given":
                h.act = lambda ob, rng=rng: ActionXY(*rng.uniform(-1, 1, 2))
            else:
                h.act = lambda ob, h=h: ActionXY(h.vx, h.vy)
    kw = dict(zip(("time_step", "time_limit", "success_reward", "collision_penalty", "discomfort_dist",
                   "discomfort_penalty_factor"), constants))
    R, Hs = [_full(robot)], [[_full(h) for h in env.humans]]
    acts, rew, done_l, info_l, dmin_l, times, hacts = [], [], [], [], [], [env.global_time], []
    look = {"reward": [], "done": [], "info": [], "humans": []}
    for t in range(MAX_STEPS):
        if t in look_steps:
            lr, ld, li, lh = [], [], [], []
            for ai in range(len(table)):
                a = _action(table, ai, kinematics)
                if so.step(R[-1], Hs[-1], table[ai], env.global_time, kinematics=kinematics, human_policy="given",
                           update=False, full=True, **kw)[7] < MIN_MARGIN:
                    return None
                ob, reward, done, info = env.onestep_lookahead(a)
                lr.append(float(reward))
                ld.append(int(done))
                li.append(INFO_CODES[str(info)])
                lh.append([[o.px, o.py, o.vx, o.vy, o.radius] for o in ob])
            for k, v in zip(("reward", "done", "info", "humans"), (lr, ld, li, lh)):
                look[k].append(v)
        ai = _choose(script, t, robot, table, kinematics, rng)
        if so.step(R[-1], Hs[-1], table[ai], env.global_time, kinematics=kinematics, human_policy="given", update=False,
                   full=True, **kw)[7] < MIN_MARGIN:
            return None
        _, reward, done, info = env.step(_action(table, ai, kinematics))
        acts.append(ai)
        rew.append(float(reward))
        done_l.append(int(done))
        info_l.append(INFO_CODES[str(info)])
        dmin_l.append(float(info.min_dist) if str(info) == "Discomfort" else np.nan)
        R.append(_full(robot))
        Hs.append([_full(h) for h in env.humans])
        hacts.append([[h.vx, h.vy] for h in env.humans])          # Agent.step stores the action as the new velocity
        times.append(env.global_time)
        if done:
            break
    k = "modes.%s." % tag
    out = {k + "robot": np.array(R, np.float64), k + "humans": np.array(Hs, np.float64), k + "actions": np.array(acts, np.int64),
           k + "reward": np.array(rew, np.float64), k + "done": np.array(done_l, np.int64), k + "info": np.array(info_l, np.int64),
           k + "dmin": np.array(dmin_l, np.float64), k + "time": np.array(times, np.float64),
           k + "human_actions": np.array(hacts, np.float64), k + "constants": np.array(constants, np.float64)}
    if look_steps:
        assert len(look["reward"]) == len(look_steps) == 3, (tag, len(acts), look_steps)      # every step lies inside the trajectory
        out[k + "look_steps"] = np.array(look_steps, np.int64)
        out[k + "look_reward"] = np.array(look["reward"], np.float64)
        out[k + "look_done"] = np.array(look["done"], np.int64)
        out[k + "look_info"] = np.array(look["info"], np.int64)
        out[k + "look_humans"] = np.array(look["humans"], np.float64)
    out["modes.table." + kinematics] = table
    return out


def build():
    JointState.self_state = property(lambda self_: self_.robot_state)
    out, meta = {}, []
    try:
        for tag, kinematics, human_policy, script, case, scenario, H, constants, look_steps in CASES:
            for _ in range(10):
                got = run_case(tag, kinematics, human_policy, script, case, scenario, H, constants, look_steps)
                if got is not None:
                    break
                case += 100
            else:
                raise RuntimeError("no case of %s keeps its margin" % tag)
            out.update(got)
            meta.append("|".join(str(x) for x in (tag, kinematics, human_policy, script, "test", case, scenario, H)))
    finally:
        del JointState.self_state
    out["modes_cases"] = np.array(meta)
    # every outcome at least twice over the file and at least once with a unicycle robot
    for code in range(5):
        n = sum(int((out["modes.%s.info" % m.split("|")[0]] == code).sum()) for m in meta)
        n_uni = sum(int((out["modes.%s.info" % m.split("|")[0]] == code).sum()) for m in meta if m.split("|")[1] == "unicycle")
        assert n >= 2 and n_uni >= 1, (code, n, n_uni)
    looks = np.concatenate([out[k].ravel() for k in out if k.endswith(".look_info")])
    assert sum(k.endswith(".look_info") for k in out) == 4 and np.all(np.bincount(looks, minlength=5) >= 2), np.bincount(looks)
    return out


if __name__ == "__main__":
    target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sim_modes.npz")
    built = build()
    np.savez_compressed(target, **built)
    for m in built["modes_cases"]:
        tag = str(m).split("|")[0]
        info = built["modes.%s.info" % tag]
        print("%-60s steps %3d  outcomes %s  last %d" % (m, len(info), np.bincount(info, minlength=5), info[-1]))
    print("wrote", target, os.path.getsize(target), "bytes")
