"""Generate tests/golden/orca.npz: the reference's own CrowdSim stepped with ORCA crowds (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_orca.py [OUT.npz]

The reference's ORCA / CentralizedORCA `import rvo2`, which is not installable here.  `tests/orca_cpu.py` -- the numpy
float32 restatement of the device kernel, with Python-RVO2's method names -- is put into sys.modules["rvo2"] before the
reference is imported (ref_loader only stubs modules that are missing), and the reference's CrowdSim.reset / step then run
unchanged.  What the fixture pins is therefore the reference's wrapper and environment semantics around RVO2: agent order,
radii (+ 0.01 + safety_space), preferred velocities, robot visibility and the `[:-1]` that drops the robot's action, the
max_speed of every agent, decentralized vs centralized planning, and the order of ORCA, collision test and motion in a step.
RVO2's numerics themselves rest on the algorithm's statement in csrc/rgl_orca.hip and on the property tests of
tests/test_orca_cpu.py, not on this file.  Each case runs in a fresh CrowdSim, so no planner carries its RVO2 agents (and
their radii) over from an earlier case.

Per case `orca.<tag>.`: robot (T+1, 9) and humans (T+1, H, 9) full states (px, py, vx, vy, radius, gx, gy, v_pref, theta),
human_vel (T, H, 2) the humans' ORCA velocities of each step, robot_vel (T, 2) the robot's action, reward / info / done (T,),
time (T+1,); `orca_cases` lists "tag|phase|case|scenario|H|visible|centralized|randomize|robot|safety_space".
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import orca_cpu  # noqa: E402

sys.modules["rvo2"] = orca_cpu
import ref_loader  # noqa: E402

policy_factory = ref_loader.load_reference()

from crowd_sim.envs.utils.action import ActionXY  # noqa: E402

INFO_CODES = {"": 0, "Discomfort": 1, "Collision": 2, "Reaching goal": 3, "Timeout": 4}

# (tag, phase, case, scenario, humans, robot visible, centralized, randomize, robot driver, safety_space)
CASES = ([("inv%d" % k, "test", k, "circle_crossing", 5, False, True, False, "table", 0.0) for k in range(8)] +
         [("vis%d" % k, "test", k, "circle_crossing", 5, True, True, False, "table", 0.0) for k in range(8)] +
         [("square12", "test", 3, "square_crossing", 12, True, True, False, "table", 0.0),
          ("decent_rand", "test", 2, "circle_crossing", 5, False, False, True, "table", 0.0)] +
         [("il%d" % k, "train", k, "circle_crossing", 5, False, True, False, "orca", 0.15) for k in range(3)])


def _full(agent):
    return [agent.px, agent.py, agent.vx, agent.vy, agent.radius, agent.gx, agent.gy, agent.v_pref, agent.theta]


def run_case(tag, phase, case, scenario, H, visible, centralized, randomize, driver, safety):
    import gym
    from crowd_sim.envs.utils.robot import Robot
    envc = importlib.import_module("crowd_nav.configs.icra_benchmark.mp_separate").EnvConfig()
    envc.sim.test_scenario = envc.sim.train_val_scenario = scenario
    envc.sim.human_num = H
    envc.sim.centralized_planning = centralized
    envc.env.randomize_attributes = randomize
    envc.robot.visible = visible
    envc.humans.policy = "orca"
    env = gym.make("CrowdSim-v0")
    env.configure(envc)
    robot = Robot(envc, "robot")
    robot.time_step = env.time_step
    mp = policy_factory["model_predictive_rl"]()
    mp.configure(importlib.import_module("crowd_nav.configs.icra_benchmark.mp_separate").PolicyConfig())
    mp.build_action_space(1.0)
    table = np.array([[a.vx, a.vy] for a in mp.action_space], np.float64)
    if driver == "orca":
        pol = policy_factory["orca"]()
        pol.multiagent_training = True
        pol.safety_space = safety
        robot.set_policy(pol)
    else:
        robot.set_policy(mp)
    env.set_robot(robot)
    ob = env.reset(phase, case)
    R, Hs, hv, rv, rew, info_l, done_l, times = [_full(robot)], [[_full(h) for h in env.humans]], [], [], [], [], [], [0.0]
    for t in range(200):
        if driver == "orca":
            action = robot.act(ob)
        else:                                    # the action of the table that points most nearly at the goal
            ai = int(np.argmax(table @ np.array([robot.gx - robot.px, robot.gy - robot.py])))
            action = ActionXY(np.float64(table[ai, 0]), np.float64(table[ai, 1]))
        ob, reward, done, info = env.step(action)
        rv.append([action.vx, action.vy])
        hv.append([[h.vx, h.vy] for h in env.humans])     # Agent.step stores the action as the new velocity
        rew.append(float(reward))
        info_l.append(INFO_CODES[str(info)])
        done_l.append(int(done))
        R.append(_full(robot))
        Hs.append([_full(h) for h in env.humans])
        times.append(env.global_time)
        if done:
            break
    k = "orca.%s." % tag
    return {k + "robot": np.array(R, np.float64), k + "humans": np.array(Hs, np.float64),
            k + "human_vel": np.array(hv, np.float64), k + "robot_vel": np.array(rv, np.float64),
            k + "reward": np.array(rew, np.float64), k + "info": np.array(info_l, np.int64),
            k + "done": np.array(done_l, np.int64), k + "time": np.array(times, np.float64)}


def build():
    np.random.seed(0)
    out, meta = {}, []
    for c in CASES:
        out.update(run_case(*c))
        meta.append("|".join(str(int(x)) if isinstance(x, bool) else str(x) for x in c))
    out["orca_cases"] = np.array(meta)
    return out


if __name__ == "__main__":
    target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "orca.npz")
    np.savez_compressed(target, **build())
    print("wrote", target, os.path.getsize(target), "bytes")
