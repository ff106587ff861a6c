"""Generate tests/golden/nonstop.npz: the reference's own CrowdSim with sim.nonstop_human on (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nonstop.py [OUT.npz]

Scripted trajectories (`ns.<tag>.`): linear humans, a holonomic robot scripted from a PRIVATE RandomState (it mostly stands and now
and then takes a random action of the table; numpy's global stream, the one CrowdSim seeds per case and regenerates humans from, is
never touched by the script) -- except that in the trajectories with draws = 1 the script calls `np.random.random()` once before
every `env.step`, the draw `predict` would make (model_predictive_rl.py:208).  Every double taken from the global stream is counted
by wrapping np.random.random / np.random.uniform on the numpy module while the episode runs; the doubles a `generate_human(human)`
call took give its attempts.  Nothing of the reference is changed on disk or copied: the file holds states, actions, settings and
outcomes only.

Per trajectory: robot (T+1, 9) and humans (T+1, H, 9) full states (px, py, vx, vy, radius, gx, gy, v_pref, theta), actions (T, 2)
velocities, reward / done / info / dmin (T,) (dmin: Discomfort.min_dist, NaN otherwise), time (T+1,), events (E, 4) =
(step, human, attempts, doubles) of every regeneration in upstream's order, draws_end = doubles taken from the case's stream since
its seed (scene, script draws, regenerations).  `ns_cases` lists "tag|scenario|H|randomize|circle_radius|time_limit|draws|case".

Exploring episodes (`nx.`): make_golden_explore.py's family -- the reference Explorer, ModelPredictiveRL (weights_goal.npz, depth 1),
epsilon 0.3, 1.5 m circle, 12 s, `train` phase -- with nonstop_human on; cases by the same rule (every greedy decision's top two root
values at least 1e-4 apart).  The arrays of explore.npz plus events (E, 5) = (case index, step, human, attempts, doubles) and
draws_end per case.

Asserted here: the host replay (tests/nonstop_cpu.py) reproduces every trajectory; no clearance or arrival test of it lies within
1e-9 of its threshold (a case that has one is replaced by the next case); the replay with all humans stepped before any regeneration, or
with the arriving human left out of its own clearance list, does not reproduce the trajectories named in TEETH; the file holds at least 50 rejected attempts, 5 steps in
which two humans of one environment arrive, one regeneration that crosses a 624-word block of the stream and 3 explored decisions
followed by a regeneration in the same episode.
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

from crowd_sim.envs.utils.action import ActionXY  # noqa: E402
from crowd_sim.envs.utils.state import JointState  # noqa: E402

from oracle import rgl_oracle as orc  # noqa: E402
from relationalgraphlearning_amd.sim import BASE_SEED, SimConfig, generate_scene_with_draws  # noqa: E402
from tests import explore_cpu as xc  # noqa: E402
from tests import golden_io as gio  # noqa: E402
from tests import nonstop_cpu as nc  # noqa: E402

INFO_CODES = {"": 0, "Discomfort": 1, "Collision": 2, "Reaching goal": 3, "Timeout": 4}
MIN_MARGIN = 1e-9
# tag, scenario, H, randomize_attributes, circle_radius, time_limit, draws per decision, first case
SCRIPTED = [
    ("circle5", "circle_crossing", 5, False, 4.0, 30, 1, 0),
    ("circle5_rand", "circle_crossing", 5, True, 4.0, 30, 1, 1),
    ("square5", "square_crossing", 5, False, 4.0, 30, 0, 2),
    ("circle1", "circle_crossing", 1, False, 4.0, 30, 1, 3),
    ("circle10", "circle_crossing", 10, False, 4.0, 20, 1, 4),
    ("tight5", "circle_crossing", 5, False, 1.5, 12, 0, 5),
]
# trajectories that must tell upstream's human order and the human in its own clearance list from their alternatives: the replay
# with tests/nonstop_cpu.py's variant must NOT reproduce them (the next case is taken until it does not)
TEETH = {"tight5": ("all_first", "no_self"), "circle10": ("no_self",)}
EPSILON, N_EXPLORING, MIN_GAP = 0.3, 6, 1e-4
X_CIRCLE_RADIUS, X_TIME_LIMIT = 1.5, 12


class Counter(object):
    """np.random.random / np.random.uniform of the numpy module behind a counter of doubles, while installed."""

    def __init__(self):
        self.doubles = 0
        self.random0, self.uniform0 = np.random.random, np.random.uniform

    def install(self):
        def random(*a):
            assert not a
            self.doubles += 1
            return self.random0()

        def uniform(lo, hi):
            self.doubles += 1
            return self.uniform0(lo, hi)
        np.random.random, np.random.uniform = random, uniform

    def remove(self):
        np.random.random, np.random.uniform = self.random0, self.uniform0


def _full(agent):
    return [agent.px, agent.py, agent.vx, agent.vy, agent.radius, agent.gx, agent.gy, agent.v_pref, agent.theta]


def _env_config(scenario, H, randomize, circle_radius, time_limit):
    mod = importlib.import_module("crowd_nav.configs.icra_benchmark.mp_separate")
    envc = mod.EnvConfig()
    envc.humans.policy = "linear"
    envc.sim.centralized_planning = False
    envc.sim.nonstop_human = True
    envc.sim.test_scenario = envc.sim.train_val_scenario = scenario
    envc.sim.human_num, envc.sim.circle_radius = H, circle_radius
    envc.env.time_limit, envc.env.randomize_attributes = time_limit, randomize
    return mod, envc


def _make_env(envc, mod):
    import gym
    from crowd_sim.envs.utils.robot import Robot
    env = gym.make("CrowdSim-v0")
    env.configure(envc)
    robot = Robot(envc, "robot")
    robot.time_step = env.time_step
    pol = policy_factory["model_predictive_rl"]()
    pol.configure(mod.PolicyConfig())
    robot.set_policy(pol)
    env.set_robot(robot)
    return env, robot, pol


def _watch_regenerations(env, counter, events, step_of):
    """Wrap env.generate_human so that every call with a human logs (step, human index, doubles)."""
    gen0 = env.generate_human

    def generate_human(human=None):
        before = counter.doubles
        out = gen0(human)
        if human is not None:
            events.append((step_of(), env.humans.index(human), counter.doubles - before))
        return out
    env.generate_human = generate_human


def _attempts(doubles, scenario, randomize):
    d = doubles - (2 if randomize else 0)
    if scenario == "circle_crossing":
        assert d % 3 == 0
        return d // 3
    assert (d - 1) % 2 == 0
    return (d - 1) // 2


def _sim_config(scenario, H, randomize, circle_radius, time_limit):
    return SimConfig(scenario=scenario, human_num=H, randomize_attributes=randomize, circle_radius=circle_radius,
                     time_limit=time_limit, nonstop_human=True)


def run_scripted(tag, scenario, H, randomize, circle_radius, time_limit, draws, case):
    """One trajectory, or None if the replay sees a margin below MIN_MARGIN."""
    mod, envc = _env_config(scenario, H, randomize, circle_radius, time_limit)
    env, robot, pol = _make_env(envc, mod)
    pol.build_action_space(1.0)
    table = np.array([[a.vx, a.vy] for a in pol.action_space], np.float64)
    rng = np.random.RandomState(700 + case)                  # the script's own stream
    counter, events, steps = Counter(), [], [0]
    counter.install()
    try:
        env.reset("test", case)
        _watch_regenerations(env, counter, events, lambda: steps[0])
        R, Hs, acts, rew, done_l, info_l, dmin_l, times = [_full(robot)], [[_full(h) for h in env.humans]], [], [], [], [], [], [0.0]
        for t in range(int(time_limit / env.time_step) + 2):
            steps[0] = t
            a = table[int(rng.randint(0, len(table)))] if rng.random_sample() < 0.3 else table[0]
            for _ in range(draws):
                np.random.random()                           # predict's `probability = np.random.random()`
            _, reward, done, info = env.step(ActionXY(np.float64(a[0]), np.float64(a[1])))
            acts.append(a)
            rew.append(float(reward))
            done_l.append(int(done))
            info_l.append(INFO_CODES[str(info)])
            dmin_l.append(float(info.min_dist) if str(info) == "Discomfort" else np.nan)
            R.append(_full(robot))
            Hs.append([_full(h) for h in env.humans])
            times.append(env.global_time)
            if done:
                break
        draws_end = counter.doubles
    finally:
        counter.remove()
    ev = np.array([(t, h, _attempts(d, scenario, randomize), d) for t, h, d in events], np.int64).reshape(-1, 4)
    # the replay on the same script: equal, and no decision near its threshold
    scfg = _sim_config(scenario, H, randomize, circle_radius, time_limit)
    states, log = nc.run_script(scfg, "test", case, np.array(acts), draws)
    if min(log["margin"]) < MIN_MARGIN:
        return None
    Hs_a = np.array(Hs, np.float64)
    assert len(states) == len(R) and log["draws"] == draws_end, (tag, len(states), len(R), log["draws"], draws_end)
    assert [tuple(e) for e in ev.tolist()] == [tuple(e) for e in log["events"]], tag
    assert np.array_equal(np.array([s[1] for s in states]), Hs_a[:, :, :5]) and np.array_equal(np.array([s[2] for s in states]), Hs_a[:, :, 5:7])
    for variant in TEETH.get(tag, ()):
        v_states, v_log = nc.run_script(scfg, "test", case, np.array(acts), draws, variant=variant)
        if (len(v_states) == len(states) and v_log["events"] == log["events"]
                and np.array_equal(np.array([s[1] for s in v_states]), Hs_a[:, :, :5])):
            return None
    k = "ns.%s." % tag
    return {k + "robot": np.array(R, np.float64), k + "humans": Hs_a, k + "actions": np.array(acts, np.float64),
            k + "reward": np.array(rew, np.float64), k + "done": np.array(done_l, np.int64), k + "info": np.array(info_l, np.int64),
            k + "dmin": np.array(dmin_l, np.float64), k + "time": np.array(times, np.float64), k + "events": ev,
            k + "draws_end": np.array(draws_end, np.int64)}


def build_exploring(candidates=range(0, 400)):
    from crowd_sim.envs.utils.info import ReachGoal, Collision
    from crowd_nav.utils.explorer import Explorer
    from crowd_nav.utils.memory import ReplayMemory
    mod, envc = _env_config("circle_crossing", 5, False, X_CIRCLE_RADIUS, X_TIME_LIMIT)
    env, robot, pol = _make_env(envc, mod)
    pol.load_state_dict(gio.checkpoint("goal"))
    pol.set_device(torch.device("cpu"))
    pol.set_time_step(env.time_step)
    pol.set_epsilon(EPSILON)
    ve_fwd = pol.value_estimator.forward
    pol.value_estimator.forward = lambda state: ve_fwd(state).reshape(())        # scalar-shape shim (make_golden.py's header)
    memory = ReplayMemory(100000)
    explorer = Explorer(env, robot, torch.device("cpu"), None, memory, 0.9, target_policy=pol)
    params, ocfg = gio.oracle_params("goal"), orc.OracleConfig()
    scfg = _sim_config("circle_crossing", 5, False, X_CIRCLE_RADIUS, X_TIME_LIMIT)

    log = {}
    counter = Counter()
    act0, step0, choice0 = robot.act, env.step, np.random.choice

    def act(ob):
        log["roots"].append((robot.get_full_state(), list(ob)))
        log["deciding"] = True
        before = counter.doubles
        a = act0(ob)
        log["deciding"] = False
        assert counter.doubles == before + 1                             # one decision, one double
        table = [(x.vx, x.vy) for x in pol.action_space]
        log["actions"].append(table.index((a.vx, a.vy)))
        if len(log["choice"]) < len(log["actions"]):
            log["choice"].append(-1)
        return a

    def step(action, update=True):
        if update:
            log["step"] = len(log["actions"]) - 1
        ob, reward, done, info = step0(action, update)
        if done and update:
            log["end"] = (3 if isinstance(info, ReachGoal) else (2 if isinstance(info, Collision) else 4), env.global_time)
        return ob, reward, done, info

    def choice(n):
        c = choice0(n)
        log["choice"].append(int(c))
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
    JointState.self_state = property(lambda self_: self_.robot_state)
    robot.act, env.step, np.random.choice = act, step, choice
    counter.install()
    _watch_regenerations(env, counter, log.setdefault("events_all", []), lambda: log["step"])
    try:
        with torch.no_grad():
            for case in candidates:
                log.update(roots=[], choice=[], actions=[], end=None, deciding=False, step=-1)
                del log["events_all"][:]
                counter.doubles = 0
                env.case_counter["train"] = case
                n_before = len(memory.memory)
                explorer.run_k_episodes(1, "train", update_memory=True, episode=3)
                gap = smallest_gap()
                events = list(log["events_all"])
                explored_then_regenerated = sum(1 for i, c in enumerate(log["choice"]) if c >= 0 and any(e[0] >= i for e in events))
                print("case %d: %d decisions, %d explored, %d regenerations, outcome %d, %d tuples, smallest gap %.3e"
                      % (case, len(log["actions"]), sum(c >= 0 for c in log["choice"]), len(events), log["end"][0],
                         len(memory.memory) - n_before, gap))
                if gap < MIN_GAP or not events:
                    continue
                # the replay of this episode: the decisions on the stream, the regenerations, the margins
                r, h, g, v, d = generate_scene_with_draws(scfg, "train", case)
                st = xc.ExploreStream(BASE_SEED["train"] + case, d)
                table = np.array([(x.vx, x.vy) for x in pol.action_space], np.float64)
                t_now, ev, margin = 0.0, [], np.inf
                for t, (a, c) in enumerate(zip(log["actions"], log["choice"])):
                    chosen, explored = st.decide(a, len(table), EPSILON)
                    assert chosen == a and explored == int(c >= 0)
                    o = nc.step(scfg, r, h, g, v, table[a], t_now, st.rs, policy_draws=0)
                    r, h, g, v, t_now = o["robot"], o["humans"], o["goals"], o["vpref"], o["time"]
                    ev.extend((t, i, n, dd) for i, n, dd in o["events"])
                    margin = min(margin, o["margin"])
                assert o["done"] and o["info"] == log["end"][0] and t_now == log["end"][1]
                assert ev == [(t, i, dd // 3, dd) for t, i, dd in events], (ev, events)
                assert counter.doubles == d + len(log["actions"]) + sum(e[2] for e in events)      # scene, decisions, regenerations
                if margin < MIN_MARGIN:
                    continue
                kept.append(dict(case=case, gap=gap, actions=list(log["actions"]), choice=list(log["choice"]), end=log["end"],
                                 scene_draws=d, n_tuples=len(memory.memory) - n_before, events=ev,
                                 draws_end=counter.doubles, followed=explored_then_regenerated))
                if len(kept) == N_EXPLORING:
                    break
    finally:
        counter.remove()
        robot.act, env.step, np.random.choice = act0, step0, choice0
        del JointState.self_state
    assert len(kept) == N_EXPLORING
    cat = lambda name, dtype: np.array([x for k in kept for x in k[name]], dtype)      # noqa: E731
    events = np.array([(ci,) + tuple(e) for ci, k in enumerate(kept) for e in k["events"]], np.int64).reshape(-1, 5)
    return {"nx.cases": np.array([k["case"] for k in kept], np.int64), "nx.draws": np.array([k["scene_draws"] for k in kept], np.int64),
            "nx.epsilon": np.array(EPSILON), "nx.n_actions": np.array(len(pol.action_space), np.int64),
            "nx.actions": cat("actions", np.int64), "nx.choice": cat("choice", np.int64),
            "nx.steps_end": np.cumsum([len(k["actions"]) for k in kept]).astype(np.int64),
            "nx.outcome": np.array([k["end"][0] for k in kept], np.int64), "nx.time": np.array([k["end"][1] for k in kept], np.float64),
            "nx.n_tuples": np.array([k["n_tuples"] for k in kept], np.int64), "nx.events": events,
            "nx.draws_end": np.array([k["draws_end"] for k in kept], np.int64),
            "nx.followed": np.array([k["followed"] for k in kept], np.int64),
            "nx.min_gap": np.array(min(k["gap"] for k in kept)), "nx.circle_radius": np.array(X_CIRCLE_RADIUS),
            "nx.time_limit": np.array(float(X_TIME_LIMIT))}


def census(out):
    """(rejected attempts, steps with two arrivals in one environment, regenerations crossing a 624-word block) over the file."""
    rejected = double = 0
    for key in [k for k in out if k.endswith(".events")]:
        ev = out[key]
        rejected += int((ev[:, -2] - 1).sum()) if key.startswith("ns.") else int((ev[:, 3] - 1).sum())
        if key.startswith("ns."):
            steps = ev[:, 0]
        else:
            steps = ev[:, 0] * 100000 + ev[:, 1]
        double += int((np.bincount(np.unique(steps, return_inverse=True)[1]) >= 2).sum()) if len(ev) else 0
    return rejected, double


def crossings(out):
    """Regenerations of the scripted trajectories that cross a 624-word block: from the replay's stream positions."""
    n = 0
    for m in out["ns_cases"]:
        tag, scenario, H, rand, radius, limit, draws, case = str(m).split("|")
        scfg = _sim_config(scenario, int(H), rand == "True", float(radius), float(limit) if "." in limit else int(limit))
        d = generate_scene_with_draws(scfg, "test", int(case))[4]
        words, t_prev = 2 * d, -1
        for t, h, attempts, doubles in out["ns.%s.events" % tag]:
            words += 2 * int(draws) * (int(t) - t_prev)
            t_prev = int(t)
            n += int(words // 624 != (words + 2 * int(doubles) - 1) // 624)
            words += 2 * int(doubles)
    return n


def build():
    JointState.self_state = property(lambda self_: self_.robot_state)
    out, meta = {}, []
    try:
        for tag, scenario, H, randomize, radius, limit, draws, case in SCRIPTED:
            for _ in range(60):
                got = run_scripted(tag, scenario, H, randomize, radius, limit, draws, case)
                if got is not None and len(got["ns.%s.events" % tag]) >= 3:
                    break
                case += 10
            else:
                raise RuntimeError("no case of %s keeps its margin" % tag)
            out.update(got)
            meta.append("|".join(str(x) for x in (tag, scenario, H, randomize, radius, limit, draws, case)))
            ev = got["ns.%s.events" % tag]
            print("%-14s case %3d: %3d steps, last info %d, %3d regenerations, %4d rejected attempts, %d doubles"
                  % (tag, case, len(got["ns.%s.info" % tag]), got["ns.%s.info" % tag][-1], len(ev), int((ev[:, 2] - 1).sum()),
                     int(got["ns.%s.draws_end" % tag])))
    finally:
        del JointState.self_state
    out["ns_cases"] = np.array(meta)
    out.update(build_exploring())
    rejected, double = census(out)
    crossing = crossings(out)
    followed = int(out["nx.followed"].sum())
    print("rejected attempts %d, double arrivals %d, block crossings %d, explored decisions followed by a regeneration %d"
          % (rejected, double, crossing, followed))
    assert rejected >= 50 and double >= 5 and crossing >= 1 and followed >= 3
    return out


if __name__ == "__main__":
    target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "nonstop.npz")
    built = build()
    np.savez_compressed(target, **built)
    print("wrote", target, os.path.getsize(target), "bytes")
    assert os.path.getsize(target) < 400000
