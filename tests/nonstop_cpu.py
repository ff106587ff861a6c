"""Host replay of the simulator step with nonstop humans -- what csrc/rgl_nonstop.hip is written from and what the nonstop tests
compare the device with.

Upstream's CrowdSim.step(update=True) with sim.nonstop_human on (crowd_sim/envs/crowd_sim.py:346-349): the robot steps, then
`for human, action in zip(humans, actions): human.step(action); if human.reached_destination(): generate_human(human)`.
Restated over the sequential python-float step of oracle/sim_oracle.py (robot, ladder, human actions), the plain-integer numpy
stream of tests/scenegen_cpu.MT19937 and, for whole exploring episodes, tests/explore_cpu.ExploreStream's decision on the same
stream object.

`step(...)` is one step of one environment and reports, besides the new state, every regeneration as (human, attempts, doubles)
and the step's smallest MARGIN: sim_oracle's margin of the ladder, |distance - radius| of every arrival test and
|distance - clearance| of every clearance test made (all agents of every attempt, also those upstream's loop would not reach after
its first hit: the device evaluates them all).  `variant` breaks one of upstream's quirks on purpose, for the tests that show the
fixture can tell: "all_first" steps every human before any regeneration, "no_self" leaves the arriving human out of its own
clearance list.
"""
import numpy as np

from oracle import sim_oracle as so
from tests.scenegen_cpu import MT19937

VARIANTS = (None, "all_first", "no_self")


def stream_from_words(words):
    """The MT19937 whose 625 state words (624 words, position) are `words`; its draw counter starts at 0."""
    w = np.asarray(words).astype(np.uint32)
    rs = MT19937.__new__(MT19937)
    rs.mt, rs.pos, rs.draws = [int(x) for x in w[:624]], int(w[624]), 0
    return rs


def words_of(rs):
    return np.array(list(rs.mt) + [rs.pos], dtype=np.uint32)


def seeded_stream(seed, draws):
    """np.random.seed(seed) after `draws` doubles: where a case's scene leaves its stream."""
    rs = MT19937(int(seed))
    for _ in range(int(draws)):
        rs.random_sample()
    return rs


class CountingMT(MT19937):
    """MT19937 that counts its twists, so that a step can say which of its draws crossed a 624-word block."""
    twists = 0

    def _twist(self):
        self.twists += 1
        MT19937._twist(self)


def counting_stream(seed, words):
    """np.random.seed(seed) after `words` 32-bit outputs (odd counts too: `choice` takes single words)."""
    rs = CountingMT(int(seed))
    for _ in range(int(words)):
        rs.next_u32()
    return rs


class Margin(object):
    def __init__(self):
        self.value = np.inf
        self.twists = {"policy": 0, "attributes": 0, "place": 0}

    def see(self, gap):
        self.value = min(self.value, float(np.min(np.abs(gap))))


def regenerate(cfg, rs, agents, v_pref, radius, me, margin, max_attempts=None):
    """generate_human(human) against `agents` ((n, 5) rows px, py, gx, gy, radius; row `me` is the human itself, or None when it
    is left out).  Returns (placed, px, py, gx, gy, v_pref, radius, attempts); margin.twists counts, for a CountingMT, the twists
    met while the attributes were drawn and while the human was placed."""
    ag = np.array(agents, np.float64)
    t0 = getattr(rs, "twists", 0)
    if cfg.randomize_attributes:
        v_pref = rs.uniform(0.5, 1.5)
        radius = rs.uniform(0.3, 0.5)
        if me is not None:
            ag[me, 4] = radius                       # the list holds the human itself, already with its new radius
    t1 = getattr(rs, "twists", 0)
    margin.twists["attributes"] += t1 - t0
    try:
        return _place(cfg, rs, ag, v_pref, radius, margin, max_attempts)
    finally:
        margin.twists["place"] += getattr(rs, "twists", 0) - t1


def _place(cfg, rs, ag, v_pref, radius, margin, max_attempts):
    attempts = [0]

    def clear_of(x, y, cx, cy):
        dx, dy = x - cx, y - cy
        dist, clearance = np.sqrt(dx * dx + dy * dy), radius + ag[:, 4] + cfg.discomfort_dist
        margin.see(dist - clearance)
        return not bool((dist < clearance).any())

    def attempt():
        if max_attempts is not None and attempts[0] >= max_attempts:
            return False
        attempts[0] += 1
        return True
    R = cfg.circle_radius
    if cfg.scenario == "circle_crossing":
        while True:
            if not attempt():
                return False, None, None, None, None, v_pref, radius, attempts[0]
            angle = rs.random_sample() * np.pi * 2
            px_noise = (rs.random_sample() - 0.5) * v_pref
            py_noise = (rs.random_sample() - 0.5) * v_pref
            px = R * np.cos(angle) + px_noise
            py = R * np.sin(angle) + py_noise
            # both tests of every agent, as one expression each (upstream's `or` per agent decides the same)
            a, b = clear_of(px, py, ag[:, 0], ag[:, 1]), clear_of(px, py, ag[:, 2], ag[:, 3])
            if a and b:
                break
        gx, gy = -px, -py
    elif cfg.scenario == "square_crossing":
        sign = -1 if rs.random_sample() > 0.5 else 1
        while True:
            if not attempt():
                return False, None, None, None, None, v_pref, radius, attempts[0]
            px = rs.random_sample() * cfg.square_width * 0.5 * sign
            py = (rs.random_sample() - 0.5) * cfg.square_width
            if clear_of(px, py, ag[:, 0], ag[:, 1]):
                break
        while True:
            if not attempt():
                return False, None, None, None, None, v_pref, radius, attempts[0]
            gx = rs.random_sample() * cfg.square_width * 0.5 * -sign
            gy = (rs.random_sample() - 0.5) * cfg.square_width
            if clear_of(gx, gy, ag[:, 2], ag[:, 3]):
                break
    else:
        raise NotImplementedError(cfg.scenario)
    return True, px, py, gx, gy, v_pref, radius, attempts[0]


def step(cfg, robot, humans, goals, vpref, action, time, rs, policy_draws=1, kinematics="holonomic", human_policy="linear",
         human_actions=None, done=False, variant=None, max_attempts=None):
    """One step of one environment.  robot (9,), humans (H, 5), goals (H, 2), vpref (H,), action (2,), `rs` the environment's
    stream (advanced in place).  Returns a dict: robot, humans, goals, vpref, time, reward, done, info, dmin (what the device
    reports: -1 after a collision), events [(human, attempts, doubles)], attempts (H,), status (1: some regeneration reached
    max_attempts; that human stays where its step left it), margin, twists (module docstring of CountingMT)."""
    assert variant in VARIANTS
    robot, humans = np.array(robot, np.float64), np.array(humans, np.float64)
    goals, vpref = np.array(goals, np.float64), np.array(vpref, np.float64)
    H = humans.shape[0]
    out = {"robot": robot, "humans": humans, "goals": goals, "vpref": vpref, "time": float(time), "reward": 0.0, "done": True,
           "info": so.INFO_DONE, "dmin": np.inf, "events": [], "attempts": np.zeros(H, np.int64), "status": 0, "margin": np.inf,
           "twists": {"policy": 0, "attributes": 0, "place": 0}}
    if done:
        return out
    margin = Margin()
    t0 = getattr(rs, "twists", 0)
    for _ in range(int(policy_draws)):
        rs.random_sample()
    margin.twists["policy"] = getattr(rs, "twists", 0) - t0
    full = [list(humans[h]) + [goals[h, 0], goals[h, 1], vpref[h], 0.0] for h in range(H)]
    nr, nh, reward, fin, info, _, last_dmin, step_margin = so.step(
        list(robot), full, (float(action[0]), float(action[1])), float(time), time_step=cfg.time_step, time_limit=cfg.time_limit,
        success_reward=cfg.success_reward, collision_penalty=cfg.collision_penalty, discomfort_dist=cfg.discomfort_dist,
        discomfort_penalty_factor=cfg.discomfort_penalty_factor, kinematics=kinematics, human_policy=human_policy,
        human_actions=None if human_actions is None else [tuple(a) for a in np.asarray(human_actions, np.float64)], full=True)
    margin.see(step_margin)
    moved = np.array([g[:5] for g in nh], np.float64)
    new = humans.copy()                              # upstream's list of humans while its loop runs
    if variant == "all_first":
        new[:] = moved
    for i in range(H):
        new[i] = moved[i]
        dx, dy = new[i, 0] - goals[i, 0], new[i, 1] - goals[i, 1]
        dist = np.sqrt(dx * dx + dy * dy)
        margin.see(dist - new[i, 4])
        if not dist < new[i, 4]:
            continue
        rows = [(nr[0], nr[1], nr[5], nr[6], nr[4])] + [(new[j, 0], new[j, 1], goals[j, 0], goals[j, 1], new[j, 4]) for j in range(H)]
        me = 1 + i
        if variant == "no_self":
            del rows[me]
            me = None
        before = rs.draws
        placed, px, py, gx, gy, vp, radius, attempts = regenerate(cfg, rs, rows, vpref[i], new[i, 4], me, margin, max_attempts)
        out["events"].append((i, attempts, rs.draws - before))
        out["attempts"][i] = attempts
        vpref[i], new[i, 4] = vp, radius
        if placed:
            new[i, :4] = (px, py, 0.0, 0.0)
            goals[i] = (gx, gy)
        else:
            out["status"] = 1
    out.update(robot=np.array(nr, np.float64), humans=new, time=float(time) + cfg.time_step, reward=float(reward), done=bool(fin),
               info=int(info), dmin=float(last_dmin), margin=margin.value, twists=margin.twists)
    return out


def run_script(cfg, phase, case, actions, policy_draws, kinematics="holonomic", variant=None, draws_offset=0):
    """A seeded case under a scripted robot: actions (T, 2).  Returns (states, log): states = per step (robot, humans, goals,
    vpref) after it, preceded by the scene; log = dict of per-step reward / done / info / dmin / time / margin lists, events
    [(step, human, attempts, doubles)] and the stream's final doubles count.  draws_offset is added to policy_draws."""
    from relationalgraphlearning_amd.sim import BASE_SEED, generate_scene_with_draws
    robot, humans, goals, vpref, draws = generate_scene_with_draws(cfg, phase, case)
    rs = seeded_stream(BASE_SEED[phase] + case, draws)
    states = [(robot, humans, goals, vpref)]
    log = {"reward": [], "done": [], "info": [], "dmin": [], "time": [0.0], "margin": [], "events": []}
    t_now = 0.0
    for t, a in enumerate(np.asarray(actions, np.float64)):
        o = step(cfg, robot, humans, goals, vpref, a, t_now, rs, policy_draws=policy_draws + draws_offset, kinematics=kinematics,
                 variant=variant)
        robot, humans, goals, vpref, t_now = o["robot"], o["humans"], o["goals"], o["vpref"], o["time"]
        states.append((robot, humans, goals, vpref))
        for k in ("reward", "done", "info", "dmin", "margin"):
            log[k].append(o[k])
        log["time"].append(t_now)
        log["events"].extend((t, h, n, d) for h, n, d in o["events"])
        if o["done"]:
            break
    log["draws"] = rs.draws
    log["stream"] = rs
    return states, log
