"""Inputs of the nonstop kernel's step-by-step test (tests/test_nonstop_gpu.py) and their host replay, shared with the CPU test that
holds the inputs to what they claim (tests/test_nonstop_cases_cpu.py).

A batch is B = 67 loaded states of one configuration (H humans, scenario, randomize_attributes, policy_draws) for ROUNDS successive
steps.  Every round starts from the replay's own state after the previous one -- so the device's one-ulp sin / cos cannot
accumulate -- with a fresh set of humans put one step from their goals: environment b gets b % 4 of them (fewer when H is smaller),
so that steps with one, two and three arrivals occur beside steps with none.  The streams start at word 612 + b % 13 of their first
block (612 .. 624: up to six words of policy draws, four of a randomize draw and six of a circle's attempt fit before its end), so
that in every configuration the policy's skip, a randomize draw and a regeneration each cross the twist somewhere in the batch; the
second round meets them in the middle of a block.  Environments with b % 11 == 5 are finished from the start.  A regeneration gets
MAX_ATTEMPTS attempts: upstream's loop has no exit, and 19 humans with randomised radii leave no room on the 4 m circle, so those
regenerations end at the cap, on the host and on the device alike.
"""
import numpy as np

from relationalgraphlearning_amd.sim import SimConfig, generate_scene
from tests import nonstop_cpu as nc

B, ROUNDS, MAX_ATTEMPTS = 67, 2, 300
CONFIGS = [(H, scenario, rand, draws) for H in (1, 5, 19) for scenario in ("circle_crossing", "square_crossing")
           for rand in (False, True) for draws in (0, 1, 3)]
_built = {}


def config(H, scenario, rand):
    return SimConfig(scenario=scenario, human_num=H, randomize_attributes=rand, nonstop_human=True, square_width=10,
                     scene_max_attempts=MAX_ATTEMPTS)


def _near_goals(rng, humans, goals, vpref, count):
    """Put `count` humans 0.4 m from their goals: one step of v_pref * 0.25 (0.125 .. 0.375 m) leaves them 0.025 .. 0.275 m from it,
    inside every radius (0.3 .. 0.5 m)."""
    H = len(humans)
    for h in rng.choice(H, size=min(count, H), replace=False):
        phi = rng.uniform(0, 2 * np.pi)
        humans[h, 0], humans[h, 1] = goals[h, 0] + 0.4 * np.cos(phi), goals[h, 1] + 0.4 * np.sin(phi)


def build(H, scenario, rand, draws):
    """[round][b] -> (inputs, replayed output): inputs = dict(robot, humans, goals, vpref, action, time, done, words)."""
    key = (H, scenario, rand, draws)
    if key in _built:
        return _built[key]
    cfg = config(H, scenario, rand)
    rng = np.random.RandomState(100 * H + 10 * draws + 2 * int(rand) + int(scenario == "square_crossing"))
    state = []
    for b in range(B):
        # the scene with fixed attributes: the host generator has no cap, and 19 randomised radii may never fit the circle
        robot, humans, goals, vpref = generate_scene(config(H, scenario, False), "test", b)
        state.append(dict(robot=robot, humans=humans, goals=goals, vpref=vpref, time=0.25 * (b % 5), done=b % 11 == 5,
                          rs=nc.counting_stream(3000 + b, 612 + b % 13)))
    rounds = []
    for _ in range(ROUNDS):
        this = []
        for b, s in enumerate(state):
            humans = s["humans"].copy()
            _near_goals(rng, humans, s["goals"], s["vpref"], b % 4)
            action = rng.uniform(-0.5, 0.5, 2)
            inputs = dict(robot=s["robot"], humans=humans, goals=s["goals"], vpref=s["vpref"], action=action, time=s["time"],
                          done=s["done"], words=nc.words_of(s["rs"]))
            out = nc.step(cfg, s["robot"], humans, s["goals"], s["vpref"], action, s["time"], s["rs"], policy_draws=draws, done=s["done"],
                          max_attempts=MAX_ATTEMPTS)
            out["words"] = nc.words_of(s["rs"])
            this.append((inputs, out))
            s.update(robot=out["robot"], humans=out["humans"], goals=out["goals"], vpref=out["vpref"], time=out["time"],
                     done=out["done"])
        rounds.append(this)
    _built[key] = rounds
    return rounds


def census(rounds):
    """What a batch met: steps by number of arrivals, twists by where they fell, finished environments, rejected attempts and the
    smallest margin."""
    met = {"arrivals": {}, "policy": 0, "attributes": 0, "place": 0, "finished": 0, "rejected": 0, "capped": 0, "margin": np.inf}
    for this in rounds:
        for inputs, out in this:
            if inputs["done"]:
                met["finished"] += 1
                continue
            n = len(out["events"])
            met["arrivals"][n] = met["arrivals"].get(n, 0) + 1
            for k in ("policy", "attributes", "place"):
                met[k] += out["twists"][k]
            met["rejected"] += sum(a - 1 for _, a, _ in out["events"])
            met["capped"] += out["status"]
            met["margin"] = min(met["margin"], out["margin"])
    return met
