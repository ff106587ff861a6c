"""Inputs for the simulator-step tests, drawn and checked on the CPU (no device needed): the seeded random batches of
tests/test_sim_gpu.py (b), the exact edges of (c) and the unicycle wraps of (d).  Every decision about what is drawn, what is
drawn again and what an edge must give is taken from the restatement (oracle/sim_oracle.py) alone."""
import numpy as np

from oracle import sim_oracle as so

MIN_MARGIN = 1e-9
TWO_PI = 2 * np.pi
CONSTANT_KEYS = ("time_step", "time_limit", "success_reward", "collision_penalty", "discomfort_dist", "discomfort_penalty_factor")
STEP_BS, STEP_HS = (1, 127, 128, 129, 1000, 4099), (1, 2, 5, 19, 64, 127)
# (B, H, kinematics, human policy): every B with all three human policies under both kinematics, the six H rotating through
STEP_SHAPES = [(B, STEP_HS[(i + j) % 6], ("holonomic", "unicycle")[j // 3], so.HUMAN_POLICIES[j % 3])
               for i, B in enumerate(STEP_BS) for j in range(6)]


def draw_constants(rng):
    return {"time_step": float(rng.choice([0.125, 0.2, 0.25, 0.4])), "time_limit": float(rng.randint(8, 40)),
            "success_reward": float(rng.uniform(0.5, 2.0)), "collision_penalty": float(-rng.uniform(0.1, 1.0)),
            "discomfort_dist": float(rng.uniform(0.1, 0.5)), "discomfort_penalty_factor": float(rng.uniform(0.2, 1.0))}


def _place(rng, robot_xy, av, hv, dist, u0, dt):
    """Position of a human with velocity hv whose closest approach to the robot (velocity av) over the step is `dist`
    between the centres when the parameter u0 of that point lies in [0, 1] (beyond: farther, by the clamp)."""
    v = hv - av
    n = np.hypot(v[0], v[1])
    if n == 0.0:
        a = rng.uniform(0, TWO_PI)
        normal = np.array([np.cos(a), np.sin(a)])
    else:
        normal = np.array([-v[1], v[0]]) / n * (1 if rng.rand() < 0.5 else -1)
    return robot_xy + normal * dist - u0 * v * dt


def _draw_envs(rng, n, H, kinematics, c):
    """n environments: a third with one human placed to collide (first, a middle or the last human; some before it
    uncomfortably close), a third with the robot one step from its goal (some colliding as well, some at the time limit), the
    rest free; uncomfortable humans sprinkled over all of them; a fifth frozen."""
    dt, ddist = c["time_step"], c["discomfort_dist"]
    robot = np.zeros((n, 9))
    robot[:, 0:2] = rng.uniform(-4, 4, (n, 2))
    robot[:, 2:4] = rng.uniform(-1, 1, (n, 2))
    robot[:, 4] = rng.uniform(0.2, 0.5, n)
    robot[:, 7] = rng.uniform(0.5, 1.5, n)
    robot[:, 8] = rng.uniform(-3 * np.pi, 5 * np.pi, n)                  # wider than [0, 2 pi) on both sides
    if kinematics == "holonomic":
        action = rng.uniform(-1, 1, (n, 2))
    else:
        action = np.stack([rng.uniform(0, 1.2, n), rng.uniform(-1, 1, n)], 1)
    action[rng.rand(n) < 0.1] = 0.0
    if kinematics == "holonomic":
        av = action.copy()
    else:
        heading = robot[:, 8] + action[:, 1]
        av = np.stack([action[:, 0] * np.cos(heading), action[:, 0] * np.sin(heading)], 1)
    end = robot[:, 0:2] + av * dt
    kind = rng.randint(0, 3, n)                                          # 0 collide, 1 near the goal, 2 free
    ang = rng.uniform(0, TWO_PI, n)
    far = rng.uniform(2, 8, n)
    near = rng.uniform(0, 0.8, n) * robot[:, 4]
    gd = np.where(kind == 1, near, far)
    robot[:, 5:7] = end + np.stack([np.cos(ang), np.sin(ang)], 1) * gd[:, None]
    humans = np.zeros((n, H, 5))
    humans[:, :, 2:4] = rng.uniform(-1, 1, (n, H, 2))
    humans[:, :, 2:4][rng.rand(n, H) < 0.15] = 0.0
    humans[:, :, 4] = rng.uniform(0.2, 0.5, (n, H))
    a = rng.uniform(0, TWO_PI, (n, H))
    # out of reach by default: two agents close at most 2 sqrt(2) m/s * 0.4 s, and discomfort_dist is at most 0.5
    r = humans[:, :, 4] + robot[:, 4:5] + 1.7 + rng.uniform(0, 4, (n, H))
    humans[:, :, 0:2] = robot[:, None, 0:2] + np.stack([np.cos(a), np.sin(a)], -1) * r[:, :, None]
    for b in range(n):
        special = {}                                                     # human index -> gap between the boundaries
        if kind[b] == 0 or (kind[b] == 1 and rng.rand() < 0.3):
            j = int(rng.choice([0, H // 2, H - 1]))
            special[j] = -rng.uniform(0.01, 0.3)
            for i in rng.permutation(j)[:max(1, j // 2) if j else 0][:3]:
                special[int(i)] = rng.uniform(0.01, 0.95 * ddist)        # dmin is set when the loop stops
            if j + 1 < H and rng.rand() < 0.3:
                special[int(rng.randint(j + 1, H))] = -rng.uniform(0.01, 0.3)
        if rng.rand() < 0.5:
            for i in rng.randint(0, H, 2):
                special.setdefault(int(i), rng.uniform(0.01, 0.95 * ddist))
        for i, gap in special.items():
            dist = max(humans[b, i, 4] + robot[b, 4] + gap, 0.0)
            humans[b, i, 0:2] = _place(rng, robot[b, 0:2], av[b], humans[b, i, 2:4], dist, rng.uniform(-0.3, 1.3), dt)
    goals = humans[:, :, 0:2] + rng.uniform(-8, 8, (n, H, 2))
    vpref = rng.uniform(0.5, 1.5, (n, H))
    human_actions = rng.uniform(-1, 1, (n, H, 2))
    last = c["time_limit"] - 1.0                                         # the first clock value that is a timeout
    steps = max(int(last / dt) - 2, 1)
    time = rng.randint(0, steps, n) * dt
    pick = rng.rand(n)
    time = np.where(pick < 0.12, last, np.where(pick < 0.20, last - dt, np.where(pick < 0.22, last + dt, time)))
    time = np.where((kind == 1) & (rng.rand(n) < 0.2), last, time)
    done = (rng.rand(n) < 0.2).astype(np.int32)
    return {"robot": robot, "humans": humans, "goals": goals, "vpref": vpref, "action": action, "human_actions": human_actions,
            "time": time, "done": done}


def restate(case, update=True):
    return so.step_batch(case["robot"], case["humans"], case["action"], case["time"], goals=case["goals"], vpref=case["vpref"],
                         kinematics=case["kinematics"], human_policy=case["human_policy"], human_actions=case["human_actions"],
                         update=update, done=case["done"], **case["constants"])


def draw_step_batch(seed, B, H, kinematics, human_policy, max_rounds=20, min_margin=MIN_MARGIN):
    """One batch of (b).  Environments whose margin is below min_margin are drawn again (the same generator goes on) until
    none is left, so every environment of the batch takes part in every comparison; `redrawn` counts them."""
    rng = np.random.RandomState(seed)
    c = draw_constants(rng)
    case = _draw_envs(rng, B, H, kinematics, c)
    case.update(constants=c, kinematics=kinematics, human_policy=human_policy, redrawn=0)
    for _ in range(max_rounds):
        bad = np.nonzero(restate(case)["margin"] < min_margin)[0]
        if bad.size == 0:
            return case
        new = _draw_envs(rng, bad.size, H, kinematics, c)
        for k, v in new.items():
            case[k][bad] = v
        case["redrawn"] += int(bad.size)
    raise AssertionError("the re-draw did not end after %d rounds" % max_rounds)


def step_seed(B, H, kinematics, human_policy):
    return 7000 + 131 * B + 17 * H + (5 if kinematics == "unicycle" else 0) + so.HUMAN_POLICIES.index(human_policy)


# -- (c) exact edges -------------------------------------------------------------------------------------------------------
EDGE_CONSTANTS = {"time_step": 0.25, "time_limit": 30.0, "success_reward": 1.0, "collision_penalty": -0.25,
                  "discomfort_dist": 0.25, "discomfort_penalty_factor": 0.5}
FAR = (4.0, 4.0, 0.0, 0.0, 0.25)           # a human that takes no part
# name, robot action as (vx, 0) [unicycle: v = vx, r = 0, theta = 0, so vx >= 0], goal, humans (px, py, vx, vy, radius), clock,
# expected info, expected last_dmin (None: not stated here).  Robot at the origin, radius 1/4; every number a multiple of 1/8.
EDGES = [
    ("touching at rest: distance 0 is no collision, degenerate segment", 0.0, (4.0, 0.0), [(0.5, 0.0, 0.0, 0.0, 0.25), FAR], 0.0, 1, 0.0),
    ("overlapping at rest: degenerate segment, collision", 0.0, (4.0, 0.0), [(0.25, 0.0, 0.0, 0.0, 0.25), FAR], 0.0, 2, -1.0),
    ("moving together: relative velocity exactly zero", 1.0, (4.0, 0.0), [(0.0, 0.5, 1.0, 0.0, 0.25), FAR], 0.0, 1, 0.0),
    ("u exactly 1, distance 0", 1.0, (4.0, 0.0), [(0.25, 0.5, 0.0, 0.0, 0.25), FAR], 0.0, 1, 0.0),
    ("u exactly 0, distance 0", 1.0, (4.0, 0.0), [(0.0, 0.5, 0.0, 0.0, 0.25), FAR], 0.0, 1, 0.0),
    ("u = 1/2 inside, distance 0", 1.0, (4.0, 0.0), [(0.25, 0.5, -1.0, 0.0, 0.25), FAR], 0.0, 1, 0.0),
    ("u = 3 clamped to 1 (unclamped: through the centre)", 1.0, (4.0, 0.0), [(0.75, 0.0, 0.0, 0.0, 0.25), FAR], 0.0, 1, 0.0),
    ("u = -2 clamped to 0 (unclamped: through the centre)", 0.0, (4.0, 0.0), [(0.5, 0.0, 1.0, 0.0, 0.25), FAR], 0.0, 1, 0.0),
    ("goal distance exactly the radius is not reaching", 1.0, (0.5, 0.0), [FAR, FAR], 0.0, 0, None),
    ("goal distance 1/8 is reaching", 1.0, (0.375, 0.0), [FAR, FAR], 0.0, 3, None),
    ("dmin exactly discomfort_dist is nothing", 0.0, (4.0, 0.0), [(0.0, 0.75, 0.0, 0.0, 0.25), FAR], 0.0, 0, 0.25),
    ("dmin 1/8 below discomfort_dist", 0.0, (4.0, 0.0), [(0.0, 0.625, 0.0, 0.0, 0.25), FAR], 0.0, 1, 0.125),
    ("clock exactly time_limit - 1: timeout over collision and goal", 1.0, (0.25, 0.0), [(0.25, 0.0, 0.0, 0.0, 0.25), FAR], 29.0, 4, -1.0),
    ("clock one step before: collision over goal", 1.0, (0.25, 0.0), [(0.25, 0.0, 0.0, 0.0, 0.25), FAR], 28.75, 2, -1.0),
    ("goal over discomfort", 1.0, (0.25, 0.0), [(0.0, 0.625, 0.0, 0.0, 0.25), FAR], 0.0, 3, 0.125),
    ("stops at the first collision: the closer second human is not seen", 0.0, (4.0, 0.0),
     [(0.0, 0.625, 0.0, 0.0, 0.25), (0.25, 0.0, 0.0, 0.0, 0.25), (0.0, 0.5, 0.0, 0.0, 0.25)], 0.0, 2, -1.0),
    ("discomfort takes the smallest: the last human", 0.0, (4.0, 0.0),
     [(0.0, 0.625, 0.0, 0.0, 0.25), FAR, (0.0, 0.5, 0.0, 0.0, 0.25)], 0.0, 1, 0.0),
]


def edge_batch(kinematics, human_policy):
    """The edges as one batch with three humans each (FAR fills up).  `constant_velocity` and `given` humans only: their
    motion is exact in binary."""
    n = len(EDGES)
    robot, humans = np.zeros((n, 9)), np.zeros((n, 3, 5))
    action, time = np.zeros((n, 2)), np.zeros(n)
    for b, (_, vx, goal, hs, clock, _, _) in enumerate(EDGES):
        robot[b] = (0.0, 0.0, 0.0, 0.0, 0.25, goal[0], goal[1], 1.0, 0.0)
        humans[b] = (list(hs) + [FAR] * 3)[:3]
        action[b, 0], time[b] = vx, clock
    human_actions = np.zeros((n, 3, 2))
    human_actions[:, :, 0], human_actions[:, :, 1] = 1.0, -1.0
    return {"robot": robot, "humans": humans, "goals": None, "vpref": None, "action": action, "human_actions": human_actions,
            "time": time, "done": np.zeros(n, np.int32), "constants": dict(EDGE_CONSTANTS), "kinematics": kinematics,
            "human_policy": human_policy, "expect_info": np.array([e[5] for e in EDGES], np.int32),
            "expect_last_dmin": np.array([np.nan if e[6] is None else e[6] for e in EDGES])}


# -- (d) unicycle wrap -----------------------------------------------------------------------------------------------------
# (theta, r): theta + r just below 0, exactly 0, just below 2 pi, exactly 2 pi, below -2 pi, above 4 pi, and some in between
WRAPS = [(1.0, float(np.nextafter(-1.0, -2.0))), (1.0, -1.0), (float(np.nextafter(TWO_PI, 0.0)) - 1.0, 1.0), (TWO_PI - 1.0, 1.0),
         (-5.0, -3.0), (9.0, 4.0), (-7.5, -1.2), (0.3, 1.1), (5.9, 1.3), (2.0, -1.5), (-0.4, -1.0), (13.5, 1.25),
         (4 * np.pi - 1.0, 1.0), (-TWO_PI + 1.0, -1.0)]


def wrap_batch(human_policy="constant_velocity"):
    """One environment per entry of WRAPS: robot radius 0.3 driving v = 1 for 0.25 s towards a human (radius 0.3, at rest)
    0.8 away along the new heading theta + r, which it therefore hits; driving along any heading 60 degrees or more off
    that one it does not."""
    n = len(WRAPS)
    robot, humans = np.zeros((n, 9)), np.zeros((n, 2, 5))
    action = np.zeros((n, 2))
    for b, (theta, r) in enumerate(WRAPS):
        robot[b] = (0.5, -0.25, 0.0, 0.0, 0.3, 6.0, 6.0, 1.0, theta)
        action[b] = (1.0, r)
        humans[b, 0] = (4.5, 4.0, 0.3, -0.2, 0.3)
        humans[b, 1] = (0.5 + 0.8 * np.cos(theta + r), -0.25 + 0.8 * np.sin(theta + r), 0.0, 0.0, 0.3)
    return {"robot": robot, "humans": humans, "goals": None, "vpref": None, "action": action,
            "human_actions": np.zeros((n, 2, 2)), "time": np.zeros(n), "done": np.zeros(n, np.int32),
            "constants": {k: v for k, v in zip(CONSTANT_KEYS, (0.25, 30.0, 1.0, -0.25, 0.2, 0.5))}, "kinematics": "unicycle",
            "human_policy": human_policy}
