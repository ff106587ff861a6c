"""CPU oracle for the batched simulator step (TEST INFRASTRUCTURE ONLY; see oracle/rgl_oracle.py for the rules).

A sequential, python-float restatement of one environment's time step in every mode the device kernel has (holonomic and
unicycle robots; `linear`, `constant_velocity` and supplied human actions; update on and off; frozen environments; every
constant of the reward ladder), following crowd_sim/envs/crowd_sim.py:252-368, crowd_sim/envs/utils/agent.py:117-142,
crowd_sim/envs/utils/utils.py:4-26 and crowd_sim/envs/policy/linear.py:16-22, and its numpy float64 twin over a batch
(`step_batch`).  Pinned against trajectories recorded from the reference simulator itself (tests/golden/sim.npz,
tests/golden/sim_modes.npz).

The MARGIN of a step is the smallest distance between any quantity the step compared and the threshold it was compared
with: every closest distance against 0 up to and including the first collision, the goal distance against the robot's
radius and, when no collision ended the loop and some human was seen, dmin against discomfort_dist.  A step whose margin
is far above rounding has the same outcome in every correct implementation; tests use it to keep decisions away from
rounding.  The clamps of u are continuous and the clock test is the same IEEE additions on every side: neither enters."""
import numpy as np

from oracle.rgl_oracle import point_to_segment_dist

INFO_NOTHING, INFO_DISCOMFORT, INFO_COLLISION, INFO_REACH_GOAL, INFO_TIMEOUT, INFO_DONE = 0, 1, 2, 3, 4, 5
HUMAN_POLICIES = ("linear", "constant_velocity", "given")
KINEMATICS = ("holonomic", "unicycle")


def linear_action(h_full):
    """h_full = (px, py, vx, vy, radius, gx, gy, v_pref, theta) of one human."""
    theta = np.arctan2(h_full[6] - h_full[1], h_full[5] - h_full[0])
    return np.cos(theta) * h_full[7], np.sin(theta) * h_full[7]


def step(robot, humans, action, global_time, time_step=0.25, time_limit=30, success_reward=1, collision_penalty=-0.25,
         discomfort_dist=0.2, discomfort_penalty_factor=0.5, kinematics="holonomic", human_policy="linear",
         human_actions=None, update=True, done=False, full=False):
    """robot: list of 9 floats (theta in slot 8), humans: list of 9-float lists (full states; `constant_velocity` and
    `given` read only the first five), action: (vx, vy) holonomic | (v, r) unicycle.  human_actions: [(vx, vy)] per
    human for `given` (not needed with update=False).  done: the environment was finished on entry (frozen).
    Returns (robot', humans', reward, done, info, dmin); with full=True also last_dmin (what the device reports: -1 after a
    collision) and the margin (module docstring).  With update=False, and for a frozen environment, the states come back
    unchanged."""
    if kinematics not in KINEMATICS:
        raise ValueError("unknown kinematics %r" % (kinematics,))
    if human_policy not in HUMAN_POLICIES:
        raise ValueError("unknown human policy %r" % (human_policy,))
    if done:
        out = (list(robot), [list(h) for h in humans], 0, True, INFO_DONE, float("inf"))
        return out + (float("inf"), float("inf")) if full else out
    if human_policy == "linear":
        human_actions = [linear_action(h) for h in humans]
    elif human_policy == "constant_velocity":
        human_actions = [(h[2], h[3]) for h in humans]
    elif update and human_actions is None:
        raise ValueError("human_policy 'given' needs human_actions to update")
    if kinematics == "holonomic":
        avx, avy = action[0], action[1]
    else:
        avx, avy = action[0] * np.cos(action[1] + robot[8]), action[0] * np.sin(action[1] + robot[8])
    dmin, collision, margin = float("inf"), False, float("inf")
    for h in humans:
        px, py = h[0] - robot[0], h[1] - robot[1]
        vx, vy = h[2] - avx, h[3] - avy
        ex, ey = px + vx * time_step, py + vy * time_step
        d = point_to_segment_dist(px, py, ex, ey, 0, 0) - h[4] - robot[4]
        margin = min(margin, abs(d))
        if d < 0:
            collision = True
            break
        if d < dmin:
            dmin = d
    if kinematics == "holonomic":
        end = np.array((robot[0] + action[0] * time_step, robot[1] + action[1] * time_step))
    else:
        theta = robot[8] + action[1]
        end = np.array((robot[0] + np.cos(theta) * action[0] * time_step, robot[1] + np.sin(theta) * action[0] * time_step))
    goal_dist = np.linalg.norm(end - np.array((robot[5], robot[6])))
    reaching = goal_dist < robot[4]
    margin = min(margin, abs(goal_dist - robot[4]))
    if not collision and dmin < float("inf"):
        margin = min(margin, abs(dmin - discomfort_dist))
    if global_time >= time_limit - 1:
        reward, fin, info = 0, True, INFO_TIMEOUT
    elif collision:
        reward, fin, info = collision_penalty, True, INFO_COLLISION
    elif reaching:
        reward, fin, info = success_reward, True, INFO_REACH_GOAL
    elif dmin < discomfort_dist:
        reward, fin, info = (dmin - discomfort_dist) * discomfort_penalty_factor * time_step, False, INFO_DISCOMFORT
    else:
        reward, fin, info = 0, False, INFO_NOTHING
    if update:
        nr = list(robot)
        nr[0], nr[1] = end[0], end[1]
        if kinematics == "holonomic":
            nr[2], nr[3] = action[0], action[1]
        else:
            nr[8] = (robot[8] + action[1]) % (2 * np.pi)
            nr[2], nr[3] = action[0] * np.cos(nr[8]), action[0] * np.sin(nr[8])
        nh = []
        for h, a in zip(humans, human_actions):
            g = list(h)
            g[0], g[1], g[2], g[3] = h[0] + a[0] * time_step, h[1] + a[1] * time_step, a[0], a[1]
            nh.append(g)
    else:
        nr, nh = list(robot), [list(h) for h in humans]
    out = (nr, nh, reward, fin, info, dmin)
    return out + (-1.0 if collision else dmin, margin) if full else out


def step_batch(robot, humans, action, global_time, goals=None, vpref=None, time_step=0.25, time_limit=30, success_reward=1,
               collision_penalty=-0.25, discomfort_dist=0.2, discomfort_penalty_factor=0.5, kinematics="holonomic",
               human_policy="linear", human_actions=None, update=True, done=None):
    """`step` for B environments at once in numpy float64, in the device's layout: robot (B, 9), humans (B, H, 5), goals
    (B, H, 2) and vpref (B, H) for `linear`, action (B, 2), global_time (B,), human_actions (B, H, 2) for `given`, done (B,)
    on entry.  The constants are scalars or (B,) arrays.  Returns a dict: robot, humans, time (the states and clock after
    the step), reward (float64), done, info, dmin, last_dmin, margin."""
    if kinematics not in KINEMATICS:
        raise ValueError("unknown kinematics %r" % (kinematics,))
    if human_policy not in HUMAN_POLICIES:
        raise ValueError("unknown human policy %r" % (human_policy,))
    robot, humans, action = np.array(robot, np.float64), np.array(humans, np.float64), np.asarray(action, np.float64)
    B, H = humans.shape[0], humans.shape[1]
    if robot.shape != (B, 9) or humans.shape != (B, H, 5) or action.shape != (B, 2):
        raise ValueError("robot (B, 9), humans (B, H, 5), action (B, 2)")
    global_time = np.array(np.broadcast_to(np.asarray(global_time, np.float64), (B,)))
    frozen = np.zeros(B, bool) if done is None else np.asarray(done).astype(bool)
    bc = lambda x: np.broadcast_to(np.asarray(x, np.float64), (B,))          # noqa: E731
    dt, limit, success, penalty = bc(time_step), bc(time_limit), bc(success_reward), bc(collision_penalty)
    ddist, factor = bc(discomfort_dist), bc(discomfort_penalty_factor)
    if human_policy == "linear":
        if goals is None or vpref is None:
            raise ValueError("human_policy 'linear' needs goals and vpref")
        goals, vpref = np.asarray(goals, np.float64), np.asarray(vpref, np.float64)
        th = np.arctan2(goals[:, :, 1] - humans[:, :, 1], goals[:, :, 0] - humans[:, :, 0])
        hact = np.stack([np.cos(th) * vpref, np.sin(th) * vpref], -1)
    elif human_policy == "constant_velocity":
        hact = humans[:, :, 2:4].copy()
    elif human_actions is not None:
        hact = np.asarray(human_actions, np.float64)
        if hact.shape != (B, H, 2):
            raise ValueError("human_actions (B, H, 2)")
    elif update:
        raise ValueError("human_policy 'given' needs human_actions to update")
    else:
        hact = None
    a0, a1 = action[:, 0], action[:, 1]
    if kinematics == "holonomic":
        avx, avy = a0, a1
        endx, endy = robot[:, 0] + a0 * dt, robot[:, 1] + a1 * dt
    else:
        avx, avy = a0 * np.cos(a1 + robot[:, 8]), a0 * np.sin(a1 + robot[:, 8])
        theta = robot[:, 8] + a1
        endx, endy = robot[:, 0] + np.cos(theta) * a0 * dt, robot[:, 1] + np.sin(theta) * a0 * dt
    dmin, margin, collision = np.full(B, np.inf), np.full(B, np.inf), np.zeros(B, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for h in range(H):
            px, py = humans[:, h, 0] - robot[:, 0], humans[:, h, 1] - robot[:, 1]
            vx, vy = humans[:, h, 2] - avx, humans[:, h, 3] - avy
            ex, ey = px + vx * dt, py + vy * dt
            sx, sy = ex - px, ey - py
            degenerate = (sx == 0) & (sy == 0)
            u = ((0 - px) * sx + (0 - py) * sy) / (sx * sx + sy * sy)
            u = np.where(u > 1, 1.0, np.where(u < 0, 0.0, u))
            cx, cy = px + u * sx - 0, py + u * sy - 0
            cx, cy = np.where(degenerate, 0 - px, cx), np.where(degenerate, 0 - py, cy)
            d = np.sqrt(cx * cx + cy * cy) - humans[:, h, 4] - robot[:, 4]
            live = ~collision                                     # the loop of this environment has not stopped yet
            margin = np.where(live, np.minimum(margin, np.abs(d)), margin)
            collision = collision | (live & (d < 0))
            dmin = np.where(live & ~(d < 0) & (d < dmin), d, dmin)
    gx, gy = endx - robot[:, 5], endy - robot[:, 6]
    goal_dist = np.sqrt(gx * gx + gy * gy)
    reaching = goal_dist < robot[:, 4]
    margin = np.minimum(margin, np.abs(goal_dist - robot[:, 4]))
    with np.errstate(invalid="ignore"):
        margin = np.where(~collision & np.isfinite(dmin), np.minimum(margin, np.abs(dmin - ddist)), margin)
        discomfort_reward = (dmin - ddist) * factor * dt
    timeout = global_time >= limit - 1
    info = np.where(timeout, INFO_TIMEOUT, np.where(collision, INFO_COLLISION, np.where(reaching, INFO_REACH_GOAL, np.where(
        dmin < ddist, INFO_DISCOMFORT, INFO_NOTHING)))).astype(np.int32)
    reward = np.select([info == INFO_COLLISION, info == INFO_REACH_GOAL, info == INFO_DISCOMFORT],
                       [penalty, success, discomfort_reward], 0.0)
    fin = (info >= INFO_COLLISION) & (info <= INFO_TIMEOUT)
    last_dmin = np.where(collision, -1.0, dmin)
    info = np.where(frozen, INFO_DONE, info).astype(np.int32)
    reward, fin = np.where(frozen, 0.0, reward), np.where(frozen, True, fin)
    dmin, last_dmin, margin = np.where(frozen, np.inf, dmin), np.where(frozen, np.inf, last_dmin), np.where(frozen, np.inf, margin)
    nr, nh, nt = robot.copy(), humans.copy(), global_time.copy()
    if update:
        m = ~frozen
        nr[m, 0], nr[m, 1] = endx[m], endy[m]
        if kinematics == "holonomic":
            nr[m, 2], nr[m, 3] = a0[m], a1[m]
        else:
            ntheta = np.mod(robot[:, 8] + a1, 2 * np.pi)           # numpy's remainder is python's %: the divisor's sign
            nr[m, 8], nr[m, 2], nr[m, 3] = ntheta[m], (a0 * np.cos(ntheta))[m], (a0 * np.sin(ntheta))[m]
        nh[m, :, 0:2] = (humans[:, :, 0:2] + hact * dt[:, None, None])[m]
        nh[m, :, 2:4] = hact[m]
        nt[m] = (global_time + dt)[m]
    return {"robot": nr, "humans": nh, "time": nt, "reward": reward, "done": fin, "info": info, "dmin": dmin,
            "last_dmin": last_dmin, "margin": margin}


def float32_ulp(x):
    """Spacing of float32 at |x| (the distance to the next float32 away from zero), as float64."""
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)
