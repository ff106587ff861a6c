"""Loop-per-agent numpy restatement of the device ORCA (relationalgraphlearning_amd/csrc/rgl_orca.hip), test infrastructure.

RVO2 2.0's doStep for agents without obstacles, written from the algorithm's statement: every agent quantity is a float32
rounded once from float64, and every operation below is an individually rounded np.float32 operation (numpy never fuses a
multiply and an add, its float32 division and square root are correctly rounded), so the device kernel -- compiled without
contraction and with correctly rounded division and square root -- must agree bit for bit.  Neighbours are found by walking
the agents in index order (RVO2 walks a kd-tree: the two differ only on exact distance ties at the max_neighbors cut-off).

`PyRVOSimulator` wraps the same arithmetic in Python-RVO2's method names, so that the reference's own ORCA / CentralizedORCA
(which `import rvo2`) run on it when `sys.modules["rvo2"]` is this module (tests/golden/make_golden_orca.py).
"""
import math

import numpy as np

f32 = np.float32
EPS = f32(1e-5)
ZERO, HALF, ONE = f32(0.0), f32(0.5), f32(1.0)


def v2(x, y):
    return (f32(x), f32(y))


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1])


def add(a, b):
    return (a[0] + b[0], a[1] + b[1])


def scale(s, a):
    return (a[0] * s, a[1] * s)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1]


def det(a, b):
    return a[0] * b[1] - a[1] * b[0]


def abs_sq(a):
    return a[0] * a[0] + a[1] * a[1]


def div(a, s):
    inv = ONE / s
    return (a[0] * inv, a[1] * inv)


def normalize(a):
    return div(a, np.sqrt(abs_sq(a)))


def linear_program1(lines, k, radius, opt, direction_opt):
    """RVO2 linearProgram1: the new result, or None when line k's segment inside the disk is empty."""
    p, d = lines[k]
    dp = dot(p, d)
    disc = dp * dp + radius * radius - abs_sq(p)
    if disc < ZERO:
        return None
    sd = np.sqrt(disc)
    t_left, t_right = -dp - sd, -dp + sd
    for i in range(k):
        pi, di = lines[i]
        den = det(d, di)
        num = det(di, sub(p, pi))
        if abs(den) <= EPS:
            if num < ZERO:
                return None
            continue
        t = num / den
        if den >= ZERO:
            t_right = t if t < t_right else t_right
        else:
            t_left = t if t_left < t else t_left
        if t_left > t_right:
            return None
    if direction_opt:
        return add(p, scale(t_right if dot(opt, d) > ZERO else t_left, d))
    t = dot(d, sub(opt, p))
    return add(p, scale(t_left if t < t_left else (t_right if t > t_right else t), d))


def linear_program2(lines, radius, opt, direction_opt):
    """RVO2 linearProgram2: (index of the first line that could not be satisfied or len(lines), result)."""
    if direction_opt:
        result = scale(radius, opt)
    elif abs_sq(opt) > radius * radius:
        result = scale(radius, normalize(opt))
    else:
        result = opt
    for i in range(len(lines)):
        if det(lines[i][1], sub(lines[i][0], result)) > ZERO:
            r = linear_program1(lines, i, radius, opt, direction_opt)
            if r is None:
                return i, result
            result = r
    return len(lines), result


def linear_program3(lines, begin, radius, result):
    """RVO2 linearProgram3 (no obstacle lines): minimise the largest violation from line `begin` on."""
    distance = ZERO
    for i in range(begin, len(lines)):
        pi, di = lines[i]
        if det(di, sub(pi, result)) > distance:
            proj = []
            for j in range(i):
                pj, dj = lines[j]
                den = det(di, dj)
                if abs(den) <= EPS:
                    if dot(di, dj) > ZERO:
                        continue
                    point = scale(HALF, add(pi, pj))
                else:
                    point = add(pi, scale(det(dj, sub(pi, pj)) / den, di))
                proj.append((point, normalize(sub(dj, di))))
            n, r = linear_program2(proj, radius, (-di[1], di[0]), True)
            if n >= len(proj):
                result = r
            distance = det(di, sub(pi, result))
    return result


def neighbours(pos, self_index, max_neighbors, neighbor_dist):
    """Indices of the agents RVO2 keeps for agent `self_index`: the max_neighbors nearest with distSq < neighbor_dist^2,
    ascending distSq (the kd-tree query's insertion, with the agents visited in index order).  pos: list of float32 pairs."""
    if max_neighbors <= 0:
        return []
    me = pos[self_index]
    range_sq = f32(neighbor_dist) * f32(neighbor_dist)
    out = []                                                   # (distSq, index)
    for a in range(len(pos)):
        if a == self_index:
            continue
        dsq = abs_sq(sub(me, pos[a]))
        if not dsq < range_sq:
            continue
        if len(out) < max_neighbors:
            out.append(None)
        k = len(out) - 1
        while k != 0 and dsq < out[k - 1][0]:
            out[k] = out[k - 1]
            k -= 1
        out[k] = (dsq, a)
        if len(out) == max_neighbors:
            range_sq = out[-1][0]
    return [a for _, a in out]


def orca_lines(pos, vel, radius, self_index, nbrs, time_horizon, time_step, branches=None):
    """One ORCA half-plane (point, direction) per neighbour, in list order (RVO2 computeNewVelocity).  `branches`, if a list,
    receives the case of each line: 'cutoff', 'left', 'right' or 'collision'."""
    me_p, me_v, me_r = pos[self_index], vel[self_index], radius[self_index]
    inv_th = ONE / f32(time_horizon)
    inv_dt = ONE / f32(time_step)
    lines = []
    for a in nbrs:
        rel_pos = sub(pos[a], me_p)
        rel_vel = sub(me_v, vel[a])
        dist_sq = abs_sq(rel_pos)
        R = me_r + radius[a]
        R_sq = R * R
        if dist_sq > R_sq:
            w = sub(rel_vel, scale(inv_th, rel_pos))
            w_len_sq = abs_sq(w)
            dp1 = dot(w, rel_pos)
            if dp1 < ZERO and dp1 * dp1 > R_sq * w_len_sq:
                w_len = np.sqrt(w_len_sq)
                unit_w = div(w, w_len)
                direction = (unit_w[1], -unit_w[0])
                u = scale(R * inv_th - w_len, unit_w)
                case = 'cutoff'
            else:
                leg = np.sqrt(dist_sq - R_sq)
                case = 'left' if det(rel_pos, w) > ZERO else 'right'
                if det(rel_pos, w) > ZERO:
                    direction = div((rel_pos[0] * leg - rel_pos[1] * R, rel_pos[0] * R + rel_pos[1] * leg), dist_sq)
                else:
                    direction = div((-(rel_pos[0] * leg + rel_pos[1] * R), -(-rel_pos[0] * R + rel_pos[1] * leg)), dist_sq)
                u = sub(scale(dot(rel_vel, direction), direction), rel_vel)
        else:
            w = sub(rel_vel, scale(inv_dt, rel_pos))
            w_len = np.sqrt(abs_sq(w))
            unit_w = div(w, w_len)
            direction = (unit_w[1], -unit_w[0])
            u = scale(R * inv_dt - w_len, unit_w)
            case = 'collision'
        if branches is not None:
            branches.append(case)
        lines.append((add(me_v, scale(HALF, u)), direction))
    return lines


def new_velocity(pos, vel, radius, self_index, pref, max_speed, time_step, neighbor_dist=10.0, max_neighbors=10,
                 time_horizon=5.0, info=None):
    """Agent `self_index`'s new velocity (float32 pair).  pos / vel / radius: float32 per agent (already rounded).
    `info`, if a dict, receives the lines and whether LP3 ran."""
    nbrs = neighbours(pos, self_index, max_neighbors, neighbor_dist)
    branches = []
    lines = orca_lines(pos, vel, radius, self_index, nbrs, time_horizon, time_step, branches)
    max_speed = f32(max_speed)
    fail, result = linear_program2(lines, max_speed, pref, False)
    if fail < len(lines):
        result = linear_program3(lines, fail, max_speed, result)
    if info is not None:
        info.update(lines=lines, lp3=fail < len(lines), neighbours=nbrs, branches=branches,
                    clipped=abs_sq(pref) > max_speed * max_speed)
    return result


# -- the entry points' agent assembly (float64 in, float32 once) ------------------------------------------------------------
def orca_radius(r, safety_space):
    return f32(float(r) + 0.01 + float(safety_space))


def orca_pref(px, py, gx, gy):
    dx, dy = float(gx) - float(px), float(gy) - float(py)
    speed = math.sqrt(dx * dx + dy * dy)
    if speed > 1.0:
        dx, dy = dx / speed, dy / speed
    return (f32(dx), f32(dy))


def humans_velocities(robot, humans, goals, vpref, robot_visible, time_step=0.25, neighbor_dist=10.0, max_neighbors=10,
                      time_horizon=5.0, safety_space=0.0, centralized=True, infos=None):
    """crowd_orca_humans_f64 for one environment: robot (9,), humans (H,5), goals (H,2), vpref (H,) float64 -> (H,2) float64."""
    rows = [np.asarray(h, np.float64) for h in humans] + ([np.asarray(robot, np.float64)] if robot_visible else [])
    pos = [v2(r[0], r[1]) for r in rows]
    vel = [v2(r[2], r[3]) for r in rows]
    rad = [orca_radius(r[4], safety_space) for r in rows]
    out = np.zeros((len(humans), 2))
    for h in range(len(humans)):
        pref = orca_pref(humans[h][0], humans[h][1], goals[h][0], goals[h][1])
        ms = f32(1.0) if centralized else f32(vpref[h])
        info = {} if infos is not None else None
        v = new_velocity(pos, vel, rad, h, pref, ms, time_step, neighbor_dist, max_neighbors, time_horizon, info)
        if infos is not None:
            infos.append(info)
        out[h] = (float(v[0]), float(v[1]))
    return out


def robot_velocity(robot, humans, time_step=0.25, neighbor_dist=10.0, max_neighbors=10, time_horizon=5.0, safety_space=0.0):
    """crowd_orca_robot_f64 for one environment -> (2,) float64."""
    rows = [np.asarray(robot, np.float64)] + [np.asarray(h, np.float64) for h in humans]
    pos = [v2(r[0], r[1]) for r in rows]
    vel = [v2(r[2], r[3]) for r in rows]
    rad = [orca_radius(r[4], safety_space) for r in rows]
    pref = orca_pref(robot[0], robot[1], robot[5], robot[6])
    v = new_velocity(pos, vel, rad, 0, pref, f32(robot[7]), time_step, neighbor_dist, max_neighbors, time_horizon)
    return np.array([float(v[0]), float(v[1])])


class PyRVOSimulator(object):
    """Python-RVO2's simulator interface over the restatement (agents only; the obstacle arguments are accepted and unused)."""

    def __init__(self, time_step, neighbor_dist, max_neighbors, time_horizon, time_horizon_obst, radius, max_speed,
                 velocity=(0, 0)):
        self.time_step = f32(time_step)
        self.defaults = (neighbor_dist, max_neighbors, time_horizon, time_horizon_obst, radius, max_speed, velocity)
        self.agents = []

    def addAgent(self, pos, neighbor_dist=None, max_neighbors=None, time_horizon=None, time_horizon_obst=None, radius=None,
                 max_speed=None, velocity=None):
        d = self.defaults
        pick = lambda v, i: d[i] if v is None else v        # noqa: E731
        self.agents.append(dict(pos=v2(*pos), vel=v2(*pick(velocity, 6)), pref=v2(0.0, 0.0),
                                neighbor_dist=f32(pick(neighbor_dist, 0)), max_neighbors=int(pick(max_neighbors, 1)),
                                time_horizon=f32(pick(time_horizon, 2)), radius=f32(pick(radius, 4)),
                                max_speed=f32(pick(max_speed, 5))))
        return len(self.agents) - 1

    def getNumAgents(self):
        return len(self.agents)

    def setAgentPosition(self, i, pos):
        self.agents[i]["pos"] = v2(*pos)

    def setAgentVelocity(self, i, vel):
        self.agents[i]["vel"] = v2(*vel)

    def setAgentPrefVelocity(self, i, vel):
        self.agents[i]["pref"] = v2(*vel)

    def getAgentPosition(self, i):
        return tuple(float(x) for x in self.agents[i]["pos"])

    def getAgentVelocity(self, i):
        return tuple(float(x) for x in self.agents[i]["vel"])

    def doStep(self):
        pos = [a["pos"] for a in self.agents]
        vel = [a["vel"] for a in self.agents]
        rad = [a["radius"] for a in self.agents]
        new = [new_velocity(pos, vel, rad, i, a["pref"], a["max_speed"], self.time_step, a["neighbor_dist"],
                            a["max_neighbors"], a["time_horizon"]) for i, a in enumerate(self.agents)]
        for a, v in zip(self.agents, new):
            a["vel"] = v
            a["pos"] = add(a["pos"], scale(self.time_step, v))
