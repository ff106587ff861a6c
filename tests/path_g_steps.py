"""Host replay of path G's steps (csrc/rgl_rotate.h: rotate_row; csrc/rgl_onestep.h: gcn_prepare_kernel, onestep_select_kernel) in numpy: every float32
operation an individually rounded float32 operation, every float64 operation a plain numpy float64 operation.

This module is the DEFINITION of those steps for the tests.  It is written from the reference's arithmetic
(crowd_nav/policy/cadrl.py:113-138,241-276, multi_human_rl.py:36-96) as oracle/rgl_oracle.py states it, and pinned to the oracle and
to fixture path_g.npz by tests/test_path_g_steps_cpu.py; nothing in it comes from the kernels.

  rotate   the pairwise relation features of (R,14) joint rows.  It never calls a libm: the caller hands in `trig = (rot, c, sn)`,
           float32 -- torch's on the CPU, the device's own (read back through probe rows) on the GPU -- and everything else is exact.
  prepare  propagate + constant-velocity humans in float64, the rounding of the 14-column rows to float32, `rotate`, and
           compute_reward in float64, for every (root, action) pair.  Holonomic: no libm call at all.  Unicycle: the float64
           cos / sin of theta + rotation are numpy's (the one libm call of this module; the tests bound its effect).
  decide   v = float64(reward) + disc * float64(value), the first maximum under strict `>`, -1 when nothing beats -inf.
  segment_reward   path M's estimate_reward for float64 joint-state roots (holonomic), for the contact family of the reward step.

`fused=True` evaluates every `x * y + z` the way a compiler that contracts them does (one rounding, `FUSED_PRODUCT` says which
product of a two-product sum stays exact).  It exists to COUNT, on the CPU, how many cases of a family can tell a contracted build
from the reference's arithmetic; it never produces an expectation.
"""
import math
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64
_math_fma = getattr(math, "fma", None)
FUSED_PRODUCT = 0      # a * b + c * d contracts to fma(a, b, rn(c * d)): the first product is the exact one


def bits(x):
    """Bit patterns with the two zeros NOT identified (callers that accept either zero compare values there)."""
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


# ---------------------------------------------------------------------------------------------------------------------------
# arithmetic: unfused = numpy; fused = exact product-sum, one rounding (scalar, slow: counting only)
# ---------------------------------------------------------------------------------------------------------------------------
def _round_f32(q):
    """Fraction -> nearest float32, ties to even (no double rounding through float64)."""
    f = F32(float(q))
    if not np.isfinite(f):
        return f
    best, err = f, abs(Fraction(float(f)) - q)
    for g in (np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))):
        if not np.isfinite(g):
            continue
        e = abs(Fraction(float(g)) - q)
        if e < err or (e == err and (int(bits(g)) & 1) == 0 and (int(bits(best)) & 1) == 1):
            best, err = g, e
    return best


def _fma_scalar(a, b, c, dtype):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return dtype(F64(a) * F64(b) + F64(c))
    if dtype is F64 and _math_fma is not None:
        return F64(_math_fma(float(a), float(b), float(c)))
    q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if q == 0:                                              # the sign of an exact zero: that of the rounded operations
        return dtype(dtype(a) * dtype(b) + dtype(c))
    return F64(float(q)) if dtype is F64 else _round_f32(q)


def fma(a, b, c, dtype):
    """a * b + c with ONE rounding, elementwise (broadcasting)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype), np.asarray(b, dtype), np.asarray(c, dtype))
    out = np.empty(a.shape, dtype)
    flat = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.reshape(-1), b.reshape(-1), c.reshape(-1))):
        flat[i] = _fma_scalar(x, y, z, dtype)
    return out


class _Arith:
    """The product-sums of the steps, in one number format.  Unfused: each product and the sum rounded on their own."""

    def __init__(self, dtype, fused):
        self.t, self.fused = dtype, fused

    def mad(self, a, b, c):
        """a * b + c"""
        t = self.t
        with np.errstate(all="ignore"):
            if self.fused:
                return fma(a, b, c, t)
            return (np.asarray(a, t) * np.asarray(b, t)).astype(t) + np.asarray(c, t)

    def dot2(self, a, b, c, d, sign=1):
        """a * b + sign * c * d"""
        t = self.t
        with np.errstate(all="ignore"):
            ab = (np.asarray(a, t) * np.asarray(b, t)).astype(t)
            cd = (np.asarray(c, t) * np.asarray(d, t)).astype(t)
            if not self.fused:
                return (ab + cd if sign > 0 else ab - cd).astype(t)
            if FUSED_PRODUCT == 0:
                return fma(a, b, cd if sign > 0 else -cd, t)
            return fma(np.asarray(c, t) if sign > 0 else -np.asarray(c, t), d, ab, t)


# ---------------------------------------------------------------------------------------------------------------------------
# rotate (cadrl.py:241-276)
# ---------------------------------------------------------------------------------------------------------------------------
def goal_offsets(joint14):
    """(dx, dy) float32: what the caller's atan2 takes (rot = atan2f(dy, dx), c = cosf(rot), sn = sinf(rot))."""
    s = np.asarray(joint14, F32)
    return (s[..., 5] - s[..., 0]).astype(F32), (s[..., 6] - s[..., 1]).astype(F32)


def rotate(joint14, kinematics, trig, fused=False):
    """(..., 14) float32 [robot 9 | human 5] -> (..., 13) float32:
    [dg, v_pref, theta, radius, vx, vy, px1, py1, vx1, vy1, radius1, da, radius_sum]; trig = (rot, c, sn) float32 arrays."""
    assert kinematics in ("holonomic", "unicycle")
    s = np.asarray(joint14, F32)
    assert s.dtype == F32 and s.shape[-1] == 14
    rot, c, sn = (np.broadcast_to(np.asarray(x, F32), s.shape[:-1]) for x in trig)
    ar = _Arith(F32, fused)
    col = lambda k: s[..., k]
    with np.errstate(all="ignore"):
        dx, dy = goal_offsets(s)
        o = np.empty(s.shape[:-1] + (13,), F32)
        o[..., 0] = np.sqrt(ar.dot2(dx, dx, dy, dy))
        o[..., 1] = col(7)
        o[..., 2] = (col(8) - rot) if kinematics == "unicycle" else F32(0)
        o[..., 3] = col(4)
        o[..., 4] = ar.dot2(col(2), c, col(3), sn)
        o[..., 5] = ar.dot2(col(3), c, col(2), sn, -1)
        rx, ry = (col(9) - col(0)).astype(F32), (col(10) - col(1)).astype(F32)
        o[..., 6] = ar.dot2(rx, c, ry, sn)
        o[..., 7] = ar.dot2(ry, c, rx, sn, -1)
        o[..., 8] = ar.dot2(col(11), c, col(12), sn)
        o[..., 9] = ar.dot2(col(12), c, col(11), sn, -1)
        o[..., 10] = col(13)
        ax, ay = (col(0) - col(9)).astype(F32), (col(1) - col(10)).astype(F32)
        o[..., 11] = np.sqrt(ar.dot2(ax, ax, ay, ay))
        o[..., 12] = col(4) + col(13)
    return o


TRIG_FREE = (0, 1, 3, 10, 11, 12)            # columns of the 13 that no trig value enters (2: theta - rot under unicycle, else 0)
ROTATED = (4, 5, 6, 7, 8, 9)


# ---------------------------------------------------------------------------------------------------------------------------
# prepare (cadrl.py:113-138, multi_human_rl.py:46-51,73-96)
# ---------------------------------------------------------------------------------------------------------------------------
def propagate(robot, humans, actions, kinematics, dt, roots64=None, fused=False):
    """-> (nr (B,A,9) float64 propagated robots, nh (B,H,5) float64 constant-velocity humans).  `roots64`: the float64
    (robot, humans) the float32 arrays were rounded from; the float64 arithmetic then starts from those."""
    assert kinematics in ("holonomic", "unicycle")
    r = np.asarray(roots64[0] if roots64 is not None else robot, F64)
    h = np.asarray(roots64[1] if roots64 is not None else humans, F64)
    act = np.asarray(actions, F64).reshape(-1, 2)
    B, A = r.shape[0], act.shape[0]
    ar = _Arith(F64, fused)
    dt = F64(dt)
    nr = np.repeat(r[:, None, :], A, axis=1)
    a0, a1 = act[None, :, 0], act[None, :, 1]
    if kinematics == "holonomic":
        nr[:, :, 0] = ar.mad(a0, dt, r[:, None, 0])
        nr[:, :, 1] = ar.mad(a1, dt, r[:, None, 1])
        nr[:, :, 2] = np.broadcast_to(a0, (B, A))
        nr[:, :, 3] = np.broadcast_to(a1, (B, A))
    else:
        th = r[:, None, 8] + a1
        nr[:, :, 2] = a0 * np.cos(th)
        nr[:, :, 3] = a0 * np.sin(th)
        nr[:, :, 0] = ar.mad(nr[:, :, 2], dt, r[:, None, 0])
        nr[:, :, 1] = ar.mad(nr[:, :, 3], dt, r[:, None, 1])
        nr[:, :, 8] = th
    nh = h.copy()
    nh[:, :, 0] = ar.mad(h[:, :, 2], dt, h[:, :, 0])
    nh[:, :, 1] = ar.mad(h[:, :, 3], dt, h[:, :, 1])
    return nr, nh


def end_point_distances(nr, nh, fused=False):
    """-> (B,A,H) float64 distances between the propagated robots and humans"""
    ar = _Arith(F64, fused)
    with np.errstate(all="ignore"):
        ddx = nr[:, :, None, 0] - nh[:, None, :, 0]
        ddy = nr[:, :, None, 1] - nh[:, None, :, 1]
        return np.sqrt(ar.dot2(ddx, ddx, ddy, ddy))


def clearances(nr, nh, fused=False):
    """-> (d (B,A,H) end-point clearances, goal distance (B,A)), float64"""
    ar = _Arith(F64, fused)
    with np.errstate(all="ignore"):
        d = end_point_distances(nr, nh, fused) - nr[:, :, None, 4] - nh[:, None, :, 4]
        gx, gy = nr[:, :, 0] - nr[:, :, 5], nr[:, :, 1] - nr[:, :, 6]
        gd = np.sqrt(ar.dot2(gx, gx, gy, gy))
    return d, gd


def reward_of(d, gd, radius, dt):
    """compute_reward's branches on the clearances d (..., H), the goal distance gd and the robot radius -> float64 rewards."""
    with np.errstate(all="ignore"):
        collision = (d < 0.0).any(axis=-1)
        dmin = np.where(np.isnan(d), np.inf, d).min(axis=-1)          # `d < dmin` never takes a NaN
        reaching = gd < radius
        return np.where(collision, -0.25, np.where(reaching, 1.0, np.where(dmin < 0.2, (dmin - 0.2) * 0.5 * F64(dt), 0.0)))


def margins(d, gd, radius):
    """Distance of every decision of compute_reward from its threshold: (min |d|, |dmin - 0.2|, |goal distance - radius|)."""
    dmin = d.min(axis=-1)
    return np.abs(d).min(axis=-1), np.abs(dmin - 0.2), np.abs(gd - radius)


def prepare(robot, humans, actions, kinematics, dt, roots64, trig, fused=False):
    """robot (B,9), humans (B,H,5) float32, actions (A,2) float64 -> (joint14 (B,A,H,14), self6 (B*A,6), hum7 (B*A,H,7),
    reward (B*A,)), float32.  `trig`: (rot, c, sn) float32 arrays of shape (B,A) (one rotation per propagated robot), or a
    function of all joint rows' (dy, dx), (B,A,H), returning them (a vectorised libm need not give equal rows equal values)."""
    robot, humans = np.asarray(robot, F32), np.asarray(humans, F32)
    assert robot.dtype == F32 and humans.dtype == F32
    nr, nh = propagate(robot, humans, actions, kinematics, dt, roots64, fused)
    B, A, H = nr.shape[0], nr.shape[1], nh.shape[1]
    joint = np.empty((B, A, H, 14), F32)
    joint[:, :, :, :9] = nr.astype(F32)[:, :, None, :]
    joint[:, :, :, 9:] = nh.astype(F32)[:, None, :, :]              # columns 2..4 of nh are the roots' own, rounded here
    if callable(trig):                                              # called with every joint row's offsets, (B,A,H), in row order
        dx, dy = goal_offsets(joint)
        rot, c, sn = (np.asarray(x, F32).reshape(B, A, H) for x in trig(dy, dx))
    else:
        rot, c, sn = (np.broadcast_to(np.asarray(x, F32), (B, A))[:, :, None] for x in trig)
    o = rotate(joint, kinematics, (rot, c, sn), fused)
    d, gd = clearances(nr, nh, fused)
    rew = reward_of(d, gd, nr[:, :, 4], dt)
    return joint, o[:, :, 0, :6].reshape(B * A, 6).copy(), o[:, :, :, 6:].reshape(B * A, H, 7).copy(), rew.astype(F32).reshape(B * A)


# ---------------------------------------------------------------------------------------------------------------------------
# decide (multi_human_rl.py:38-64)
# ---------------------------------------------------------------------------------------------------------------------------
def discount(gamma, dt, v_pref):
    """pow(gamma, dt * v_pref) in float64, v_pref widened from the float32 robot row: (B,)"""
    e = F64(dt) * np.asarray(v_pref, F32).astype(F64)
    return np.array([math.pow(float(gamma), float(x)) for x in np.atleast_1d(e)], F64)


def first_strict_maximum(v):
    """(B,A) -> (B,) int32: the first column that is strictly greater than everything before it and than -inf; -1 when none is."""
    v = np.asarray(v)
    best = np.full(v.shape[0], -np.inf, v.dtype)
    ba = np.full(v.shape[0], -1, np.int32)
    with np.errstate(invalid="ignore"):
        for a in range(v.shape[1]):
            m = v[:, a] > best
            best = np.where(m, v[:, a], best)
            ba = np.where(m, a, ba).astype(np.int32)
    return ba, best


def decide(reward, value, gamma, dt, v_pref, disc=None):
    """reward, value (B,A) float32 -> (action_values (B,A) float32, best_action (B,) int32, best_value (B,) float32).
    The device keeps the rewards of `prepare` as float32 numbers, so that is what this step reads.  (The reference adds its float64
    reward: handed float64 rewards this function does the same, which is how the CPU tests pin it to the oracle; the two differ by
    one rounding of the reward, at most one float32 unit of the action value, wherever the reward is not a float32 number.)
    `disc` (B,): the discount to use instead of the host's pow (tests of a general exponent try its float64 neighbours)."""
    reward = np.asarray(reward)
    assert reward.dtype in (F32, F64)
    value = np.asarray(value, F32)
    disc = discount(gamma, dt, v_pref) if disc is None else np.asarray(disc, F64)
    with np.errstate(all="ignore"):
        v = reward.astype(F64) + (disc[:, None] * value.astype(F64))
        ba, best = first_strict_maximum(v)
        return v.astype(F32), ba, np.where(ba >= 0, best, 0.0).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# path M's reward step for float64 joint-state roots, holonomic (model_predictive_rl.py:304-357, utils.py:4-26)
# ---------------------------------------------------------------------------------------------------------------------------
def segment_clearances(robot64, humans64, actions, dt, fused=False, distances=False):
    """-> (d (P,A,H): distance of the origin from the relative segment minus the radii (`distances`: the distance alone),
    goal distance (P,A)), float64"""
    r, h = np.asarray(robot64, F64), np.asarray(humans64, F64)
    act = np.asarray(actions, F64).reshape(-1, 2)
    ar = _Arith(F64, fused)
    dt = F64(dt)
    with np.errstate(all="ignore"):
        px = np.broadcast_to((h[:, :, 0] - r[:, None, 0])[:, None, :], (r.shape[0], act.shape[0], h.shape[1]))
        py = np.broadcast_to((h[:, :, 1] - r[:, None, 1])[:, None, :], px.shape)
        vx = h[:, None, :, 2] - act[None, :, None, 0]
        vy = h[:, None, :, 3] - act[None, :, None, 1]
        ex, ey = ar.mad(vx, dt, px), ar.mad(vy, dt, py)
        sx, sy = ex - px, ey - py
        degenerate = (sx == 0) & (sy == 0)
        den = np.where(degenerate, 1.0, ar.dot2(sx, sx, sy, sy))
        u = np.where(degenerate, 0.0, ar.dot2(0.0 - px, sx, 0.0 - py, sy) / den)
        u = np.where(u > 1.0, 1.0, np.where(u < 0.0, 0.0, u))
        cx, cy = ar.mad(u, sx, px), ar.mad(u, sy, py)
        d = np.sqrt(ar.dot2(cx, cx, cy, cy))
        if not distances:
            d = d - h[:, None, :, 4] - r[:, None, None, 4]
        nx = ar.mad(act[None, :, 0], dt, r[:, None, 0])
        ny = ar.mad(act[None, :, 1], dt, r[:, None, 1])
        gx, gy = nx - r[:, None, 5], ny - r[:, None, 6]
        gd = np.sqrt(ar.dot2(gx, gx, gy, gy))
    return d, gd


def segment_reward(robot64, humans64, actions, dt, fused=False):
    """estimate_reward for every (parent, action) pair: (P,A) float64"""
    d, gd = segment_clearances(robot64, humans64, actions, dt, fused)
    return reward_of(d, gd, np.asarray(robot64, F64)[:, None, 4], dt)


# ---------------------------------------------------------------------------------------------------------------------------
# the families of the reward thresholds (committed seeds and recipes)
# ---------------------------------------------------------------------------------------------------------------------------
CONTACT_SEED, CONTACT_PAIRS = 20261, 4096


def _contact_scenes(P, H, seed):
    rng = np.random.RandomState(seed)
    robot = np.zeros((P, 9))
    robot[:, 0:2] = rng.uniform(-3, 3, (P, 2))
    robot[:, 2:4] = rng.uniform(-0.5, 0.5, (P, 2))
    robot[:, 4] = rng.uniform(0.2, 0.4, P)
    robot[:, 5:7] = robot[:, 0:2] + rng.uniform(4, 6, (P, 2))                 # goals out of reach
    robot[:, 7] = 1.0
    humans = np.zeros((P, H, 5))
    # (no libm call in the recipe: the counts the CPU tests assert must not depend on the host's cos / sin)
    humans[:, 0, 0:2] = robot[:, 0:2] + rng.uniform(0.6, 1.5, (P, 2)) * rng.choice([-1.0, 1.0], (P, 2))
    humans[:, 0, 2:4] = rng.uniform(-1, 1, (P, 2))
    humans[:, 1:, 0:2] = robot[:, None, 0:2] + 50.0 + np.arange(1, H)[None, :, None]   # the others far away
    humans[:, 1:, 4] = 0.3
    return robot, humans


def contact_family(table, P=CONTACT_PAIRS, H=1, dt=0.25, seed=CONTACT_SEED, segment=False):
    """Exact-contact pairs: float64 scenes (not float32 numbers) in which, for parent p under action p % A of `table` (A,2),
    the distance between robot and human 0, evaluated in float64 with the reference's individually rounded operations, minus the
    radii is exactly 0 -- not a collision.  Path G (end-point distance; clearance = dist - robot radius - human radius): the
    human's radius is set to `dist - robot radius`.  `segment`: path M (distance of the origin from the relative segment;
    clearance = dist - human radius - robot radius): the robot's radius is set to `dist - human radius`.
    -> (robot64 (P,9), humans64 (P,H,5), table (A,2), contact action (P,))."""
    table = np.asarray(table, F64).reshape(-1, 2)
    robot, humans = _contact_scenes(P, H, seed + (7 if segment else 0))
    mine = np.arange(P) % table.shape[0]
    if segment:
        humans[:, 0, 4] = 0.3
        dist, _ = segment_clearances(robot, humans, table, dt, distances=True)
        robot[:, 4] = dist[np.arange(P), mine, 0] - humans[:, 0, 4]
    else:
        nr, nh = propagate(None, None, table, "holonomic", dt, (robot, humans))
        dist = end_point_distances(nr, nh)
        humans[:, 0, 4] = dist[np.arange(P), mine, 0] - robot[:, 4]
    return robot, humans, table, mine


def goal_boundary_family():
    """Dyadic float64 scenes whose goal distance after the step of action k is exactly the robot radius (not reaching: strict
    `<`), each next to the same scene with the radius one float64 ulp larger (reaching).  One human, far away.  Table: the 4 axis
    steps of 1 m/s, dt = 0.25.  -> (robot64 (P,9), humans64 (P,1,5), table (4,2), k (P,), reaching (P,) bool)."""
    table = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    rows, ks, reach = [], [], []
    for k, (ux, uy) in enumerate(table):
        for radius in (0.25, 0.5, 0.3125):
            for ox, oy in ((0.0, 0.0), (3.0, -2.0), (-1024.0, 512.5)):
                ex, ey = ox + 0.25 * ux, oy + 0.25 * uy                      # the robot after the step of action k
                if radius == 0.3125:                                         # 3-4-5: (0.1875, 0.25) in the frame of u
                    gx, gy = ex + 0.1875 * ux - 0.25 * uy, ey + 0.1875 * uy + 0.25 * ux
                else:
                    gx, gy = ex + radius * ux, ey + radius * uy
                for rad, inside in ((radius, False), (np.nextafter(radius, 1.0), True)):
                    rows.append([ox, oy, 0.0, 0.0, rad, gx, gy, 1.0, 0.0])
                    ks.append(k)
                    reach.append(inside)
    robot = np.array(rows)
    humans = np.zeros((len(rows), 1, 5))
    humans[:, 0, 0:2] = robot[:, 0:2] + 40.0
    humans[:, 0, 4] = 0.3
    return robot, humans, table, np.array(ks), np.array(reach)


def collision_beats_goal_family():
    """The step of action 0 ends inside the goal AND inside human 0 (reward -0.25, not 1); of action 1 inside the goal only (1);
    of action 2 in neither, 0.125 m from human 1 (discomfort: (0.125 - 0.2) * 0.5 * dt); action 3 touches human 1 exactly
    (clearance 0: no collision, -0.2 * 0.5 * dt).  Dyadic float64 numbers throughout, dt = 0.25."""
    table = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    robot = np.array([[2.0, -1.0, 0.0, 0.0, 0.25, 2.125, -0.875, 1.0, 0.0]])          # goal 0.125 * sqrt(2) from both end points
    humans = np.array([[[2.5, -1.0, 0.0, 0.0, 0.125],                                   # 0.25 from end point 0: clearance -0.125
                        [1.25, -1.0, 0.0, 0.0, 0.125],                                  # 0.5 from end point 2: clearance 0.125
                        [2.0, -1.75, 0.0, 0.0, 0.25]]])                                 # 0.5 from end point 3: clearance 0
    return robot, humans, table, np.array([[-0.25, 1.0, (0.125 - 0.2) * 0.5 * 0.25, (0.0 - 0.2) * 0.5 * 0.25]])


def rotate_rows(R, seed=5):
    """(R,14) float32 joint rows, by row index modulo 8: 0, 6, 7 dense random scenes; 1 robot at its goal (dx = dy = 0); 2 / 3 goals
    on the robot's own x / y line (either side); 4 coordinates of order 1e4; 5 denormal goal offsets."""
    rng = np.random.RandomState(seed)
    s = np.zeros((R, 14), F32)
    s[:, 0:2] = rng.uniform(-5, 5, (R, 2))
    s[:, 2:4] = rng.uniform(-1, 1, (R, 2))
    s[:, 4] = 0.3
    s[:, 5:7] = rng.uniform(-5, 5, (R, 2))
    s[:, 7] = 1.0
    s[:, 8] = rng.uniform(-np.pi, np.pi, R)
    s[:, 9:11] = s[:, 0:2] + rng.uniform(-3, 3, (R, 2))
    s[:, 11:13] = rng.uniform(-1, 1, (R, 2))
    s[:, 13] = rng.uniform(0.2, 0.5, R)
    k = np.arange(R) % 8
    s[k == 1, 5:7] = s[k == 1, 0:2]
    s[k == 2, 6] = s[k == 2, 1]
    s[k == 3, 5] = s[k == 3, 0]
    big = k == 4
    s[big, 0:2] *= F32(4096.0)
    s[big, 5:7] *= F32(-4096.0)
    s[big, 9:11] = s[big, 0:2] + rng.uniform(-3, 3, (int(big.sum()), 2)).astype(F32)
    den = np.nonzero(k == 5)[0]
    tiny = (rng.randint(-2000, 2000, (len(den), 2)) * 1e-42).astype(F32)                 # multiples of 1e-42: subnormal float32
    s[den, 0:2] = 0.0
    s[den, 5:7] = tiny
    return s


def with_probes(rows):
    """(R,14) -> (3R,14): every row followed by its two probe rows (same px, py, gx, gy): one with velocity (1, 0) -- columns 4
    and 5 of its features are c and -sn exactly -- and one with theta = 0 -- column 2 is -rot exactly under unicycle."""
    out = np.repeat(np.asarray(rows, F32), 3, axis=0)
    out[1::3, 2], out[1::3, 3] = 1.0, 0.0
    out[2::3, 8] = 0.0
    return out


def trig_from_probes(holonomic13, unicycle13):
    """The device's (rot, c, sn) of every test row, from the features of with_probes(rows) under the two kinematics."""
    with np.errstate(all="ignore"):
        return -unicycle13[2::3, 2], holonomic13[1::3, 4] + F32(0), -holonomic13[1::3, 5]


UNICYCLE_CASES = [(6, 5, 811), (3, 64, 812), (2, 127, 813)]           # (B, H, seed) of probe_scenes for the unicycle family


def probe_scenes(rng, B, H, float64_roots=False):
    """tests.helpers.dense_scenes' recipe (copied: this module imports nothing of the project) with human H - 1 made the probe:
    velocity (1, 0), so that columns 2 and 3 of its hum7 row are c and -sn of its (root, action) pair.  -> (robot (B,9), humans
    (B,H,5)) float32 and, with `float64_roots`, the float64 arrays they were rounded from (not float32 numbers)."""
    robot = np.zeros((B, 9), F32)
    robot[:, 0:2] = rng.uniform(-3, 3, (B, 2))
    robot[:, 2:4] = rng.uniform(-0.5, 0.5, (B, 2))
    robot[:, 4] = 0.3
    robot[:, 5:7] = robot[:, 0:2] + rng.uniform(-0.6, 0.6, (B, 2)) * (rng.rand(B, 1) < 0.3) + rng.uniform(-4, 4, (B, 2)) * (rng.rand(B, 1) < 0.7)
    robot[:, 7] = 1.0
    robot[:, 8] = rng.uniform(-np.pi, np.pi, B)
    humans = np.zeros((B, H, 5), F32)
    ang = rng.uniform(0, 2 * np.pi, (B, H))
    rad = np.where(rng.rand(B, H) < 0.25, rng.uniform(0.45, 1.6, (B, H)), rng.uniform(1.6, 6.0, (B, H)))
    humans[:, :, 0] = robot[:, None, 0] + rad * np.cos(ang)
    humans[:, :, 1] = robot[:, None, 1] + rad * np.sin(ang)
    humans[:, :, 2:4] = rng.uniform(-1, 1, (B, H, 2))
    humans[:, :, 4] = 0.3
    humans[:, H - 1, 2], humans[:, H - 1, 3] = 1.0, 0.0
    if not float64_roots:
        return robot, humans, None
    r64, h64 = robot.astype(F64), humans.astype(F64)
    r64[:, [0, 1, 5, 6]] += rng.uniform(-1e-8, 1e-8, (B, 4))
    h64[:, :, 0:2] += rng.uniform(-1e-8, 1e-8, (B, H, 2))
    return r64.astype(F32), h64.astype(F32), (r64, h64)


def trig_from_probe_human(hum7, B, A):
    """(rot unknown: zeros, c, sn) (B,A) of every (root, action) pair from the probe human's hum7 row (the last human)."""
    with np.errstate(all="ignore"):
        p = np.asarray(hum7, F32).reshape(B, A, -1, 7)[:, :, -1, :]
        return np.zeros((B, A), F32), p[:, :, 2] + F32(0), -p[:, :, 3]


def dyadic_table(A, duplicates=()):
    """A holonomic velocities on a 0.25 m/s grid (end points 1/16 m apart at dt = 0.25); `duplicates`: pairs (k1, k2), row k2 made
    a copy of row k1."""
    a = np.arange(A)
    t = np.stack([(a % 16) * 0.25 - 2.0, (a // 16) * 0.25 - 2.0], axis=1)
    for k1, k2 in duplicates:
        t[k2] = t[k1]
    return t


def lane_scenes(table, targets, H, v_pref, dt=0.25):
    """One scene per entry of `targets`: the goal sits exactly on the end point of that table row (-1: out of every action's reach),
    robot radius 1/64 -- only that action (and its duplicates) reaches -- humans far away.  Dyadic float32 numbers."""
    B = len(targets)
    robot = np.zeros((B, 9), F32)
    robot[:, 0], robot[:, 1] = 3.0, -1.5
    robot[:, 4] = 1.0 / 64
    for b, k in enumerate(targets):
        robot[b, 5:7] = (robot[b, 0:2] + table[k] * dt) if k >= 0 else (robot[b, 0:2] + 16.0)
    robot[:, 7] = v_pref
    humans = np.zeros((B, H, 5), F32)
    humans[:, :, 0] = robot[:, None, 0] + 32.0 + np.arange(H)[None, :]
    humans[:, :, 1] = robot[:, None, 1] - 32.0
    humans[:, :, 4] = 0.25
    return robot, humans
