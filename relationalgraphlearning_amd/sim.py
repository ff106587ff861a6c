"""Batched crowd simulator: B independent environments on the MI355X (float64 state, one kernel per time step).

Mirrors the parts of crowd_sim/envs/crowd_sim.py the rollout needs: seeded scene generation (`reset`, :171-247 with
`generate_human`, :117-169 -- host numpy, reproducing the reference's RNG stream so test case k is the same scene),
`step` / `onestep_lookahead` (:248-368, device: crowd_step_f64) and an Explorer-style episode loop over many
environments at once (crowd_nav/utils/explorer.py:21-111).  Humans follow the reference's `linear` policy
(crowd_sim/envs/policy/linear.py), constant velocity, externally supplied actions, or ORCA (`human_policy="orca"`: the
reference's default crowd, CentralizedORCA or per-human ORCA on device -- orca.py, csrc/rgl_orca.hip -- whose velocities
the step then applies as supplied actions).  `SimConfig.nonstop_human` (crowd_sim.py:96, 346-349) regenerates arriving humans
in the step itself, from the case's own numpy stream (crowd_step_nonstop_f64, csrc/rgl_nonstop.hip; `BatchedCrowdSim.stream`).
"""
import ctypes as C

import numpy as np
import torch

from . import _native as nat
from .nets import _stream

INFO = {0: "", 1: "Discomfort", 2: "Collision", 3: "Reaching goal", 4: "Timeout", 5: "(finished earlier)"}
HUMAN_POLICY = {"given": 0, "linear": 1, "constant_velocity": 2, "orca": 0}     # orca: crowd_orca_humans_f64, then GIVEN
BASE_SEED = {"train": 2000, "val": 0, "test": 1000}       # crowd_sim.py:185-186 with its case capacities
# Default attempt cap per human of the device generator (the reference's placement loop has none).  Measured with the host
# generator's restatement (tests/scenegen_cpu.py) over circle_crossing H = 5 (randomize_attributes off and on), 10, 19 and
# square_crossing H = 4, 12, 19 (off and on), cases test 0-499 (H = 19 circle: 0-199), val 0-99, train 0-255 and the last 64
# train cases: the largest attempt count of any single human was 30 094 (19-human circle; the next configuration, the 10-human
# circle, needed 59, every square at most 7).  Margin 8.  The cap is there to bound a launch, not to clear every case, which on
# the 19-human circle no cap does: its attempt counts have a power-law tail (of 262 144 fresh train cases, 36 took more than
# 300 000 draws under this cap and 19 were flagged, one case in 13 800; with a cap of 4 000 000 three took more than 3 000 000
# draws and one was still flagged -- profiles/scenegen.txt).  8 x 30 094 attempts are about 4 600 rounds of 64 attempts, some 20 ms
# of kernel time for one human, so a hopeless case costs a launch tens of milliseconds; the cap clears every test configuration
# eight times over and flagged none of 262 144 train cases with 15 humans or fewer.  Training on the 19-human circle wants
# scene_on_unplaced = "host" or a larger cap.
SCENE_MAX_ATTEMPTS_MEASURED = 30094
SCENE_MAX_ATTEMPTS = 8 * SCENE_MAX_ATTEMPTS_MEASURED


class SimConfig(object):
    """Attribute bag with the reference's EnvConfig defaults (crowd_nav/configs/icra_benchmark/config.py:14-52)."""

    def __init__(self, **over):
        self.time_limit, self.time_step, self.randomize_attributes = 30, 0.25, False
        self.success_reward, self.collision_penalty = 1, -0.25
        self.discomfort_dist, self.discomfort_penalty_factor = 0.2, 0.5
        self.scenario, self.square_width, self.circle_radius, self.human_num = "circle_crossing", 20, 4, 5
        self.human_radius, self.human_v_pref = 0.3, 1
        self.robot_radius, self.robot_v_pref = 0.3, 1
        self.robot_visible, self.centralized_planning = False, True          # config.py:37, 47 (read by human_policy "orca")
        # not upstream's: who generates reset()'s scenes ("host": generate_scene, memoised; "device": generate_scenes_device) and
        # the device generator's attempt cap per human and what reset() does with a case that reaches it
        self.scene_generator, self.scene_max_attempts = "host", SCENE_MAX_ATTEMPTS
        self.scene_on_unplaced = "raise"                 # device generator, a case at the cap: "raise" | "host" (generate_scene)
        # upstream's sim.nonstop_human (crowd_sim.py:96, 346-349): a human that reaches its goal is regenerated in the same step,
        # from the case's own numpy stream (BatchedCrowdSim.stream); scene_max_attempts bounds one regeneration as well
        self.nonstop_human = False
        for k, v in over.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    @staticmethod
    def from_env_config(c):
        """From the reference's EnvConfig object (same attribute names as upstream)."""
        return SimConfig(time_limit=c.env.time_limit, time_step=c.env.time_step,
                         randomize_attributes=c.env.randomize_attributes, success_reward=c.reward.success_reward,
                         collision_penalty=c.reward.collision_penalty, discomfort_dist=c.reward.discomfort_dist,
                         discomfort_penalty_factor=c.reward.discomfort_penalty_factor, scenario=c.sim.test_scenario,
                         square_width=c.sim.square_width, circle_radius=c.sim.circle_radius, human_num=c.sim.human_num,
                         human_radius=c.humans.radius, human_v_pref=c.humans.v_pref, robot_radius=c.robot.radius,
                         robot_v_pref=c.robot.v_pref, robot_visible=c.robot.visible,
                         centralized_planning=c.sim.centralized_planning,
                         nonstop_human=bool(getattr(c.sim, "nonstop_human", False)))


def generate_scene(cfg, phase, case):
    """Initial state of seeded case `case` of `phase`: (robot (9,), humans (H,5), human goals (H,2), human v_pref (H,)),
    float64.  Consumes the legacy numpy stream exactly like CrowdSim.reset/generate_human."""
    return generate_scene_with_draws(cfg, phase, case)[:4]


def generate_scene_with_draws(cfg, phase, case):
    """generate_scene plus, as a fifth value, the number of doubles (random_sample / uniform calls) it took from the case's
    stream: where the episode's exploration draws continue (vector_explorer, exploration="device")."""
    draws = 0
    rs = np.random.RandomState(BASE_SEED[phase] + case)
    R = cfg.circle_radius
    robot = np.array([0.0, -R, 0.0, 0.0, cfg.robot_radius, 0.0, R, cfg.robot_v_pref, np.pi / 2])
    # agents placed so far as columns (px, py, gx, gy, radius): the rejection tests below run as one vector expression per
    # attempt -- sqrt(dx*dx + dy*dy) element by element, the arithmetic of np.linalg.norm on a pair -- instead of two
    # np.linalg.norm calls per placed agent (20 ms per 19-human scene that way, almost all of it call overhead)
    ag = np.empty((cfg.human_num + 1, 5))
    ag[0] = (robot[0], robot[1], robot[5], robot[6], cfg.robot_radius)
    n = 1
    humans, goals, vprefs = [], [], []

    def clear_of(x, y, cx, cy, radius):        # every distance from (x, y) to the points (cx, cy) at least the margin
        dx, dy = x - cx, y - cy
        return not bool((np.sqrt(dx * dx + dy * dy) < radius + ag[:n, 4] + cfg.discomfort_dist).any())
    for _ in range(cfg.human_num):
        v_pref, radius = cfg.human_v_pref, cfg.human_radius
        if cfg.randomize_attributes:
            v_pref = rs.uniform(0.5, 1.5)
            radius = rs.uniform(0.3, 0.5)
            draws += 2
        if cfg.scenario == "circle_crossing":
            while True:
                draws += 3
                angle = rs.random_sample() * np.pi * 2
                px_noise = (rs.random_sample() - 0.5) * v_pref
                py_noise = (rs.random_sample() - 0.5) * v_pref
                px = R * np.cos(angle) + px_noise
                py = R * np.sin(angle) + py_noise
                if clear_of(px, py, ag[:n, 0], ag[:n, 1], radius) and clear_of(px, py, ag[:n, 2], ag[:n, 3], radius):
                    break
            gx, gy = -px, -py
        elif cfg.scenario == "square_crossing":
            sign = -1 if rs.random_sample() > 0.5 else 1
            draws += 1
            while True:
                draws += 2
                px = rs.random_sample() * cfg.square_width * 0.5 * sign
                py = (rs.random_sample() - 0.5) * cfg.square_width
                if clear_of(px, py, ag[:n, 0], ag[:n, 1], radius):
                    break
            while True:
                draws += 2
                gx = rs.random_sample() * cfg.square_width * 0.5 * -sign
                gy = (rs.random_sample() - 0.5) * cfg.square_width
                if clear_of(gx, gy, ag[:n, 2], ag[:n, 3], radius):
                    break
        else:
            raise NotImplementedError(cfg.scenario)
        ag[n] = (px, py, gx, gy, radius)
        n += 1
        humans.append([px, py, 0.0, 0.0, radius])
        goals.append([gx, gy])
        vprefs.append(v_pref)
    return robot, np.array(humans), np.array(goals), np.array(vprefs, dtype=np.float64), draws


class UnplacedSceneError(RuntimeError):
    """The device generator gave up on some cases (`cases`: their (phase, case) pairs)."""

    def __init__(self, message, cases):
        RuntimeError.__init__(self, message)
        self.cases = cases


def _scene_config(cfg):
    if cfg.scenario not in nat.CROWD_SCENARIOS:
        raise NotImplementedError(cfg.scenario)
    c = nat.CrowdSceneConfig()
    c.circle_radius, c.square_width, c.discomfort_dist = cfg.circle_radius, cfg.square_width, cfg.discomfort_dist
    c.robot_radius, c.robot_v_pref = cfg.robot_radius, cfg.robot_v_pref
    c.human_radius, c.human_v_pref = cfg.human_radius, cfg.human_v_pref
    c.scenario, c.randomize_attributes = nat.CROWD_SCENARIOS[cfg.scenario], int(bool(cfg.randomize_attributes))
    c.max_attempts = int(cfg.scene_max_attempts)
    return c


def _seed_tensor(phase, cases, device):
    """The cases' numpy seeds BASE_SEED[phase] + case, as the int32 bit patterns of uint32 values on `device`."""
    seeds = np.asarray([int(k) for k in cases], np.int64) + BASE_SEED[phase]
    if len(seeds) == 0 or seeds.min() < 0 or seeds.max() > 0xFFFFFFFF:
        raise ValueError("cases must be a non-empty list whose seeds (%d + case) fit 32 bits" % BASE_SEED[phase])
    return torch.from_numpy(seeds.astype(np.uint32).view(np.int32)).to(device)


def _launch_scene_generator(cfg, phase, cases, device):
    """crowd_generate_scenes_f64 for `cases`: (robot, humans, goals, v_pref, status, draws) on `device`, flagged cases and all."""
    device = torch.device(device)
    if len(cases) == 0:
        raise ValueError("cases must be a non-empty list whose seeds (%d + case) fit 32 bits" % BASE_SEED[phase])
    B, H = len(cases), int(cfg.human_num)
    seeds_d = _seed_tensor(phase, cases, device)
    robot = torch.empty(B, 9, dtype=torch.float64, device=device)
    humans = torch.empty(B, H, 5, dtype=torch.float64, device=device)
    goals = torch.empty(B, H, 2, dtype=torch.float64, device=device)
    vpref = torch.empty(B, H, dtype=torch.float64, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    draws = torch.empty(B, dtype=torch.int32, device=device)
    c = _scene_config(cfg)
    with torch.cuda.device(device):
        rc = nat.lib().crowd_generate_scenes_f64(C.byref(c), seeds_d.data_ptr(), B, H, robot.data_ptr(), humans.data_ptr(),
                                                 goals.data_ptr(), vpref.data_ptr(), status.data_ptr(), draws.data_ptr(),
                                                 _stream())
    nat.check(rc, "crowd_generate_scenes_f64")
    return robot, humans, goals, vpref, status, draws


def generate_scenes_device(cfg, phase, cases, device, on_unplaced="raise"):
    """generate_scene for every case of `cases` in one launch (crowd_generate_scenes_f64): (robot (B,9), humans (B,H,5), goals
    (B,H,2), v_pref (B,H), status (B,) int32, draws (B,) int32) on `device`, float64.  Same stream, same accept / reject
    decisions as the host generator; circle_crossing positions differ from it by the device's sin / cos (a few ulp).
    A case in which some human is not placed within cfg.scene_max_attempts attempts has status 1: on_unplaced="raise" raises
    UnplacedSceneError naming those cases, "host" fills them in with generate_scene (which has no cap: like upstream, it does
    not return when there is no room for the human) and writes the host's draw count into draws[b]."""
    if on_unplaced not in ("raise", "host"):
        raise ValueError("on_unplaced must be 'raise' or 'host', not %r" % (on_unplaced,))
    cases = [int(k) for k in cases]
    robot, humans, goals, vpref, status, draws = _launch_scene_generator(cfg, phase, cases, device)
    unplaced = torch.nonzero(status).flatten().tolist()           # one synchronisation per call: the cap must not pass silently
    if unplaced:
        what = ("%d of %d %s cases were not placed within scene_max_attempts = %d attempts per human (%s, human_num = %d, "
                "randomize_attributes = %s): cases %s" % (len(unplaced), len(cases), phase, int(cfg.scene_max_attempts), cfg.scenario,
                                                          int(cfg.human_num), bool(cfg.randomize_attributes),
                                                          [cases[b] for b in unplaced]))
        if on_unplaced == "raise":
            raise UnplacedSceneError(what + ".  Raise SimConfig.scene_max_attempts, or use on_unplaced='host' (SimConfig."
                                     "scene_on_unplaced) to hand them to the host generator, which has no cap and may never "
                                     "return.", [(phase, cases[b]) for b in unplaced])
        for b in unplaced:
            r, h, g, v, d = generate_scene_with_draws(cfg, phase, cases[b])
            robot[b], humans[b], goals[b], vpref[b] = (torch.as_tensor(a, dtype=torch.float64).to(robot.device) for a in (r, h, g, v))
            draws[b] = d
    return robot, humans, goals, vpref, status, draws


def check_action_shapes(robot_actions, human_actions, B, H):
    """ValueError unless robot_actions is (B, 2) and human_actions, if any, (B, H, 2): crowd_step_f64 reads exactly that many
    values from each and knows nothing of their sizes.  Takes tensors, arrays or bare shapes; needs no device."""
    for what, x, want in (("robot_actions", robot_actions, (int(B), 2)), ("human_actions", human_actions, (int(B), int(H), 2))):
        if x is None:
            continue
        shape = tuple(x.shape) if hasattr(x, "shape") else tuple(x)
        if shape != want:
            raise ValueError("%s must have shape %s, not %s" % (what, want, shape))


class BatchedCrowdSim(object):
    def __init__(self, device, config=None, human_policy="linear", kinematics="holonomic"):
        self.cfg = config or SimConfig()
        self.device = torch.device(device)
        if human_policy not in HUMAN_POLICY:
            raise ValueError("unknown human policy %r" % human_policy)
        self.human_policy = human_policy
        self.kinematics = kinematics
        self.B = 0
        self._scene_cache = {}
        self.scene_seeds = self.scene_draws = None
        # nonstop humans (cfg.nonstop_human): the environments' numpy streams, (B, 625) int32 (624 MT19937 words and the position
        # of the next one: crowd_explore_seed_u32's layout, shared with VectorExplorer's device exploration), the cap flags that
        # steps accumulate on the device, and per human the attempts its regeneration took in the last step (0: it did not arrive)
        self.stream = self.nonstop_status = self.last_attempts = None

    # -- state ---------------------------------------------------------------------------------------------------
    def reset(self, phase, cases, generator=None):
        """Load seeded cases (one environment each).  Returns the fp32 observation (robot (B,9), humans (B,H,5)).
        generator: "host" (generate_scene per case, memoised), "device" (generate_scenes_device: one launch, nothing memoised,
        no copy through the host; an unplaced case raises or goes to the host generator, cfg.scene_on_unplaced), None: cfg.scene_generator.
        After a seeded reset `scene_seeds` and `scene_draws` hold, per environment, the case's numpy seed (the uint32 bits) and
        the number of doubles its scene took from that stream, as int32 device tensors; load() clears them."""
        generator = self.cfg.scene_generator if generator is None else generator
        if generator == "device":
            robot, humans, goals, vpref, _, draws = generate_scenes_device(self.cfg, phase, cases, self.device, self.cfg.scene_on_unplaced)
            obs = self._load_tensors(robot, humans, goals, vpref)
            self.scene_seeds, self.scene_draws = _seed_tensor(phase, cases, self.device), draws
            self._seed_stream()
            return obs
        if generator != "host":
            raise ValueError("unknown scene generator %r" % (generator,))
        scenes = []
        for k in cases:                      # scene generation is sequential host work (seeded rejection sampling): memoise
            key = (phase, int(k), self.cfg.scenario, self.cfg.human_num, self.cfg.randomize_attributes, self.cfg.circle_radius,
                   self.cfg.square_width)
            if key not in self._scene_cache:
                self._scene_cache[key] = generate_scene_with_draws(self.cfg, phase, int(k))
            scenes.append(self._scene_cache[key])
        obs = self.load(np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes]),
                        np.stack([s[2] for s in scenes]), np.stack([s[3] for s in scenes]))
        self.scene_seeds = _seed_tensor(phase, cases, self.device)
        self.scene_draws = torch.tensor([s[4] for s in scenes], dtype=torch.int32).to(self.device)
        self._seed_stream()
        return obs

    def _seed_stream(self):
        """Nonstop humans: every environment's stream where its scene left it (crowd_explore_seed_u32 of scene_seeds / scene_draws)."""
        if not self.cfg.nonstop_human:
            return
        state = torch.empty(self.B, nat.EXPLORE_STATE_WORDS, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = nat.lib().crowd_explore_seed_u32(self.scene_seeds.data_ptr(), self.scene_draws.data_ptr(), self.B, state.data_ptr(),
                                                  _stream())
        nat.check(rc, "crowd_explore_seed_u32")
        self.stream = state

    def set_stream(self, state):
        """Nonstop humans on a loaded state: the environments' streams, (B, 625) int32 or uint32 values -- 624 MT19937 words and
        the position of the next one (0..624, 624 = twist first).  The simulator keeps a device copy and advances it in place."""
        if not self.cfg.nonstop_human:
            raise ValueError("set_stream is for a simulator with SimConfig.nonstop_human on")
        if torch.is_tensor(state):
            state = state.to(self.device)
            state = state.view(torch.int32) if state.dtype == getattr(torch, "uint32", None) else state.to(torch.int32)
        else:
            state = torch.from_numpy(np.ascontiguousarray(np.asarray(state).astype(np.uint32)).view(np.int32)).to(self.device)
        if tuple(state.shape) != (self.B, nat.EXPLORE_STATE_WORDS):
            raise ValueError("the stream state must have shape (%d, %d), not %s" % (self.B, nat.EXPLORE_STATE_WORDS, tuple(state.shape)))
        self.stream = state.contiguous().clone()

    def load(self, robot, humans, human_goals=None, human_vpref=None):
        dev = self.device
        return self._load_tensors(
            torch.as_tensor(np.asarray(robot, np.float64)).to(dev).contiguous(),
            torch.as_tensor(np.asarray(humans, np.float64)).to(dev).contiguous(),
            None if human_goals is None else torch.as_tensor(np.asarray(human_goals, np.float64)).to(dev).contiguous(),
            None if human_vpref is None else torch.as_tensor(np.asarray(human_vpref, np.float64)).to(dev).contiguous())

    def _owned(self, given, shape, dtype, what):
        """A caller-owned buffer after its check, or a fresh one."""
        if given is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if (tuple(given.shape) != tuple(shape) or given.dtype != dtype or given.device != self.robot.device
                or not given.is_contiguous()):
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (what, dtype, tuple(shape), self.robot.device))
        return given

    def _load_tensors(self, robot, humans, human_goals, human_vpref, time=None, done=None, obs=None):
        """load() for contiguous float64 tensors already on the device (the simulator keeps them: its steps write in place).
        Optional caller-owned buffers, which the simulator then keeps as well: time (B,) float64 and done (B,) int32 (both
        zeroed here), obs = (robot (B, 9), humans (B, H, 5)) float32 for the observation."""
        self.robot, self.humans, self.human_goals, self.human_vpref = robot, humans, human_goals, human_vpref
        self.scene_seeds = self.scene_draws = None           # reset() sets them afterwards; loaded states have no stream to continue
        self.B, self.H = self.robot.shape[0], self.humans.shape[1]
        dev = self.device
        self.time = self._owned(time, (self.B,), torch.float64, "time").zero_()
        self.done = self._owned(done, (self.B,), torch.int32, "done").zero_()
        self._r32 = self._owned(None if obs is None else obs[0], (self.B, 9), torch.float32, "obs[0]")
        self._h32 = self._owned(None if obs is None else obs[1], (self.B, self.H, 5), torch.float32, "obs[1]")
        self._orca = torch.zeros(self.B, self.H, 2, dtype=torch.float64, device=dev) if self.human_policy == "orca" else None
        self.stream = self.nonstop_status = self.last_attempts = None      # loaded states carry no stream: set_stream()
        if self.cfg.nonstop_human:
            self.nonstop_status = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self.last_attempts = torch.zeros(self.B, self.H, dtype=torch.int32, device=dev)
        return self.observe()

    def observe(self):
        with torch.cuda.device(self.device):
            nat.check(nat.lib().crowd_observe_f32(self.robot.data_ptr(), self.humans.data_ptr(), self.B, self.H,
                                                  self._r32.data_ptr(), self._h32.data_ptr(), _stream()), "crowd_observe_f32")
        return self._r32, self._h32

    def _config(self):
        c = nat.CrowdSimConfig()
        c.time_step, c.time_limit = self.cfg.time_step, self.cfg.time_limit
        c.success_reward, c.collision_penalty = self.cfg.success_reward, self.cfg.collision_penalty
        c.discomfort_dist, c.discomfort_penalty_factor = self.cfg.discomfort_dist, self.cfg.discomfort_penalty_factor
        if self.kinematics not in nat.KINEMATICS:
            raise ValueError("unknown kinematics %r" % (self.kinematics,))
        c.kinematics = nat.KINEMATICS[self.kinematics]
        c.human_policy = HUMAN_POLICY[self.human_policy]
        return c

    def orca_params(self):
        from .orca import OrcaParams
        return OrcaParams(time_step=self.cfg.time_step)

    def _orca_humans(self, robot, humans, goals, vpref, done, out):
        """The humans' ORCA velocities for the state before anyone moves (crowd_sim.py:256-262) into `out`."""
        from .orca import orca_human_velocities
        if goals is None or (not self.cfg.centralized_planning and vpref is None):
            raise ValueError("human_policy 'orca' needs the humans' goals (and v_pref under decentralized planning)")
        return orca_human_velocities(robot, humans, goals, vpref, done, self.cfg.robot_visible, self.orca_params(),
                                     self.cfg.centralized_planning, out)

    # -- dynamics ------------------------------------------------------------------------------------------------
    def step(self, robot_actions, human_actions=None, update=True, out=None, policy_draws=0):
        """robot_actions (B,2) float64 (vx,vy)|(v,r).  Returns (obs, reward (B,) fp32, done (B,) bool, info (B,) int32);
        `self.last_dmin` holds the closest approach (Discomfort.min_dist).  Finished environments stay frozen.
        out: optional caller-owned (reward (B,) float32, info (B,) int32, dmin (B,) float64) the step writes instead of
        allocating.
        With cfg.nonstop_human an updating step is crowd_step_nonstop_f64: humans that arrive are regenerated from `self.stream`
        as upstream regenerates them (include/rgl_hip.h), after the stream of every live environment has been advanced past
        `policy_draws` doubles -- what the robot's policy drew from numpy for this decision on the host (upstream's `predict`: 1;
        0 when the draw was made on `self.stream` itself, or by a policy that draws nothing).  `self.last_attempts` (B, H) then
        holds the attempts each regeneration took, and `self.nonstop_status` (B,) accumulates 1 where one reached
        cfg.scene_max_attempts (that human stays where its step left it); nothing synchronises for it.  update=False regenerates
        nothing and draws nothing."""
        dev = self.device
        act = torch.as_tensor(robot_actions, dtype=torch.float64).to(dev).contiguous()
        ha = None if human_actions is None else torch.as_tensor(human_actions, dtype=torch.float64).to(dev).contiguous()
        check_action_shapes(act, ha, self.B, self.H)
        if ha is None and update and self.human_policy == "orca":
            ha = self._orca_humans(self.robot, self.humans, self.human_goals, self.human_vpref, self.done, self._orca)
        reward = self._owned(None if out is None else out[0], (self.B,), torch.float32, "out[0]")
        info = self._owned(None if out is None else out[1], (self.B,), torch.int32, "out[1]")
        dmin = self._owned(None if out is None else out[2], (self.B,), torch.float64, "out[2]")
        cfg = self._config()
        if self.cfg.nonstop_human and update:
            self._step_nonstop(cfg, act, ha, reward, info, dmin, policy_draws)
            self.last_dmin = dmin
            return self.observe(), reward, self.done.bool(), info
        with torch.cuda.device(dev):
            rc = nat.lib().crowd_step_f64(C.byref(cfg), self.robot.data_ptr(), self.humans.data_ptr(),
                                          None if self.human_goals is None else self.human_goals.data_ptr(),
                                          None if self.human_vpref is None else self.human_vpref.data_ptr(),
                                          act.data_ptr(), None if ha is None else ha.data_ptr(), self.time.data_ptr(),
                                          self.done.data_ptr(), self.B, self.H, int(update), reward.data_ptr(),
                                          info.data_ptr(), dmin.data_ptr(), _stream())
        nat.check(rc, "crowd_step_f64")
        self.last_dmin = dmin
        done = (info >= 2) & (info <= 4) if not update else self.done.bool()
        return self.observe(), reward, done, info

    def _step_nonstop(self, cfg, act, ha, reward, info, dmin, policy_draws):
        if self.stream is None:
            raise ValueError("nonstop humans regenerate from the case's numpy stream: reset() from seeded cases, or give the "
                             "loaded state one with set_stream()")
        if self.human_goals is None or self.human_vpref is None:
            raise ValueError("nonstop humans need the humans' goals and v_pref")
        if int(policy_draws) < 0:
            raise ValueError("policy_draws must not be negative")
        job = nat.CrowdNonstopJob()
        job.sim, job.scene = cfg, _scene_config(self.cfg)
        job.robot, job.humans = self.robot.data_ptr(), self.humans.data_ptr()
        job.human_goals, job.human_vpref = self.human_goals.data_ptr(), self.human_vpref.data_ptr()
        job.robot_action, job.human_actions = act.data_ptr(), None if ha is None else ha.data_ptr()
        job.time, job.done, job.state = self.time.data_ptr(), self.done.data_ptr(), self.stream.data_ptr()
        job.status, job.attempts = self.nonstop_status.data_ptr(), self.last_attempts.data_ptr()
        job.reward, job.info, job.dmin = reward.data_ptr(), info.data_ptr(), dmin.data_ptr()
        job.B, job.H, job.policy_draws = self.B, self.H, int(policy_draws)
        with torch.cuda.device(self.device):
            job.stream = _stream()
            rc = nat.lib().crowd_step_nonstop_f64(C.byref(job))
        nat.check(rc, "crowd_step_nonstop_f64")

    def onestep_lookahead(self, robot_actions, human_actions=None):
        return self.step(robot_actions, human_actions, update=False)

    def onestep_lookahead_actions(self, actions, env_index=0):
        """CrowdSim.onestep_lookahead (crowd_sim.py:249-250) for EVERY action of a table at once: A copies of environment
        `env_index` are stepped once on the device (the environment itself is untouched).  actions (A,2) float64 ->
        (next observable human states (A,H,5) float64, reward (A,) float32).  What path G's query_env=True asks per action
        (multi_human_rl.py:43-44)."""
        dev = self.device
        act = torch.as_tensor(actions, dtype=torch.float64).to(dev).contiguous()
        if act.dim() != 2:
            raise ValueError("actions must have shape (A, 2), not %s" % (tuple(act.shape),))
        A = act.shape[0]
        check_action_shapes(act, None, A, self.H)
        b = int(env_index)
        if A < 1 or not 0 <= b < self.B:
            raise ValueError("onestep_lookahead_actions needs at least one action and an env_index in [0, %d)" % self.B)
        robot = self.robot[b:b + 1].repeat(A, 1).contiguous()
        humans = self.humans[b:b + 1].repeat(A, 1, 1).contiguous()
        goals = None if self.human_goals is None else self.human_goals[b:b + 1].repeat(A, 1, 1).contiguous()
        vpref = None if self.human_vpref is None else self.human_vpref[b:b + 1].repeat(A, 1).contiguous()
        time = self.time[b:b + 1].repeat(A).contiguous()
        done = torch.zeros(A, dtype=torch.int32, device=dev)
        reward = torch.empty(A, dtype=torch.float32, device=dev)
        info = torch.empty(A, dtype=torch.int32, device=dev)
        dmin = torch.empty(A, dtype=torch.float64, device=dev)
        cfg = self._config()
        ha = None
        if self.human_policy == "orca":
            ha = self._orca_humans(robot, humans, goals, vpref, None, None)
        with torch.cuda.device(dev):
            rc = nat.lib().crowd_step_f64(C.byref(cfg), robot.data_ptr(), humans.data_ptr(),
                                          None if goals is None else goals.data_ptr(),
                                          None if vpref is None else vpref.data_ptr(), act.data_ptr(),
                                          None if ha is None else ha.data_ptr(),
                                          time.data_ptr(), done.data_ptr(), A, self.H, 1, reward.data_ptr(),
                                          info.data_ptr(), dmin.data_ptr(), _stream())
        nat.check(rc, "crowd_step_f64")
        return humans, reward


def run_episodes(sim, policy, phase, cases, gamma=0.9, max_steps=None, on_step=None):
    """Explorer.run_k_episodes for len(cases) environments in lock-step: the policy decides for every live environment
    at once (`predict_batch`), the simulator advances them together.  Returns per-case outcome codes, times and
    discounted cumulative rewards plus the aggregate statistics the reference logs.
    on_step(t, actions (B, 2) float64, info (B,) int32), if given, is called after every step with the actions the step took
    (device tensors; a finished environment's row is what the policy chose for its frozen state and moved nothing)."""
    robot32, humans32 = sim.reset(phase, cases)
    B = sim.B
    if policy.action_space is None:
        policy.build_action_space(sim.cfg.robot_v_pref)
    from .actions import as_array
    table = torch.tensor(as_array(policy.action_space), dtype=torch.float64, device=sim.device)
    outcome = torch.zeros(B, dtype=torch.int32, device=sim.device)
    cum = torch.zeros(B, dtype=torch.float64, device=sim.device)
    discomfort_steps = torch.zeros(B, dtype=torch.int32, device=sim.device)
    max_steps = max_steps or int(sim.cfg.time_limit / sim.cfg.time_step) + 2
    disc = 1.0
    for t in range(max_steps):
        live = sim.done == 0
        if not bool(live.any()):
            break
        act_idx, _ = policy.predict_batch(robot32, humans32, roots_are_joint_states=True)
        actions = table[act_idx.long()]
        # upstream's predict draws one np.random.random() per decision in every phase: nonstop regenerations read what follows
        (robot32, humans32), reward, done, info = sim.step(actions, policy_draws=1) if sim.cfg.nonstop_human else sim.step(actions)
        if on_step is not None:
            on_step(t, actions, info)
        cum += disc * reward.double()
        discomfort_steps += (info == 1).int()
        ended = (info >= 2) & (info <= 4)
        outcome = torch.where(ended, info, outcome)
        disc *= pow(gamma, sim.cfg.time_step * sim.cfg.robot_v_pref)
    outcome_c = outcome.cpu().numpy()
    times = sim.time.cpu().numpy()
    success, collision, timeout = outcome_c == 3, outcome_c == 2, outcome_c == 4
    nav = times[success]
    return {"outcome": outcome_c, "time": np.where(timeout, sim.cfg.time_limit, times), "cumulative_reward": cum.cpu().numpy(),
            "success_rate": float(success.mean()), "collision_rate": float(collision.mean()),
            "timeout_rate": float(timeout.mean()), "unfinished": int((outcome_c == 0).sum()),
            "avg_nav_time": float(nav.mean()) if nav.size else float(sim.cfg.time_limit),
            "discomfort_steps": discomfort_steps.cpu().numpy()}
