"""ORCA on the MI355X: the reference's `orca` / `centralized_orca` policies and a batched imitation-learning expert.

The reference's crowd (crowd_sim/envs/policy/orca.py) calls Python-RVO2: one sequential CPU simulation per environment per
step.  Here RVO2 2.0's doStep for agents without obstacles runs as a HIP kernel (csrc/rgl_orca.hip) with one thread per
(environment, agent), in RVO2's own float32 arithmetic: the velocities are Python-RVO2's (neighbours are found in agent index
order rather than through a kd-tree; the two differ only on exact distance ties at the max_neighbors cut-off).

  * `orca_human_velocities` / `orca_robot_velocity`: the two entry points over B environments (float64 device tensors);
  * `ORCA`, `CentralizedORCA`: the reference's classes with its attributes and `predict` signatures (one launch for one
    environment), so that `register(crowd_sim.envs.policy.policy_factory.policy_factory)` lets the reference's own CrowdSim,
    train.py and test.py run without rvo2;
  * `OrcaPolicy`: a batched acting policy (`acts_in_velocity`) whose `predict_batch` returns the robot's ORCA velocities for
    every environment at once -- the imitation-learning expert of train.py:143-154 for `VectorExplorer`.

One difference from the reference, by design: its policy objects keep their RVO2 simulator between calls while the agent count
stays the same, so agents keep the radius and max_speed of the first state they were built from; here every call reads the
state it is given (the same thing whenever radii do not change between episodes, i.e. without randomize_attributes).
"""
import ctypes as C

import torch

from . import _native as nat
from .actions import ActionXY
from .nets import _stream


class OrcaParams(object):
    """ORCA.__init__'s settings (crowd_sim/envs/policy/orca.py:58-67); time_step is the simulator's."""

    def __init__(self, time_step=0.25, neighbor_dist=10.0, max_neighbors=10, time_horizon=5.0, safety_space=0.0):
        self.time_step, self.neighbor_dist, self.max_neighbors = time_step, neighbor_dist, max_neighbors
        self.time_horizon, self.safety_space = time_horizon, safety_space

    def native(self, centralized=True):
        p = nat.CrowdOrcaParams()
        p.time_step, p.neighbor_dist, p.time_horizon = float(self.time_step), float(self.neighbor_dist), float(self.time_horizon)
        p.safety_space, p.max_neighbors = float(self.safety_space), int(self.max_neighbors)
        p.max_speed_rule = nat.ORCA_MAX_SPEED_RULES["one" if centralized else "v_pref"]
        return p


def _f64(x, device):
    return torch.as_tensor(x, dtype=torch.float64).to(device).contiguous()


def _done_ptr(done, device):
    if done is None:
        return None, None
    d = torch.as_tensor(done).to(device=device, dtype=torch.int32).contiguous()
    return d, d.data_ptr()


def orca_human_velocities(robot, humans, human_goals, human_vpref=None, done=None, robot_visible=False, params=None,
                          centralized=True, out=None):
    """crowd_orca_humans_f64: the humans' ORCA velocities (B,H,2) float64 on the device of `humans`.
    robot (B,9), humans (B,H,5), human_goals (B,H,2) float64; human_vpref (B,H) is each human's max_speed when not
    `centralized`.  Rows of environments with done != 0 are left as they are in `out`."""
    humans = torch.as_tensor(humans)
    dev = humans.device
    robot, humans, goals = _f64(robot, dev), _f64(humans, dev), _f64(human_goals, dev)
    B, H = humans.shape[0], humans.shape[1]
    vpref = None if human_vpref is None else _f64(human_vpref, dev)
    _keep, dptr = _done_ptr(done, dev)
    if out is None:
        out = torch.zeros(B, H, 2, dtype=torch.float64, device=dev)
    p = (params or OrcaParams()).native(centralized)
    with torch.cuda.device(dev):
        rc = nat.lib().crowd_orca_humans_f64(C.byref(p), robot.data_ptr(), humans.data_ptr(), goals.data_ptr(),
                                             None if vpref is None else vpref.data_ptr(), dptr, B, H, int(bool(robot_visible)),
                                             out.data_ptr(), _stream())
    nat.check(rc, "crowd_orca_humans_f64")
    return out


def orca_robot_velocity(robot, humans, done=None, params=None, out=None):
    """crowd_orca_robot_f64: the robot's ORCA velocity (B,2) float64 (ORCA.predict with the robot as agent 0)."""
    humans = torch.as_tensor(humans)
    dev = humans.device
    robot, humans = _f64(robot, dev), _f64(humans, dev)
    B, H = humans.shape[0], humans.shape[1]
    _keep, dptr = _done_ptr(done, dev)
    if out is None:
        out = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    p = (params or OrcaParams()).native(True)
    with torch.cuda.device(dev):
        rc = nat.lib().crowd_orca_robot_f64(C.byref(p), robot.data_ptr(), humans.data_ptr(), dptr, B, H, out.data_ptr(),
                                            _stream())
    nat.check(rc, "crowd_orca_robot_f64")
    return out


def _device(policy):
    d = getattr(policy, "device", None)
    if d is not None and torch.device(d).type == "cuda":
        return torch.device(d)
    return torch.device("cuda", torch.cuda.current_device())


def _full_row(s):
    return [s.px, s.py, s.vx, s.vy, s.radius, s.gx, s.gy, s.v_pref, getattr(s, "theta", 0.0)]


class ORCA(object):
    """The reference's ORCA policy (crowd_sim/envs/policy/orca.py:7-125) on the device.  `predict(JointState)` returns the
    ORCA velocity of `state.robot_state` (agent 0: max_speed its v_pref, preferred velocity toward its goal) among the
    observable `state.human_states` -- the robot's imitation-learning expert and, under decentralized planning, each human."""

    def __init__(self):
        self.name = 'ORCA'
        self.trainable = False
        self.multiagent_training = True
        self.kinematics = 'holonomic'
        self.safety_space = 0
        self.neighbor_dist = 10
        self.max_neighbors = 10
        self.time_horizon = 5
        self.time_horizon_obst = 5
        self.radius = 0.3
        self.max_speed = 1
        self.sim = None
        self.phase = None
        self.model = None
        self.device = None
        self.last_state = None
        self.time_step = None
        self.env = None

    # the reference Policy's plumbing (crowd_sim/envs/policy/policy.py)
    def configure(self, config):
        return

    def set_phase(self, phase):
        self.phase = phase

    def set_device(self, device):
        self.device = device

    def set_env(self, env):
        self.env = env

    def set_time_step(self, time_step):
        self.time_step = time_step

    def get_model(self):
        return self.model

    def params(self):
        if self.time_step is None:
            raise ValueError('Time step is None')
        return OrcaParams(self.time_step, self.neighbor_dist, self.max_neighbors, self.time_horizon, self.safety_space)

    def predict(self, state):
        dev = _device(self)
        robot = torch.tensor([_full_row(state.robot_state)], dtype=torch.float64)
        humans = torch.tensor([[[h.px, h.py, h.vx, h.vy, h.radius] for h in state.human_states]], dtype=torch.float64)
        if humans.shape[1] == 0:
            raise ValueError('ORCA.predict needs at least one other agent')
        v = orca_robot_velocity(robot.to(dev), humans.to(dev), params=self.params()).cpu().numpy()[0]
        self.last_state = state
        return ActionXY(float(v[0]), float(v[1]))


class CentralizedORCA(ORCA):
    """CentralizedORCA.predict (orca.py:128-161): every agent of `state` (a list of full states) plans with max_speed 1 and
    its preferred velocity toward its goal; returns one ActionXY per agent (CrowdSim.step drops the robot's, the last)."""

    def predict(self, state):
        dev = _device(self)
        rows = torch.tensor([_full_row(s) for s in state], dtype=torch.float64)
        humans = rows[:, :5].unsqueeze(0)
        goals = rows[:, 5:7].unsqueeze(0)
        v = orca_human_velocities(rows[:1].to(dev), humans.to(dev), goals.to(dev), robot_visible=False,
                                  params=self.params(), centralized=True).cpu().numpy()[0]
        return [ActionXY(float(x), float(y)) for x, y in v]


def register(crowd_sim_policy_factory):
    """Install 'orca' and 'centralized_orca' into the reference's crowd_sim policy factory
    (crowd_sim/envs/policy/policy_factory.py), replacing the rvo2-backed classes."""
    crowd_sim_policy_factory['orca'] = ORCA
    crowd_sim_policy_factory['centralized_orca'] = CentralizedORCA
    return crowd_sim_policy_factory


class OrcaPolicy(object):
    """Batched ORCA for the robot: `predict_batch(robot, humans)` -> (B,2) float64 velocities (vx, vy), one launch for all
    environments.  `acts_in_velocity` tells VectorExplorer to step the simulator with these velocities directly.  Give it the
    simulator's float64 state (VectorExplorer does) for the reference's numbers: ORCA rounds positions and velocities to float32
    itself, but radii and preferred velocities are formed in float64 first.  Holonomic robots only, as in the reference
    (an ActionXY for a unicycle robot fails its validity check)."""
    acts_in_velocity = True

    def __init__(self, safety_space=0.0, time_step=0.25, neighbor_dist=10, max_neighbors=10, time_horizon=5):
        self.name = 'ORCA'
        self.trainable = False
        self.multiagent_training = True
        self.kinematics = 'holonomic'
        self.safety_space, self.time_step = safety_space, time_step
        self.neighbor_dist, self.max_neighbors, self.time_horizon = neighbor_dist, max_neighbors, time_horizon
        self.phase = None
        self.action_space = None

    def set_phase(self, phase):
        self.phase = phase

    def set_time_step(self, time_step):
        self.time_step = time_step

    def check_kinematics(self, kinematics):
        if kinematics != 'holonomic':
            raise ValueError('ORCA acts in (vx, vy): the robot must be holonomic, not %s' % kinematics)

    def predict_batch(self, robot, humans, roots_are_joint_states=True, done=None):
        params = OrcaParams(self.time_step, self.neighbor_dist, self.max_neighbors, self.time_horizon, self.safety_space)
        return orca_robot_velocity(robot, humans, done=done, params=params)
