"""ORCA on the MI355X (-m gpu): the device kernel against the float32 restatement bit for bit, the reference's recorded ORCA
episodes (tests/golden/orca.npz) step by step and free-running, BatchedCrowdSim(human_policy="orca"), imitation learning
through VectorExplorer with OrcaPolicy, and the reference-facing ORCA / CentralizedORCA classes."""
import numpy as np
import pytest
import torch

from relationalgraphlearning_amd.orca import (ORCA, CentralizedORCA, OrcaParams, OrcaPolicy, orca_human_velocities,
                                              orca_robot_velocity)
from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig
from tests import golden_io as gio
from tests import orca_cpu as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def random_crowds(rng, B, H):
    """B environments drawn to reach every branch: tight clusters (overlaps: the collision case), crowds wider than
    max_neighbors, fast head-on velocities (cut-off circles, both legs, infeasible sets for LP3), goals near and far."""
    spread = rng.choice([0.8, 1.5, 3.0, 6.0], B)[:, None, None]
    humans = np.zeros((B, H, 5))
    humans[:, :, :2] = rng.uniform(-1, 1, (B, H, 2)) * spread
    humans[:, :, 2:4] = rng.uniform(-1.3, 1.3, (B, H, 2))
    humans[:, :, 4] = rng.uniform(0.25, 0.5, (B, H))
    goals = humans[:, :, :2] + rng.uniform(-1, 1, (B, H, 2)) * rng.choice([0.5, 8.0], (B, H, 1))
    vpref = rng.uniform(0.5, 1.5, (B, H))
    robot = np.zeros((B, 9))
    robot[:, :2] = rng.uniform(-1, 1, (B, 2)) * spread[:, 0]
    robot[:, 2:4] = rng.uniform(-1, 1, (B, 2))
    robot[:, 4] = 0.3
    robot[:, 5:7] = rng.uniform(-5, 5, (B, 2))
    robot[:, 7] = rng.uniform(0.5, 1.5, B)
    return robot, humans, goals, vpref


@pytest.mark.parametrize("H", [1, 5, 10, 19, 30])
def test_device_matches_the_restatement_bit_for_bit(dev, H):
    """Same operation sequence, IEEE float32, no contraction, correctly rounded division and square root: identical bits.
    Half the environments see the robot (centralized), the other half plan decentralized with their own v_pref."""
    rng = np.random.RandomState(100 + H)
    B = 2048
    robot, humans, goals, vpref = random_crowds(rng, B, H)
    half = B // 2
    t = lambda x: torch.tensor(x, dtype=torch.float64, device=dev)          # noqa: E731
    out = torch.cat([orca_human_velocities(t(robot[:half]), t(humans[:half]), t(goals[:half]), None, robot_visible=True),
                     orca_human_velocities(t(robot[half:]), t(humans[half:]), t(goals[half:]), t(vpref[half:]),
                                           robot_visible=False, centralized=False)]).cpu().numpy()
    rob = orca_robot_velocity(t(robot), t(humans), params=OrcaParams(safety_space=0.15)).cpu().numpy()
    assert np.array_equal(out, out.astype(np.float32).astype(np.float64))
    assert np.array_equal(rob, rob.astype(np.float32).astype(np.float64))
    check = range(B) if H <= 10 else range(0, B, 4)          # the restatement is a Python loop: a quarter of the big crowds
    seen = set()
    for b in check:
        infos = []
        exp = oc.humans_velocities(robot[b], humans[b], goals[b], vpref[b], b < half, centralized=b < half, infos=infos)
        assert np.array_equal(out[b], exp), (b, out[b], exp)
        assert np.array_equal(rob[b], oc.robot_velocity(robot[b], humans[b], safety_space=0.15)), b
        for i in infos:
            seen.update(i["branches"])
            seen.update(["lp3"] if i["lp3"] else [])
            seen.update(["full"] if len(i["neighbours"]) == 10 else [])
    if H >= 10:
        assert {"cutoff", "left", "right", "collision", "lp3"} <= seen, seen
    if H >= 19:
        assert "full" in seen


def test_done_environments_are_skipped(dev):
    rng = np.random.RandomState(3)
    robot, humans, goals, _ = random_crowds(rng, 64, 5)
    t = lambda x: torch.tensor(x, dtype=torch.float64, device=dev)          # noqa: E731
    done = torch.zeros(64, dtype=torch.int32, device=dev)
    done[::3] = 1
    out = torch.full((64, 5, 2), 7.0, dtype=torch.float64, device=dev)
    orca_human_velocities(t(robot), t(humans), t(goals), done=done, out=out)
    full = orca_human_velocities(t(robot), t(humans), t(goals))
    assert bool((out[::3] == 7.0).all())
    keep = done == 0
    assert torch.equal(out[keep], full[keep])


def orca_cases():
    return [str(c).split("|") for c in gio.load("orca")["orca_cases"]]


def _sim_config(case):
    tag, phase, k, scenario, H, visible, centralized, randomize = case[:8]
    return SimConfig(scenario=scenario, human_num=int(H), robot_visible=visible == "1", centralized_planning=centralized == "1",
                     randomize_attributes=randomize == "1")


@pytest.mark.parametrize("case", orca_cases(), ids=lambda c: c[0])
def test_replay_of_the_reference_orca_episodes(dev, case):
    """Every recorded step i of the reference's CrowdSim at once (one environment per step): the ORCA velocities of the humans
    (and of the robot where ORCA drives it) equal the reference's; stepping with GIVEN reaches state i+1 (atol 1e-9, as
    test_device_step_against_reference_trajectories)."""
    g = gio.load("orca")
    tag, visible, centralized, driver, safety = case[0], case[5] == "1", case[6] == "1", case[8], float(case[9])
    k = "orca.%s." % tag
    R, Hs, T = g[k + "robot"], g[k + "humans"], len(g[k + "info"])
    cfg = _sim_config(case)
    hv = orca_human_velocities(torch.tensor(R[:T], device=dev), torch.tensor(Hs[:T, :, :5], device=dev),
                               torch.tensor(Hs[:T, :, 5:7], device=dev), torch.tensor(Hs[:T, :, 7], device=dev),
                               robot_visible=visible, params=OrcaParams(), centralized=centralized).cpu().numpy()
    assert np.array_equal(hv, g[k + "human_vel"]), tag
    if driver == "orca":
        rv = orca_robot_velocity(torch.tensor(R[:T], device=dev), torch.tensor(Hs[:T, :, :5], device=dev),
                                 params=OrcaParams(safety_space=safety)).cpu().numpy()
        assert np.array_equal(rv, g[k + "robot_vel"]), tag
    sim = BatchedCrowdSim(dev, cfg, human_policy="given")
    sim.load(R[:T], Hs[:T, :, :5], Hs[:T, :, 5:7], Hs[:T, :, 7])
    sim.time.copy_(torch.tensor(g[k + "time"][:T], device=dev))
    _, reward, done, info = sim.step(g[k + "robot_vel"], g[k + "human_vel"])
    assert np.allclose(sim.robot.cpu().numpy(), R[1:T + 1], rtol=0, atol=1e-9)
    assert np.allclose(sim.humans.cpu().numpy()[:, :, :4], Hs[1:T + 1, :, :4], rtol=0, atol=1e-9)
    assert np.allclose(reward.cpu().numpy(), g[k + "reward"], rtol=0, atol=1e-7)
    assert np.array_equal(info.cpu().numpy(), g[k + "info"]) and np.array_equal(done.cpu().numpy().astype(int), g[k + "done"])


@pytest.mark.parametrize("case", orca_cases(), ids=lambda c: c[0])
def test_free_running_orca_episodes_reach_the_reference_outcome(dev, case):
    g = gio.load("orca")
    tag, phase, num, driver, safety = case[0], case[1], int(case[2]), case[8], float(case[9])
    k = "orca.%s." % tag
    sim = BatchedCrowdSim(dev, _sim_config(case), human_policy="orca")
    sim.reset(phase, [num])
    assert np.array_equal(sim.robot.cpu().numpy()[0], g[k + "robot"][0])
    assert np.array_equal(sim.humans.cpu().numpy()[0], g[k + "humans"][0][:, :5])
    table = gio.load("sim")["sim.action_table"]
    infos = []
    for _ in range(len(g[k + "info"]) + 5):
        if bool(sim.done.any()):
            break
        if driver == "orca":
            act = orca_robot_velocity(sim.robot, sim.humans, params=OrcaParams(safety_space=safety))
        else:
            r = sim.robot.cpu().numpy()[0]
            act = table[int(np.argmax(table @ np.array([r[5] - r[0], r[6] - r[1]])))][None]
        _, _, _, info = sim.step(act)
        infos.append(int(info[0]))
    assert len(infos) == len(g[k + "info"]) and infos[-1] == g[k + "info"][-1], (tag, infos, g[k + "info"])


def _run(sim, steps):
    traj = []
    for _ in range(steps):
        r = sim.robot.cpu().numpy()
        to_goal = r[:, 5:7] - r[:, 0:2]
        act = to_goal / np.maximum(np.linalg.norm(to_goal, axis=1, keepdims=True), 1.0)
        sim.step(act)
        traj.append((sim.robot.clone(), sim.humans.clone(), sim.done.clone()))
    return traj


def test_orca_sim_is_deterministic_and_batch_independent(dev):
    a = BatchedCrowdSim(dev, human_policy="orca")
    a.reset("test", list(range(64)))
    ta = _run(a, 40)
    b = BatchedCrowdSim(dev, human_policy="orca")
    b.reset("test", list(range(64)))
    tb = _run(b, 40)
    c = BatchedCrowdSim(dev, human_policy="orca")
    c.reset("test", [7])
    tc = _run(c, 40)
    for (ra, ha, da), (rb, hb, db), (rc, hc, dc) in zip(ta, tb, tc):
        assert torch.equal(ra, rb) and torch.equal(ha, hb) and torch.equal(da, db)
        assert torch.equal(ra[7], rc[0]) and torch.equal(ha[7], hc[0]) and torch.equal(da[7], dc[0])
    # environments that finished stay frozen
    ended = [(i, t) for t, (_, _, d) in enumerate(ta) for i in range(64) if bool(d[i]) and (t == 0 or not bool(ta[t - 1][2][i]))]
    assert ended
    for i, t in ended:
        for r, h, _ in ta[t + 1:]:
            assert torch.equal(r[i], ta[t][0][i]) and torch.equal(h[i], ta[t][1][i])


def _min_human_gap(humans):
    p, r = humans[:, :, None, :2] - humans[:, None, :, :2], humans[:, :, 4]
    d = torch.linalg.norm(p, dim=-1) - r[:, :, None] - r[:, None, :]
    H = humans.shape[1]
    d = d + torch.eye(H, device=humans.device, dtype=humans.dtype)[None] * 1e9
    return float(d.min())


@pytest.mark.parametrize("policy", ["orca", "linear"])
def test_orca_humans_do_not_overlap(dev, policy):
    """256 cases x 120 steps, invisible robot walking to its goal: ORCA humans keep apart (1e-3 m), linear ones do not."""
    sim = BatchedCrowdSim(dev, SimConfig(time_limit=1e9), human_policy=policy)
    sim.reset("test", list(range(256)))
    worst = 0.0
    for _ in range(120):
        r = sim.robot.cpu().numpy()
        to_goal = r[:, 5:7] - r[:, 0:2]
        sim.step(to_goal / np.maximum(np.linalg.norm(to_goal, axis=1, keepdims=True), 1.0))
        sim.done.zero_()                                 # keep every crowd moving for the whole horizon
        worst = min(worst, _min_human_gap(sim.humans))
    if policy == "orca":
        assert worst > -1e-3, worst
    else:
        assert worst < -1e-3, worst


def test_imitation_learning_with_the_orca_expert(dev):
    """train.py's imitation-learning phase: OrcaPolicy (safety_space 0.15, invisible robot) drives, ORCA humans walk, the memory
    takes returns-to-go in the ModelPredictiveRL layout, and one MPRLTrainer epoch runs on it."""
    from relationalgraphlearning_amd import MPRLTrainer, ReplayMemory, VectorExplorer
    from tests.helpers import make_mprl_policy
    pol = make_mprl_policy("trained", 1, device=dev)
    mem = ReplayMemory(100000)
    expert = OrcaPolicy(safety_space=0.15)
    ex = VectorExplorer(BatchedCrowdSim(dev, human_policy="orca"), expert, memory=mem, gamma=0.9, target_policy=pol)
    ex.run_k_episodes(48, "train", update_memory=True, imitation_learning=True)
    run = ex.last_run
    assert set(run["outcome"]) <= {2, 3, 4} and 3 in run["outcome"]
    assert all(isinstance(a, tuple) and len(a) == 2 for a in run["actions"][0])
    stored = [i for i in range(48) if run["outcome"][i] in (2, 3)]
    assert len(mem) == sum(run["length"][i] - 1 for i in stored)
    robot, humans, value, reward, nrobot, nhumans = mem[0]
    assert robot.shape == (1, 9) and humans.shape == (5, 5) and value.shape == (1,) and reward.shape == (1,)
    assert nrobot.shape == (1, 9) and nhumans.shape == (5, 5)
    d = pow(0.9, 0.25 * 1.0)                                  # gamma ** (time_step * v_pref)
    e0, n = stored[0], run["length"][stored[0]]
    rewards = [float(mem[j][3]) for j in range(n - 1)] + [_last_reward(run, e0)]
    assert abs(float(mem[0][2]) - sum(d ** j * r for j, r in enumerate(rewards))) < 1e-5     # G_0, the discounted return
    assert abs(float(mem[n - 2][2]) - (rewards[n - 2] + d * rewards[n - 1])) < 1e-5
    t = MPRLTrainer(pol.value_estimator, pol.state_predictor, mem, dev, pol, _Scalars(), 100, "Adam", 5,
                    reduce_sp_update_frequency=False, freeze_state_predictor=False, detach_state_predictor=True,
                    share_graph_model=False)
    t.set_learning_rate(1e-3)
    t.optimize_epoch(1)
    assert t.writer.scalars and all(np.isfinite(v) for _, v, _ in t.writer.scalars)


class _Scalars(object):
    """The SummaryWriter surface optimize_epoch logs its losses through."""

    def __init__(self):
        self.scalars = []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), step))


def _last_reward(run, e):
    return {3: 1.0, 2: -0.25}[int(run["outcome"][e])]


def test_reference_classes_equal_the_batched_entry_points(dev):
    from tests.helpers import JS
    rng = np.random.RandomState(11)
    robot, humans, goals, vpref = random_crowds(rng, 4, 5)
    for b in range(4):
        o = ORCA()
        o.set_time_step(0.25)
        o.safety_space = 0.15
        a = o.predict(JS(robot[b], humans[b]))
        exp = orca_robot_velocity(torch.tensor(robot[b:b + 1], device=dev), torch.tensor(humans[b:b + 1], device=dev),
                                  params=OrcaParams(safety_space=0.15)).cpu().numpy()[0]
        assert (a.vx, a.vy) == tuple(exp)
        names = ["px", "py", "vx", "vy", "radius", "gx", "gy", "v_pref", "theta"]
        rows = [list(humans[b][h]) + list(goals[b][h]) + [1.0, 0.0] for h in range(5)] + [list(robot[b])]
        c = CentralizedORCA()
        c.time_step = 0.25
        acts = c.predict([JS.Row(names, r) for r in rows])
        assert len(acts) == 6
        exp = orca_human_velocities(torch.tensor(robot[b:b + 1], device=dev), torch.tensor(humans[b:b + 1], device=dev),
                                    torch.tensor(goals[b:b + 1], device=dev), robot_visible=True).cpu().numpy()[0]
        assert [(x.vx, x.vy) for x in acts[:-1]] == [tuple(v) for v in exp]
