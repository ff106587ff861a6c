"""The simulator step on the MI355X (-m gpu) in every mode, against the float64 restatement (oracle/sim_oracle.py) and the
reference's recorded trajectories (tests/golden/sim_modes.npz): crowd_step_f64 / crowd_observe_f32 through BatchedCrowdSim,
one launch per step for the whole batch.  The inputs, and which of them are drawn again, are decided on the CPU
(tests/sim_cases.py, checked there without a device); nothing here is left out of a comparison because of device output."""
import numpy as np
import pytest
import torch

from oracle import sim_oracle as so
from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig
from tests import golden_io as gio
from tests import sim_cases as sc

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def report(name, value):
    WORST[name] = max(WORST.get(name, 0.0), float(value))


def make_env(dev, case):
    env = BatchedCrowdSim(dev, SimConfig(**case["constants"]), human_policy=case["human_policy"], kinematics=case["kinematics"])
    env.load(case["robot"], case["humans"], case["goals"], case["vpref"])
    env.time.copy_(torch.as_tensor(case["time"], dtype=torch.float64))
    env.done.copy_(torch.as_tensor(case["done"], dtype=torch.int32))
    return env


def device_step(dev, case, update):
    """One launch on a fresh environment: everything the step returns and leaves behind, as numpy."""
    env = make_env(dev, case)
    ha = case["human_actions"] if case["human_policy"] == "given" else None
    (r32, h32), reward, done, info = env.step(case["action"], ha, update=update)
    return {"robot": env.robot.cpu().numpy(), "humans": env.humans.cpu().numpy(), "time": env.time.cpu().numpy(),
            "state_done": env.done.cpu().numpy(), "reward": reward.cpu().numpy(), "done": done.cpu().numpy(),
            "info": info.cpu().numpy(), "last_dmin": env.last_dmin.cpu().numpy(), "r32": r32.cpu().numpy(), "h32": h32.cpu().numpy()}


def same_or_close(got, want, bound):
    """Largest |got - want| where they are not the same value (inf equals inf); 0 for nothing to compare."""
    if np.size(got) == 0 and np.size(want) == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        diff = np.where(got == want, 0.0, np.abs(got - want))
    assert not np.isnan(diff).any() and diff.max() <= bound, diff.max()
    return diff.max()


def compare_with_restatement(got, want, case, update, tag, bit_for_bit=False):
    bound = 0.0 if bit_for_bit else 1e-12
    frozen = case["done"].astype(bool)
    assert np.array_equal(got["info"], want["info"]), (tag, np.nonzero(got["info"] != want["info"])[0][:8])
    assert np.array_equal(got["time"], want["time"]), tag
    if update:
        assert np.array_equal(got["state_done"].astype(bool), want["done"]) and np.array_equal(got["done"], want["done"]), tag
    else:
        assert np.array_equal(got["state_done"], case["done"]) and np.array_equal(got["done"], want["done"] & ~frozen), tag
    report("robot", same_or_close(got["robot"], want["robot"], bound))
    report("humans", same_or_close(got["humans"], want["humans"], bound))
    report("last_dmin", same_or_close(got["last_dmin"], want["last_dmin"], bound))
    want32 = want["reward"].astype(np.float32)
    err = np.abs(got["reward"].astype(np.float64) - want32.astype(np.float64))
    assert np.all(err <= (0.0 if bit_for_bit else so.float32_ulp(want32))), (tag, err.max())
    report("reward (float32 ulps)", (err / so.float32_ulp(want32)).max())
    still = frozen if update else np.ones_like(frozen)
    assert np.array_equal(got["robot"][still], case["robot"][still]) and np.array_equal(got["humans"][still], case["humans"][still]), tag
    assert np.array_equal(got["time"][still], case["time"][still]), tag
    assert np.array_equal(got["r32"], got["robot"].astype(np.float32)) and np.array_equal(got["h32"], got["humans"].astype(np.float32))


# -- (a) the reference's recorded trajectories ----------------------------------------------------------------------------
def modes_groups():
    groups = {}
    for c in gio.load("sim_modes")["modes_cases"]:
        c = str(c).split("|")
        k = "modes.%s." % c[0]
        key = (c[1], c[2], int(c[7]), tuple(gio.load("sim_modes")[k + "constants"]))
        groups.setdefault(key, []).append(c[0])
    return sorted(groups.items())


@pytest.mark.parametrize("group", modes_groups(), ids=lambda g: "-".join(g[1]))
def test_device_replays_reference_modes(dev, group):
    """Every trajectory of one shape and setting in one batch, every step compared with what the reference produced."""
    (kinematics, policy, H, constants), tags = group
    sim = gio.load("sim_modes")
    table = sim["modes.table." + kinematics]
    key = lambda t, what: sim["modes.%s.%s" % (t, what)]          # noqa: E731
    n_steps = max(len(key(t, "actions")) for t in tags)
    env = BatchedCrowdSim(dev, SimConfig(**dict(zip(sc.CONSTANT_KEYS, constants))), human_policy=policy, kinematics=kinematics)
    first = [key(t, "humans")[0] for t in tags]
    env.load(np.stack([key(t, "robot")[0] for t in tags]), np.stack([f[:, :5] for f in first]),
             np.stack([f[:, 5:7] for f in first]), np.stack([f[:, 7] for f in first]))
    if policy == "constant_velocity":
        assert any(np.abs(f[:, 2:4]).max() > 0 for f in first)
    finished = [False] * len(tags)
    for i in range(n_steps):
        live = [i < len(key(t, "actions")) for t in tags]
        acts = np.stack([table[key(t, "actions")[i]] if ok else table[0] for t, ok in zip(tags, live)])
        ha = np.stack([key(t, "human_actions")[i] if ok else np.zeros((H, 2)) for t, ok in zip(tags, live)]) if policy == "given" else None
        obs, reward, done, info = env.step(acts, ha)
        r, h, tm = env.robot.cpu().numpy(), env.humans.cpu().numpy(), env.time.cpu().numpy()
        reward, done, info, dmin = reward.cpu().numpy(), done.cpu().numpy(), info.cpu().numpy(), env.last_dmin.cpu().numpy()
        for e, t in enumerate(tags):
            if not live[e]:
                assert finished[e] and info[e] == 5 and reward[e] == 0
                continue
            want = key(t, "robot")[i + 1]
            assert np.allclose(r[e][:8], want[:8], rtol=0, atol=1e-12), (t, i)
            dth = abs(r[e][8] - want[8])
            assert min(dth, abs(dth - 2 * np.pi)) <= 1e-12 and 0 <= r[e][8] <= 2 * np.pi, (t, i)
            assert np.allclose(h[e][:, :4], key(t, "humans")[i + 1][:, :4], rtol=0, atol=1e-9), (t, i)
            assert abs(reward[e] - key(t, "reward")[i]) < 1e-7 and int(done[e]) == key(t, "done")[i], (t, i)
            assert info[e] == key(t, "info")[i] and abs(tm[e] - key(t, "time")[i + 1]) < 1e-12, (t, i)
            if info[e] == 1:
                assert abs(dmin[e] - key(t, "dmin")[i]) < 1e-12
            report("replay robot", np.abs(r[e][:8] - want[:8]).max())
            report("replay humans", np.abs(h[e][:, :4] - key(t, "humans")[i + 1][:, :4]).max())
            finished[e] = bool(done[e])
    assert all(finished)


# -- (b) one step, many shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.STEP_SHAPES, ids=lambda s: "B%d-H%d-%s-%s" % s)
@pytest.mark.parametrize("update", [1, 0])
def test_one_step_against_the_restatement(dev, shape, update):
    B, H, kinematics, policy = shape
    case = sc.draw_step_batch(sc.step_seed(B, H, kinematics, policy), B, H, kinematics, policy)
    want = sc.restate(case, update=bool(update))
    assert want["margin"].min() >= sc.MIN_MARGIN
    got = device_step(dev, case, bool(update))
    compare_with_restatement(got, want, case, bool(update), shape)


# -- (c) exact edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinematics", so.KINEMATICS)
@pytest.mark.parametrize("policy", ["constant_velocity", "given"])
@pytest.mark.parametrize("update", [1, 0])
def test_exact_edges_bit_for_bit(dev, kinematics, policy, update):
    """Numbers exact in binary: device and restatement agree bit for bit, and every edge gives the outcome its name states."""
    case = sc.edge_batch(kinematics, policy)
    want = sc.restate(case, update=bool(update))
    got = device_step(dev, case, bool(update))
    for b, edge in enumerate(sc.EDGES):
        assert got["info"][b] == edge[5], (edge[0], got["info"][b])
        assert edge[6] is None or got["last_dmin"][b] == edge[6], (edge[0], got["last_dmin"][b])
    compare_with_restatement(got, want, case, bool(update), (kinematics, policy), bit_for_bit=True)


# -- (d) the unicycle wrap -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["constant_velocity", "given"])
def test_unicycle_wrap(dev, policy):
    case = sc.wrap_batch(policy)
    want = sc.restate(case)
    got = device_step(dev, case, True)
    python = np.array([(t + r) % (2 * np.pi) for t, r in sc.WRAPS])
    theta = got["robot"][:, 8]
    assert np.all(np.abs(theta - python) <= 1e-15) and np.all((theta >= 0) & (theta <= 2 * np.pi)), theta - python
    sums = case["robot"][:, 8] + case["action"][:, 1]
    assert np.all(np.abs(got["robot"][:, 0] - (0.5 + np.cos(sums) * 0.25)) <= 1e-12)         # position: the un-wrapped angle
    assert np.all(np.abs(got["robot"][:, 1] - (-0.25 + np.sin(sums) * 0.25)) <= 1e-12)
    assert np.all(np.abs(got["robot"][:, 2] - np.cos(python)) <= 1e-12) and np.all(np.abs(got["robot"][:, 3] - np.sin(python)) <= 1e-12)
    assert np.all(got["info"] == so.INFO_COLLISION)               # a heading wrong by r or by a sign misses the human
    compare_with_restatement(got, want, case, True, "wrap")
    # the same headings with the human just out of reach: last_dmin carries the collision test's cos(r + theta)
    case["humans"][:, 1, 0:2] = case["robot"][:, 0:2] + (case["humans"][:, 1, 0:2] - case["robot"][:, 0:2]) * (0.9 / 0.8)
    want = sc.restate(case)
    assert np.all(want["info"] == so.INFO_DISCOMFORT) and want["margin"].min() > 1e-3
    compare_with_restatement(device_step(dev, case, True), want, case, True, "wrap, near miss")


# -- (e) containment -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", [(129, 1), (1000, 19)])
def test_every_buffer_of_the_step_stays_inside_its_allocation(dev, B, H):
    """Robot, humans, clock, done, reward, info, dmin and both observation buffers as caller-owned views into larger
    allocations filled with a sentinel: after steps in every mode the surroundings are untouched and every element inside
    was written."""
    pad = 4096
    for kinematics, policy in (("holonomic", "linear"), ("unicycle", "given"), ("unicycle", "constant_velocity")):
        case = sc.draw_step_batch(11 + B + H, B, H, kinematics, policy)
        env = BatchedCrowdSim(dev, SimConfig(**case["constants"]), human_policy=policy, kinematics=kinematics)
        big, views = {}, {}
        for name, shape, dtype, fill in (("robot", (B, 9), torch.float64, -777.25), ("humans", (B, H, 5), torch.float64, -777.25),
                                         ("time", (B,), torch.float64, -777.25), ("done", (B,), torch.int32, -77),
                                         ("r32", (B, 9), torch.float32, -777.25), ("h32", (B, H, 5), torch.float32, -777.25),
                                         ("reward", (B,), torch.float32, -777.25), ("info", (B,), torch.int32, -77),
                                         ("dmin", (B,), torch.float64, -777.25)):
            n = int(np.prod(shape))
            big[name] = (torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev), fill, n)
            views[name] = big[name][0][pad:pad + n].view(shape)
        t = lambda x: torch.as_tensor(x, dtype=torch.float64).to(dev)          # noqa: E731
        views["robot"].copy_(t(case["robot"]))
        views["humans"].copy_(t(case["humans"]))
        obs = env._load_tensors(views["robot"], views["humans"], t(case["goals"]), t(case["vpref"]), time=views["time"],
                                done=views["done"], obs=(views["r32"], views["h32"]))
        assert obs[0].data_ptr() == views["r32"].data_ptr() and env.time.data_ptr() == views["time"].data_ptr()
        env.time.copy_(t(case["time"]))
        env.done.copy_(torch.as_tensor(case["done"]).to(dev))
        ha = case["human_actions"] if policy == "given" else None
        out = (views["reward"], views["info"], views["dmin"])
        env.step(case["action"], ha, update=False, out=out)
        _, reward, _, info = env.step(case["action"], ha, out=out)
        assert reward.data_ptr() == views["reward"].data_ptr() and info.data_ptr() == views["info"].data_ptr()
        assert env.last_dmin.data_ptr() == views["dmin"].data_ptr()
        want = sc.restate(case)
        assert np.array_equal(info.cpu().numpy(), want["info"])
        same_or_close(env.last_dmin.cpu().numpy(), want["last_dmin"], 1e-12)
        env.step(case["action"], ha, out=out)
        torch.cuda.synchronize()
        for name, (buf, fill, n) in big.items():
            assert bool((buf[:pad] == fill).all()) and bool((buf[pad + n:] == fill).all()), (name, kinematics)
            assert not bool((buf[pad:pad + n] == fill).any()), name
        with pytest.raises(ValueError):
            env.step(case["action"], ha, out=(views["reward"][:-1], views["info"], views["dmin"]))
        with pytest.raises(ValueError):
            env.step(case["action"], ha, out=(views["reward"], views["info"].float(), views["dmin"]))


@pytest.mark.parametrize("H", [1, 2, 127])
def test_observation_is_the_float32_cast(dev, H):
    for B in (1, 3, 129):
        rng = np.random.RandomState(B + H)
        robot, humans = rng.uniform(-9, 9, (B, 9)) * (1 + 1e-9), rng.uniform(-9, 9, (B, H, 5)) / 3
        env = BatchedCrowdSim(dev, human_policy="constant_velocity")
        r32, h32 = env.load(robot, humans)
        assert r32.shape == (B, 9) and h32.shape == (B, H, 5)
        assert np.array_equal(r32.cpu().numpy(), robot.astype(np.float32)) and np.array_equal(h32.cpu().numpy(), humans.astype(np.float32))


# -- (f) batch independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinematics,policy", [("holonomic", "linear"), ("unicycle", "given"), ("unicycle", "constant_velocity")])
def test_batch_composition_does_not_matter(dev, kinematics, policy):
    case = sc.draw_step_batch(77, 1000, 5, kinematics, policy)
    got = device_step(dev, case, True)
    perm = np.random.RandomState(1).permutation(1000)
    per_env = ("robot", "humans", "goals", "vpref", "action", "human_actions", "time", "done")
    shuffled = device_step(dev, dict(case, **{k: case[k][perm] for k in per_env}), True)
    for k in got:
        assert np.array_equal(shuffled[k], got[k][perm], equal_nan=True), k
    for b in (0, 127, 128, 999):
        solo = device_step(dev, dict(case, **{k: case[k][b:b + 1] for k in per_env}), True)
        for k in got:
            assert np.array_equal(solo[k], got[k][b:b + 1], equal_nan=True), (k, b)


# -- (g) onestep_lookahead_actions -----------------------------------------------------------------------------------------
def lookahead_cases():
    sim = gio.load("sim_modes")
    return [str(c).split("|") for c in sim["modes_cases"] if "modes.%s.look_steps" % str(c).split("|")[0] in sim]


@pytest.mark.parametrize("case", lookahead_cases(), ids=lambda c: c[0])
def test_lookahead_over_the_action_table(dev, case):
    """Every action of the table from mid-episode states the reference recorded: next human states and rewards equal the
    restatement stepped once per action and the reference's own lookaheads; the environment is bit for bit what it was."""
    tag, kinematics, policy, H = case[0], case[1], case[2], int(case[7])
    sim = gio.load("sim_modes")
    k = "modes.%s." % tag
    table, constants = sim["modes.table." + kinematics], dict(zip(sc.CONSTANT_KEYS, (float(v) for v in sim[k + "constants"])))
    A = len(table)
    for li, step in enumerate(sim[k + "look_steps"]):
        robot, full = sim[k + "robot"][step], sim[k + "humans"][step]
        env = BatchedCrowdSim(dev, SimConfig(**constants), human_policy=policy, kinematics=kinematics)
        filler = np.random.RandomState(step).uniform(-3, 3, (2, H, 5))
        env.load(np.stack([robot + 1.0, robot, robot - 1.0]), np.stack([filler[0], full[:, :5], filler[1]]),
                 np.stack([full[:, 5:7]] * 3), np.stack([full[:, 7]] * 3))
        env.time.fill_(float(sim[k + "time"][step]))
        before = [x.clone() for x in (env.robot, env.humans, env.time, env.done)]
        nh, reward = env.onestep_lookahead_actions(table, env_index=1)
        assert all(torch.equal(a, b) for a, b in zip(before, (env.robot, env.humans, env.time, env.done)))
        nh, reward = nh.cpu().numpy(), reward.cpu().numpy()
        want = so.step_batch(np.tile(robot, (A, 1)), np.tile(full[:, :5], (A, 1, 1)), table, np.full(A, sim[k + "time"][step]),
                             goals=np.tile(full[:, 5:7], (A, 1, 1)), vpref=np.tile(full[:, 7], (A, 1)), kinematics=kinematics,
                             human_policy=policy, **constants)
        assert want["margin"].min() >= sc.MIN_MARGIN
        report("lookahead humans", same_or_close(nh, want["humans"], 1e-12))
        want32 = want["reward"].astype(np.float32)
        assert np.all(np.abs(reward.astype(np.float64) - want32) <= so.float32_ulp(want32))
        assert np.allclose(nh, sim[k + "look_humans"][li], rtol=0, atol=1e-9)
        assert np.all(np.abs(reward - sim[k + "look_reward"][li]) < 1e-7)
        assert np.array_equal(want["info"], sim[k + "look_info"][li])


def test_lookahead_over_the_action_table_with_orca_humans(dev):
    """The `orca` branch of onestep_lookahead_actions from a mid-episode state: the humans' velocities are those of the ORCA
    restatement (tests/orca_cpu.py, held bit for bit by the ORCA tests), the step is the restatement's with them supplied."""
    from tests import orca_cpu as oc
    sim = gio.load("sim_modes")
    table = sim["modes.table.holonomic"]
    A = len(table)
    seen = np.zeros(5, int)
    for tag, step in (("holo_other", 5), ("holo_other", 7), ("holo_dt", 50), ("holo_dt", 68)):
        k = "modes.%s." % tag
        robot, full = sim[k + "robot"][step], sim[k + "humans"][step]
        clock = float(sim[k + "time"][step])
        env = BatchedCrowdSim(dev, SimConfig(), human_policy="orca")
        env.load(np.stack([robot, robot + 0.5]), np.stack([full[:, :5]] * 2), np.stack([full[:, 5:7]] * 2), np.stack([full[:, 7]] * 2))
        env.time.fill_(clock)
        before = [x.clone() for x in (env.robot, env.humans, env.time, env.done)]
        nh, reward = env.onestep_lookahead_actions(table, env_index=0)
        assert all(torch.equal(a, b) for a, b in zip(before, (env.robot, env.humans, env.time, env.done)))
        vel = oc.humans_velocities(robot, full[:, :5], full[:, 5:7], full[:, 7], False, time_step=0.25, centralized=True)
        want = so.step_batch(np.tile(robot, (A, 1)), np.tile(full[:, :5], (A, 1, 1)), table, np.full(A, clock), human_policy="given",
                             human_actions=np.tile(vel, (A, 1, 1)))
        assert want["margin"].min() >= sc.MIN_MARGIN
        report("lookahead humans, orca", same_or_close(nh.cpu().numpy(), want["humans"], 1e-12))
        assert np.array_equal(nh.cpu().numpy()[:, :, 2:4], np.tile(vel, (A, 1, 1)))
        want32 = want["reward"].astype(np.float32)
        assert np.all(np.abs(reward.cpu().numpy().astype(np.float64) - want32) <= so.float32_ulp(want32))
        seen += np.bincount(want["info"], minlength=6)[:5]
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0 and seen[3] > 0, seen


# -- (h) closed loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinematics,H", [("holonomic", 5), ("holonomic", 19), ("unicycle", 5)])
def test_closed_loop_against_the_restatement(dev, kinematics, H):
    """run_episodes over 64 seeded test cases with the model-predictive policy; the restatement replays the actions it chose
    from the same scenes: same outcome and end time, every step's states within the bounds of the reference replay.  An
    environment is compared up to the first step at which the restatement's margin is below 1e-9 (at most one of the 64)."""
    from relationalgraphlearning_amd.sim import generate_scene, run_episodes
    from tests.conftest import PARITY_REPORT
    from tests.helpers import make_mprl_policy
    pol = make_mprl_policy("trained", 1, device=dev, kinematics=kinematics)
    cfg = SimConfig(human_num=H)
    env = BatchedCrowdSim(dev, cfg, kinematics=kinematics)
    log = []
    stats = run_episodes(env, pol, "test", list(range(64)), on_step=lambda t, a, info: log.append(
        [x.cpu().numpy() for x in (a, info, env.robot, env.humans, env.time, env.last_dmin)]))
    assert stats["unfinished"] == 0
    scenes = [generate_scene(cfg, "test", k) for k in range(64)]
    robot, humans, goals, vpref = (np.stack([s[i] for s in scenes]) for i in range(4))
    clock, done, compared = np.zeros(64), np.zeros(64, bool), np.ones(64, bool)
    outcome, end = np.zeros(64, int), np.zeros(64)
    for a, info, r, h, tm, dmin in log:
        want = so.step_batch(robot, humans, a, clock, goals=goals, vpref=vpref, kinematics=kinematics, done=done)
        compared &= ~(want["margin"] < sc.MIN_MARGIN)
        m = compared
        assert np.array_equal(info[m], want["info"][m])
        report("closed loop robot", same_or_close(r[m][:, :8], want["robot"][m][:, :8], 1e-12))
        dth = np.abs(r[m][:, 8] - want["robot"][m][:, 8])
        assert np.all(np.minimum(dth, np.abs(dth - 2 * np.pi)) <= 1e-12) and np.all((r[:, 8] >= 0) & (r[:, 8] <= 2 * np.pi))
        report("closed loop humans", same_or_close(h[m], want["humans"][m], 1e-9))
        assert np.all(np.abs(tm[m] - want["time"][m]) <= 1e-12)
        disc = m & (want["info"] == so.INFO_DISCOMFORT)
        same_or_close(dmin[disc], want["dmin"][disc], 1e-12)
        ended = (want["info"] >= 2) & (want["info"] <= 4)
        outcome[ended], end[ended] = want["info"][ended], np.where(want["info"] == so.INFO_TIMEOUT, cfg.time_limit, want["time"])[ended]
        robot, humans, clock, done = want["robot"], want["humans"], want["time"], want["done"]
    cut = int((~compared).sum())
    PARITY_REPORT.append("closed loop, %s H = %d: %d of 64 environments cut short by a margin below 1e-9; outcomes %s"
                         % (kinematics, H, cut, np.bincount(stats["outcome"], minlength=5).tolist()))
    assert cut <= 1
    assert np.array_equal(outcome[compared], stats["outcome"][compared])
    assert np.all(np.abs(end[compared] - stats["time"][compared]) <= 1e-12)
    if kinematics == "unicycle":
        assert any(np.abs(a[:, 1]).max() > 0 for a, *_ in log)          # the policy did turn


# -- (i) refusals before any launch ----------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched(dev):
    case = sc.draw_step_batch(5, 64, 5, "holonomic", "linear")

    def refused(env, error, *args, **kw):
        before = [x.clone() for x in (env.robot, env.humans, env.time, env.done)]
        with pytest.raises(error):
            env.step(*args, **kw)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, (env.robot, env.humans, env.time, env.done)))
    with pytest.raises(ValueError):
        BatchedCrowdSim(dev, human_policy="social_force")
    env = make_env(dev, case)
    env.kinematics = "bicycle"
    refused(env, (ValueError, nat.NativeLibraryError), case["action"])
    env = make_env(dev, case)
    env.human_goals = None                                           # linear without goals
    refused(env, (ValueError, nat.NativeLibraryError), case["action"])
    env = make_env(dev, dict(case, human_policy="given"))
    refused(env, (ValueError, nat.NativeLibraryError), case["action"])          # given, update, no actions
    env.step(case["action"], update=False)                           # ... which a lookahead does not need
    env = make_env(dev, case)
    env.H = 0
    refused(env, (ValueError, nat.NativeLibraryError), case["action"])
    # shapes (checked before the library is called)
    env = make_env(dev, dict(case, human_policy="given"))
    refused(env, ValueError, case["action"][:63], case["human_actions"])
    refused(env, ValueError, case["action"].reshape(-1), case["human_actions"])
    refused(env, ValueError, case["action"], case["human_actions"][:, :4])
    refused(env, ValueError, case["action"], case["human_actions"][:63])
    with pytest.raises(ValueError):
        env.onestep_lookahead_actions(np.zeros((81, 3)))
    with pytest.raises(ValueError):
        env.onestep_lookahead_actions(np.zeros(162))
    for bad in (-1, 64):
        with pytest.raises(ValueError):
            env.onestep_lookahead_actions(np.zeros((81, 2)), env_index=bad)
    with pytest.raises(ValueError):
        env.onestep_lookahead_actions(np.zeros((0, 2)))


def test_zz_report_worst_deviations():
    """Not a check: hands the worst deviations the tests above measured to the parity report."""
    from tests.conftest import PARITY_REPORT
    PARITY_REPORT.append("simulator step, worst deviations measured: " + ", ".join("%s %.2e" % kv for kv in sorted(WORST.items())))
