"""Nonstop humans on the device (csrc/rgl_nonstop.hip) against the host replay (tests/nonstop_cpu.py) and against what the
reference's own CrowdSim and Explorer recorded with sim.nonstop_human on (tests/golden/nonstop.npz)."""
import numpy as np
import pytest
import torch

from relationalgraphlearning_amd import sim as simmod
from relationalgraphlearning_amd.sim import BASE_SEED, BatchedCrowdSim, SimConfig, generate_scene_with_draws
from relationalgraphlearning_amd.vector_explorer import DeviceReplayMemory, VectorExplorer
from tests import golden_io as gio
from tests import nonstop_cases as ncs
from tests import nonstop_cpu as nc
from tests.test_nonstop_cpu import scripted_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _words(t):
    return t.cpu().numpy().view(np.uint32)


# -- the kernel, step by step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,scenario,rand,draws", ncs.CONFIGS)
def test_kernel_step_by_step_against_the_replay(dev, H, scenario, rand, draws):
    """B = 67 loaded states per round, every round from the replay's own state (tests/nonstop_cases.py says what the batches hold
    and tests/test_nonstop_cases_cpu.py checks it): attempt counts, cap flags, stream words, outcomes exact; a regenerated human
    of the square (no transcendental in its placement) bit for bit; every other state to the 1e-12 of tests/test_sim_gpu.py's
    single steps (moved humans and the circle's candidates go through the device's sin / cos)."""
    rounds = ncs.build(H, scenario, rand, draws)
    assert ncs.census(rounds)["margin"] >= 1e-9
    sim = BatchedCrowdSim(dev, ncs.config(H, scenario, rand))
    for this in rounds:
        ins, outs = [i for i, _ in this], [o for _, o in this]
        stack = lambda k, src=ins: np.stack([np.asarray(x[k]) for x in src])      # noqa: E731
        sim.load(stack("robot"), stack("humans"), stack("goals"), stack("vpref"))
        sim.time.copy_(torch.from_numpy(stack("time")))
        sim.done.copy_(torch.from_numpy(stack("done").astype(np.int32)))
        sim.set_stream(stack("words"))
        _, reward, done, info = sim.step(stack("action"), policy_draws=draws)
        torch.cuda.synchronize()
        assert np.array_equal(sim.last_attempts.cpu().numpy(), stack("attempts", outs))
        assert np.array_equal(sim.nonstop_status.cpu().numpy(), stack("status", outs))
        assert np.array_equal(_words(sim.stream), stack("words", outs))
        assert np.array_equal(info.cpu().numpy(), stack("info", outs)) and np.array_equal(done.cpu().numpy(), stack("done", outs))
        got_h, got_g, got_v = sim.humans.cpu().numpy(), sim.human_goals.cpu().numpy(), sim.human_vpref.cpu().numpy()
        want_h, want_g, want_v = stack("humans", outs), stack("goals", outs), stack("vpref", outs)
        assert np.abs(got_h - want_h).max() <= 1e-12 and np.abs(got_g - want_g).max() <= 1e-12
        assert np.array_equal(got_v, want_v) and np.array_equal(got_h[:, :, 4], want_h[:, :, 4])
        assert np.abs(sim.robot.cpu().numpy() - stack("robot", outs)).max() <= 1e-12
        assert np.abs(sim.time.cpu().numpy() - stack("time", outs)).max() <= 1e-12
        assert np.abs(reward.cpu().numpy().astype(np.float64) - stack("reward", outs)).max() <= 1e-7
        placed = (stack("attempts", outs) > 0) & (got_h[:, :, 2] == 0) & (got_h[:, :, 3] == 0)
        assert placed.sum() >= 20
        if scenario == "square_crossing":
            assert np.array_equal(got_h[placed], want_h[placed]) and np.array_equal(got_g[placed], want_g[placed])
        frozen = stack("done").astype(bool)
        assert np.array_equal(got_h[frozen], stack("humans")[frozen]) and np.array_equal(_words(sim.stream)[frozen], stack("words")[frozen])


# -- the reference's trajectories, end to end ------------------------------------------------------------------------------------
@pytest.mark.parametrize("generator", ["host", "device"])
@pytest.mark.parametrize("c", scripted_cases(), ids=lambda c: c["tag"])
def test_reference_trajectories_through_the_simulator(dev, c, generator):
    """Info, done, regeneration events and the final stream exact; humans to 1e-9, robot and clock to 1e-12, reward to 1e-7
    (tests/test_sim_gpu.py's bounds for whole trajectories)."""
    fx, k = gio.load("nonstop"), "ns.%s." % c["tag"]
    sim = BatchedCrowdSim(dev, c["cfg"])
    sim.reset("test", [c["case"]] * 3, generator=generator)            # three environments of the same case
    assert sim.stream is not None and tuple(sim.stream.shape) == (3, 625)
    actions, T = fx[k + "actions"], len(fx[k + "actions"])
    attempts, infos, dones, rewards, states = [], [], [], [], []
    for t in range(T):
        _, reward, done, info = sim.step(np.repeat(actions[t][None], 3, 0), policy_draws=c["draws"])
        attempts.append(sim.last_attempts.clone()), infos.append(info), dones.append(done), rewards.append(reward)
        states.append((sim.humans.clone(), sim.human_goals.clone(), sim.human_vpref.clone(), sim.robot.clone(), sim.time.clone()))
    got = [torch.stack([st[f] for st in states]).cpu().numpy() for f in range(5)]         # every step of the trajectory
    humans = fx[k + "humans"][1:, None]
    assert np.abs(got[0] - humans[:, :, :, :5]).max() <= 1e-9 and np.abs(got[1] - humans[:, :, :, 5:7]).max() <= 1e-9
    assert np.abs(got[2] - humans[:, :, :, 7]).max() <= 1e-9
    assert np.abs(got[3] - fx[k + "robot"][1:, None]).max() <= 1e-12 and np.abs(got[4] - fx[k + "time"][1:, None]).max() <= 1e-12
    attempts = torch.stack(attempts).cpu().numpy()
    for b in range(3):
        events = [(t, h, int(attempts[t, b, h])) for t in range(T) for h in range(attempts.shape[2]) if attempts[t, b, h]]
        assert events == [tuple(e[:3]) for e in fx[k + "events"].tolist()]
        assert np.array_equal(torch.stack(infos).cpu().numpy()[:, b], fx[k + "info"])
        assert np.array_equal(torch.stack(dones).cpu().numpy()[:, b].astype(np.int64), fx[k + "done"])
        assert np.abs(torch.stack(rewards).cpu().numpy()[:, b].astype(np.float64) - fx[k + "reward"]).max() <= 1e-7
    _, log = nc.run_script(c["cfg"], "test", c["case"], actions, c["draws"])
    assert np.array_equal(_words(sim.stream), np.repeat(nc.words_of(log["stream"])[None], 3, 0))
    assert int(sim.nonstop_status.sum()) == 0
    # the lookahead regenerates nothing and draws nothing
    before, humans_before = sim.stream.clone(), sim.humans.clone()
    sim.done.zero_()
    sim.onestep_lookahead(np.zeros((3, 2)))
    sim.onestep_lookahead_actions(np.zeros((4, 2)))
    assert torch.equal(sim.stream, before) and torch.equal(sim.humans, humans_before)


# -- the reference's exploring episodes --------------------------------------------------------------------------------------------
def _explorer(dev, exploration, epsilon=None, memory=None, **cfg):
    from tests.helpers import make_mprl_policy
    fx = gio.load("nonstop")
    pol = make_mprl_policy("goal", 1, device=dev)
    if epsilon is not None:
        pol.set_epsilon(epsilon)
    config = SimConfig(circle_radius=float(fx["nx.circle_radius"]), time_limit=float(fx["nx.time_limit"]), nonstop_human=True, **cfg)
    return VectorExplorer(BatchedCrowdSim(dev, config), pol, memory=memory, gamma=0.9, target_policy=pol, exploration=exploration)


def test_against_the_reference_explorers_exploring_episodes(dev):
    """tests/golden/nonstop.npz, `nx.`: the REFERENCE Explorer exploring in the train phase with nonstop humans; decisions and
    regenerations share the case's stream.  Every action, explored flag, outcome, end time and the pushed tuple count."""
    fx = gio.load("nonstop")
    memory = DeviceReplayMemory(100000)
    ex = _explorer(dev, "device", float(fx["nx.epsilon"]), memory)
    cases, ends = [int(k) for k in fx["nx.cases"]], fx["nx.steps_end"]
    want_actions = [[int(a) for a in x] for x in np.split(fx["nx.actions"], ends[:-1])]
    want_explored = [[int(c >= 0) for c in x] for x in np.split(fx["nx.choice"], ends[:-1])]
    got = {"actions": [], "explored": [], "outcome": [], "time": []}
    i = 0
    while i < len(cases):                        # one call per run of consecutive cases
        j = i
        while j + 1 < len(cases) and cases[j + 1] == cases[j] + 1:
            j += 1
        ex.case_counter["train"] = cases[i]
        ex.run_k_episodes(j - i + 1, "train", update_memory=True, episode=3)
        for k in got:
            got[k] += ex.last_run[k]
        i = j + 1
    assert got["actions"] == want_actions and got["explored"] == want_explored
    assert got["outcome"] == [int(o) for o in fx["nx.outcome"]]
    finished = np.array(got["outcome"]) != 4
    assert np.allclose(np.array(got["time"])[finished], fx["nx.time"][finished], rtol=0, atol=1e-12)
    assert len(memory) == int(fx["nx.n_tuples"].sum())


def test_test_phase_is_the_same_under_host_and_device_exploration(dev):
    """Outside `train` nothing explores, but upstream's predict still draws: the host mode skips that double in the step, the
    device mode draws it with epsilon 0.  Same trajectories, same final streams; and the streams moved past regenerations."""
    runs = {}
    for mode in ("host", "device"):
        ex = _explorer(dev, mode, 0.3)
        ex.run_k_episodes(8, "test")
        runs[mode] = (ex.last_run, _words(ex.sim.stream), ex.sim.scene_draws.cpu().numpy())
    for k in ("actions", "outcome", "time", "length"):
        assert runs["host"][0][k] == runs["device"][0][k], k
    assert np.array_equal(runs["host"][1], runs["device"][1])
    assert runs["device"][0]["explored"] == [[0] * n for n in runs["device"][0]["length"]]
    regenerated = 0
    for b in range(8):          # more words went than the scene's and the decisions': some human was regenerated
        rs = nc.seeded_stream(BASE_SEED["test"] + b, int(runs["host"][2][b]) + runs["host"][0]["length"][b])
        regenerated += int(not np.array_equal(nc.words_of(rs), runs["host"][1][b]))
    assert regenerated >= 3


def test_cap_is_reported_at_the_chunks_end(dev):
    ex = _explorer(dev, "device", 0.0, scene_max_attempts=1)
    with pytest.raises(simmod.UnplacedSceneError) as err:
        ex.run_k_episodes(16, "test")
    flagged = torch.nonzero(ex.sim.nonstop_status).flatten().tolist()
    assert flagged and err.value.cases == [("test", b) for b in flagged]


def _snapshot(sim):
    return {k: getattr(sim, k).cpu().numpy().copy() for k in ("robot", "humans", "human_goals", "human_vpref", "time", "done", "stream")}


def test_capped_human_stays_where_its_step_left_it(dev):
    """scene_max_attempts = 1 on the 1.5 m circle, 16 test cases, a standing robot, 9 steps (on the host replay: 8 environments
    get flagged, 4 regenerate without ever meeting the cap), beside the same run without a cap.  In the step that flags an
    environment the capped human is where its step left it -- moved by its action, velocity kept, goal kept -- and the whole
    environment is the replay's under the cap; an environment that was never flagged equals the uncapped run bit for bit."""
    fx = gio.load("nonstop")
    sims = {}
    for name, over in (("capped", {"scene_max_attempts": 1}), ("free", {})):
        cfg = SimConfig(circle_radius=float(fx["nx.circle_radius"]), time_limit=float(fx["nx.time_limit"]), nonstop_human=True, **over)
        sims[name] = BatchedCrowdSim(dev, cfg)
        sims[name].reset("test", list(range(16)))
    capped, free = sims["capped"], sims["free"]
    act = np.zeros((16, 2))
    flagged_before, checked = np.zeros(16, bool), 0
    for _ in range(9):
        before = _snapshot(capped)
        capped.step(act, policy_draws=1)
        free.step(act, policy_draws=1)
        after, attempts = _snapshot(capped), capped.last_attempts.cpu().numpy()
        status = capped.nonstop_status.cpu().numpy().astype(bool)
        for b in np.nonzero(status & ~flagged_before)[0]:
            o = nc.step(capped.cfg, before["robot"][b], before["humans"][b], before["human_goals"][b], before["human_vpref"][b], act[b],
                        before["time"][b], nc.stream_from_words(before["stream"][b].view(np.uint32)), policy_draws=1, max_attempts=1)
            assert o["status"] == 1 and o["margin"] >= 1e-9 and np.array_equal(o["attempts"], attempts[b])
            assert np.abs(after["humans"][b] - o["humans"]).max() <= 1e-12 and np.array_equal(after["human_goals"][b], o["goals"])
            stuck = [h for h in range(capped.H) if attempts[b, h] and (after["humans"][b, h, 2:4] != 0).any()]
            assert stuck                                                    # at the cap and not placed: the velocity is its step's
            for h in stuck:
                moved = before["humans"][b, h, :2] + after["humans"][b, h, 2:4] * capped.cfg.time_step
                assert np.abs(after["humans"][b, h, :2] - moved).max() <= 1e-12
                assert np.array_equal(after["human_goals"][b, h], before["human_goals"][b, h])
                checked += 1
        flagged_before |= status
    assert checked >= 4 and int(free.nonstop_status.sum()) == 0
    clean = ~flagged_before
    assert clean.sum() >= 2
    a, b = _snapshot(capped), _snapshot(free)
    for k in a:
        assert np.array_equal(a[k][clean], b[k][clean]), k
    regenerated = [int(not np.array_equal(a["human_goals"][e], _scene_goals(capped.cfg, e))) for e in np.nonzero(clean)[0]]
    assert sum(regenerated) >= 2                                            # the unflagged ones did regenerate


def _scene_goals(cfg, case):
    return generate_scene_with_draws(cfg, "test", int(case))[2]


# -- ORCA humans -------------------------------------------------------------------------------------------------------------------
def test_orca_humans_regenerate_as_the_replay_predicts(dev):
    """H = 5 ORCA humans, B = 8, to the time limit (the robot stands far outside the circle, so nothing ends an episode early):
    crowd_orca_humans_f64's velocities go to the nonstop step as supplied actions.  Every step is replayed on the host from the
    recorded state before it and the recorded velocities: every regeneration the replay predicts occurs with its attempt count,
    the humans agree to the single step's 1e-12 and the stream matches word for word."""
    cfg = SimConfig(nonstop_human=True)
    sim = BatchedCrowdSim(dev, cfg, human_policy="orca")
    sim.reset("test", list(range(8)))
    sim.robot[:, 1], sim.robot[:, 6] = -40.0, -44.0
    act = np.zeros((8, 2))
    T = int(round(cfg.time_limit / cfg.time_step)) - 3
    records = []
    for t in range(T):
        before = _snapshot(sim)
        _, _, done, info = sim.step(act, policy_draws=1)
        records.append((before, sim._orca.cpu().numpy().copy(), _snapshot(sim), sim.last_attempts.cpu().numpy().copy(), info.cpu().numpy()))
    assert (records[-1][4] == 4).all() and all((r[4] == 0).all() for r in records[:-1])          # nothing but the time limit
    assert int(sim.nonstop_status.sum()) == 0
    regenerations, margin = 0, np.inf
    for before, velocities, after, attempts, _ in records:
        for b in range(8):
            rs = nc.stream_from_words(before["stream"][b].view(np.uint32))
            o = nc.step(cfg, before["robot"][b], before["humans"][b], before["human_goals"][b], before["human_vpref"][b], act[b],
                        before["time"][b], rs, policy_draws=1, human_policy="given", human_actions=velocities[b])
            assert np.array_equal(o["attempts"], attempts[b])
            assert np.array_equal(nc.words_of(rs), after["stream"][b].view(np.uint32))
            assert np.abs(after["humans"][b] - o["humans"]).max() <= 1e-12 and np.abs(after["human_goals"][b] - o["goals"]).max() <= 1e-12
            regenerations += len(o["events"])
            margin = min(margin, o["margin"])
    assert regenerations >= 8 and margin >= 1e-9


def test_nonstop_off_keeps_the_plain_step(dev, monkeypatch):
    sim = BatchedCrowdSim(dev, SimConfig())
    sim.reset("test", [0, 1])
    assert sim.stream is None and sim.nonstop_status is None
    lib, names = simmod.nat.lib(), []

    class Spy(object):
        def __getattr__(self, name):
            names.append(name)
            return getattr(lib, name)
    monkeypatch.setattr(simmod.nat, "lib", lambda: Spy())
    sim.step(np.zeros((2, 2)))
    assert names == ["crowd_step_f64", "crowd_observe_f32"]
