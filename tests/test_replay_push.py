"""The replay memory filled on the device (csrc/rgl_replay.hip through DeviceReplayMemory.push_episodes) against the code as it stands:
`ReplayMemory` filled by `VectorExplorer.update_memory`.  After the same run the two memories have equal len and position and
torch.equal rows for every item index and field -- no tolerance, no item left out (tests/replay_push.py: assert_same_memory)."""
import numpy as np
import pytest
import torch

import relationalgraphlearning_amd as rga
from relationalgraphlearning_amd.vector_explorer import DeviceReplayMemory, ReplayMemory, VectorExplorer
from tests import replay_push as rp

pytestmark = pytest.mark.gpu

T = 6
LAYOUTS = [("mprl", "holonomic"), ("gcn", "holonomic"), ("gcn", "unicycle")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _Writer(object):
    def add_scalar(self, *args):
        pass


_RUNS, _TUPLES = {}, {}


def _run(B, H, dev):
    """The synthetic chunk of (B, H) and its device tensors, built once."""
    if (B, H) not in _RUNS:
        run = rp.synthetic_run(T, B, H)
        run["device"] = tuple(torch.as_tensor(run[k]).to(dev) for k in ("robot", "humans", "rewards", "info"))
        _RUNS[(B, H)] = run
    return _RUNS[(B, H)]


def _host_tuples(B, H, layout, kinematics, il, dev):
    """What update_memory pushes for the chunk, in push order: computed once per case and shared (never modified) by the memory states
    below -- every one of which pushes these very tuples through ReplayMemory.push."""
    key = (B, H, layout, kinematics, il)
    if key not in _TUPLES:
        _TUPLES[key] = list(rp.host_fill(ReplayMemory(1 << 20), _run(B, H, dev), layout, kinematics, il, dev).memory)
    return _TUPLES[key]


def _filler(i, H, layout, dev):
    """Item i of what a memory holds before the call: distinct finite values in the layout's shapes."""
    shapes = rga.vector_explorer.REPLAY_FIELD_SHAPES[layout](H)
    return tuple(torch.full(shape, -100.0 - i - 0.01 * f, dtype=torch.float32, device=dev) for f, shape in enumerate(shapes))


def _push_device(memory, run, layout, kinematics, il, with_host_arrays=True):
    robot, humans, rewards, info = run["device"]
    extra = dict(lengths=run["lengths"], outcomes=run["outcome"]) if with_host_arrays else {}
    return memory.push_episodes(robot, humans, rewards, info, layout, kinematics, rp.STEP_DISCOUNT, il, **extra)


# capacity, pushes before, clear() after them, pushes after the clear, calls
STATES = {
    "fresh_large": (4096, 0, False, 0, 1),
    "capacity_16": (16, 0, False, 0, 1),                 # 70 episodes: some 150 tuples, the ring wraps several times
    "full_position_7": (50, 57, False, 0, 1),
    "cleared_position_ahead": (64, 41, True, 0, 1),      # position 41, nothing stored: appended from item 0
    "cleared_then_three": (64, 62, True, 3, 1),          # three pushes wrap: position 1 behind length 2 -- overwrite, then append
    "two_calls": (100, 5, False, 0, 2),
}


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("il", [True, False], ids=["il", "rl"])
@pytest.mark.parametrize("layout,kinematics", LAYOUTS)
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 70, 300])
def test_push_episodes_equals_the_host_path(B, H, layout, kinematics, il, state, dev):
    """Synthetic chunks (T = 6; episode lengths 1, 2, 3, 5 and 6; collisions, goals and time-outs; info 0 / 1 before the end; NaN in
    every row of a step past an episode's end) pushed into memories in every ring state: equal to ReplayMemory + update_memory, which
    runs the real `rotate` for "gcn".  B = 70 passes a wave of the offsets' scan, B = 300 its 256-episode pass."""
    capacity, before, clear, after, calls = STATES[state]
    run = _run(B, H, dev)
    tuples = _host_tuples(B, H, layout, kinematics, il, dev)
    assert len(tuples) == sum(L - 1 for L, o in zip(run["lengths"], run["outcome"]) if o in (2, 3))
    host, device = ReplayMemory(capacity), DeviceReplayMemory(capacity)
    for i in range(before + after):
        if clear and i == before:
            host.clear(), device.clear()
        item = _filler(i, H, layout, dev)
        host.push(item), device.push(item)
    if clear and after == 0:
        host.clear(), device.clear()
    identity = None if device.stacked_capacity_fields() is None else [f.data_ptr() for f in device.stacked_capacity_fields()]
    for _ in range(calls):
        for item in tuples:
            host.push(item)
        assert _push_device(device, run, layout, kinematics, il) == len(tuples)
    rp.assert_same_memory(device, host)
    if identity is not None and len(device):
        assert [f.data_ptr() for f in device.stacked_capacity_fields()] == identity
    if state == "fresh_large" and len(tuples):
        assert len(device) == len(tuples) and device.position == len(tuples)


@pytest.mark.parametrize("layout,kinematics", LAYOUTS)
def test_a_call_that_stores_nothing_leaves_the_memory_alone(layout, kinematics, dev):
    """Every episode timed out (N = 0), and a chunk of one-step episodes (stored outcomes, no transition): contents, len and position
    stay; lengths / outcomes read back from `info` when the caller has none give the same result as the explorer's arrays."""
    H = 3
    host, device = ReplayMemory(16), DeviceReplayMemory(16)
    for i in range(21):
        item = _filler(i, H, layout, dev)
        host.push(item), device.push(item)
    for run in (rp.synthetic_run(T, 5, H, outcomes=(4,)), rp.synthetic_run(1, 5, H, outcomes=(3, 2))):
        run["device"] = tuple(torch.as_tensor(run[k]).to(dev) for k in ("robot", "humans", "rewards", "info"))
        assert _push_device(device, run, layout, kinematics, True) == 0
        assert _push_device(device, run, layout, kinematics, True, with_host_arrays=False) == 0
        rp.assert_same_memory(device, host)
    run = _run(70, H, dev)
    for item in _host_tuples(70, H, layout, kinematics, True, dev):
        host.push(item)
    assert _push_device(device, run, layout, kinematics, True, with_host_arrays=False) > 16
    rp.assert_same_memory(device, host)
    with pytest.raises(ValueError):                      # the memory's shapes are fixed: another crowd size is refused, nothing moves
        _push_device(device, _run(5, 1, dev), layout, kinematics, True)
    rp.assert_same_memory(device, host)


# -- VectorExplorer end to end -------------------------------------------------------------------------------------------------------
def _explorers(which, dev, max_batch):
    from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig
    from tests.helpers import make_mprl_policy, make_gcn_policy
    from tests.test_vector_explorer import GoalSeeker
    pol = make_mprl_policy("trained", 1, device=dev) if which == "mprl" else make_gcn_policy(device=dev)
    out = []
    for mem in (ReplayMemory(100000), DeviceReplayMemory(100000)):
        out.append(VectorExplorer(BatchedCrowdSim(dev, SimConfig(human_num=2)), GoalSeeker(pol), memory=mem, gamma=0.9,
                                  target_policy=pol, max_batch=max_batch))
    return out


@pytest.mark.parametrize("max_batch", [4096, 8], ids=["one_chunk", "three_chunks"])
@pytest.mark.parametrize("which", ["mprl", "gcn"])
def test_explorer_fills_both_memories_alike(which, max_batch, dev):
    """The scenario of test_experience_tuples (k = 20, H = 2, a goal-seeking policy, both target policies, imitation learning and RL)
    with a DeviceReplayMemory beside a second explorer with a ReplayMemory on the same cases: equal memories, statistics and last_run;
    with max_batch = 8 the fill spans three push_episodes calls."""
    host_ex, device_ex = _explorers(which, dev, max_batch)
    total = 0
    for il in (True, False):
        want = host_ex.run_k_episodes(20, "test", update_memory=True, imitation_learning=il)
        got = device_ex.run_k_episodes(20, "test", update_memory=True, imitation_learning=il)
        assert got == want and device_ex.last_run == host_ex.last_run
        run = device_ex.last_run
        stored = [i for i in range(20) if run["outcome"][i] in (2, 3)]
        assert len(stored) >= 5 and len(set(run["outcome"])) >= 2
        rp.assert_same_memory(device_ex.memory, host_ex.memory)
        total += sum(run["length"][i] - 1 for i in stored)
        assert len(device_ex.memory) == total                     # the second call continues with the next 20 cases
    item = device_ex.memory[0]
    assert [tuple(x.shape) for x in item] == ([(1, 9), (2, 5), (1,), (1,), (1, 9), (2, 5)] if which == "mprl" else
                                              [(2, 13), (1,), (1,), (2, 13)])
    no_gamma = VectorExplorer(device_ex.sim, device_ex.policy, memory=DeviceReplayMemory(10), gamma=None, target_policy=device_ex.target_policy)
    with pytest.raises(ValueError):
        no_gamma.run_k_episodes(2, "test", update_memory=True)


def test_reference_explorer_fixture_with_a_device_memory(dev):
    """tests/golden/explorer.npz (the REFERENCE Explorer.run_k_episodes driving the reference CrowdSim and ModelPredictiveRL): the
    scenario and the bounds of test_against_the_reference_explorer_fixture with a DeviceReplayMemory -- tuple counts and tuples."""
    from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig
    from tests import golden_io as gio
    from tests.helpers import make_mprl_policy
    fx = gio.load("explorer")
    pol = make_mprl_policy("goal", 1, device=dev)
    pol.set_epsilon(0.0)
    cfg = SimConfig(circle_radius=float(fx["ex.circle_radius"]), time_limit=float(fx["ex.time_limit"]))
    mem = DeviceReplayMemory(100000)
    ex = VectorExplorer(BatchedCrowdSim(dev, cfg), pol, memory=mem, gamma=0.9, target_policy=pol)
    for line in fx["explorer_cases"]:
        tag, phase, k, upd = str(line).split("|")
        k, upd, key = int(k), bool(int(upd)), "ex.%s." % tag
        n_before = len(mem)
        stats = ex.run_k_episodes(k, phase, update_memory=upd, episode=3)
        run = ex.last_run
        assert run["outcome"] == [int(o) for o in fx[key + "outcome"]]
        want = fx[key + "stats"]
        assert stats[0] == want[0] and stats[1] == want[1]
        assert abs(stats[2] - want[2]) < 1e-9 and abs(stats[3] - want[3]) < 1e-6 and abs(stats[4] - want[4]) < 1e-6, (stats, want)
        if upd:
            n = int(fx[key + "n_tuples"])
            assert len(mem) - n_before == n
            robot, humans, value, reward, nrobot, nhumans = (f[n_before:n_before + n].cpu().numpy() for f in mem.as_tensors())
            assert np.allclose(robot[:, 0], fx[key + "mem_robot"][:n].reshape(n, 9), rtol=0, atol=1e-6)
            assert np.allclose(humans, fx[key + "mem_humans"][:n], rtol=0, atol=1e-6)
            assert np.allclose(nrobot[:, 0], fx[key + "mem_next_robot"][:n].reshape(n, 9), rtol=0, atol=1e-6)
            assert np.allclose(nhumans, fx[key + "mem_next_humans"][:n], rtol=0, atol=1e-6)
            assert np.abs(value[:, 0] - fx[key + "mem_value"][:n, 0]).max() < 1e-6
            assert np.abs(reward[:, 0] - fx[key + "mem_reward"][:n, 0]).max() < 1e-6
            for j in (0, n - 1):                          # and item by item, as that test reads them
                assert np.allclose(mem[n_before + j][0].cpu().numpy(), fx[key + "mem_robot"][j], rtol=0, atol=1e-6)
                assert abs(float(mem[n_before + j][2]) - float(fx[key + "mem_value"][j, 0])) < 1e-6


# -- the trainers --------------------------------------------------------------------------------------------------------------------
def _filled_pair(layout, kinematics, dev, H=3):
    run = _run(70, H, dev)
    host, device = ReplayMemory(4096), DeviceReplayMemory(4096)
    for item in _host_tuples(70, H, layout, kinematics, False, dev):
        host.push(item)
    _push_device(device, run, layout, kinematics, False)
    rp.assert_same_memory(device, host)
    return host, device


def test_mprl_trainer_steps_alike_over_both_memories(dev):
    """One MPRLTrainer.optimize_batch over a DeviceReplayMemory filled by push_episodes and over the equal ReplayMemory, same seed:
    both gather from equal stacked fields, so losses and updated parameters are equal."""
    from tests.helpers import make_mprl_policy
    H, results = 3, []
    for mem in _filled_pair("mprl", "holonomic", dev, H):
        pol = make_mprl_policy("trained", 1, device=dev)
        t = rga.MPRLTrainer(pol.value_estimator, pol.state_predictor, mem, dev, pol, _Writer(), 32, "Adam", H,
                            reduce_sp_update_frequency=False, freeze_state_predictor=False, detach_state_predictor=True,
                            share_graph_model=False)
        t.set_learning_rate(1e-3)
        t.update_target_model(pol.value_estimator)
        torch.manual_seed(4)
        losses = t.optimize_batch(2, 0)
        params = torch.cat([p.detach().flatten() for p in list(pol.value_estimator.parameters()) + list(pol.state_predictor.parameters())])
        results.append((losses, params.cpu()))
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert bool(torch.isfinite(results[1][1]).all()) and torch.equal(results[0][1], results[1][1])


def test_vnrl_trainer_steps_alike_over_both_memories(dev):
    """The same for path G: one VNRLTrainer.optimize_batch (DataLoader + pad_batch over the memory's items) both ways."""
    from tests.helpers import make_gcn_policy
    results = []
    for mem in _filled_pair("gcn", "holonomic", dev):
        pol = make_gcn_policy(device=dev)
        t = rga.VNRLTrainer(pol.model, mem, dev, pol, 32, "Adam", _Writer())
        t.set_learning_rate(1e-3)
        t.update_target_model(pol.model)
        torch.manual_seed(4)
        loss = t.optimize_batch(2)
        results.append((loss, torch.cat([p.detach().flatten() for p in pol.model.parameters()]).cpu()))
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert bool(torch.isfinite(results[1][1]).all()) and torch.equal(results[0][1], results[1][1])
