"""The replay memory filled with SARL / OM-SARL rows on the device (csrc/rgl_replay.hip: rgl_replay_push_sarl_f32 through
DeviceReplayMemory.push_sarl_episodes) against the host path -- `VectorExplorer.update_memory`, which makes the rows of an episode
with one `rotate` and one `occupancy_maps` and pushes tuple by tuple: equal len and position and torch.equal rows for every item and
field (tests/replay_push.py: assert_same_memory).  Besides that the stored rows against float64 (tests/sarl_cpu.py), which shares no
kernel with either, the stores against guards around every field, and the explorer's routing.

Crowd sizes: 1 (no maps only), 2, 5; 32 and 33 on both sides of the kernel's one-wave form and of its pair-record group (above 32
humans a state's humans are walked in groups of 1024 // H, by four waves); 65 (lanes stride over the other humans) and 127 (the
largest).  T = 6, B = 8 (3 from H = 65 on)."""
import ctypes as C

import numpy as np
import pytest
import torch

from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd.vector_explorer import DeviceReplayMemory, ReplayMemory, VectorExplorer, replay_slot_runs
from tests import replay_push as rp
from tests import sarl_cpu as cpu
from tests import sarl_replay_push as srp

pytestmark = pytest.mark.gpu

CROWDS = [1, 2, 5, 32, 33, 65, 127]
KINEMATICS = ["holonomic", "unicycle"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_RUNS, _TUPLES = {}, {}


def _run(H, dev):
    if H not in _RUNS:
        run = srp.crowded_run(H)
        run["device"] = tuple(torch.as_tensor(run[k]).to(dev) for k in ("robot", "humans", "rewards", "info"))
        _RUNS[H] = run
    return _RUNS[H]


def _host_tuples(H, kinematics, channels, il, dev):
    """The host path's tuples of a case, computed once and never modified."""
    key = (H, kinematics, channels, il)
    if key not in _TUPLES:
        _TUPLES[key] = srp.host_tuples(_run(H, dev), kinematics, srp.om_of(channels), il, dev)
    return _TUPLES[key]


def _push(memory, run, kinematics, channels, il, with_host_arrays=True):
    robot, humans, rewards, info = run["device"]
    extra = dict(lengths=run["lengths"], outcomes=run["outcome"]) if with_host_arrays else {}
    return memory.push_sarl_episodes(robot, humans, rewards, info, kinematics, rp.STEP_DISCOUNT, il, om=srp.om_of(channels), **extra)


def _filler(i, H, D, dev):
    shapes = ((H, D), (1,), (1,), (H, D))
    return tuple(torch.full(shape, -100.0 - i - 0.01 * f, dtype=torch.float32, device=dev) for f, shape in enumerate(shapes))


def _check_inputs(run, H, channels):
    """Teeth of the inputs, on the CPU: of the map rows a case stores at least a quarter is non-zero and, with the velocity channels
    and a third human to share a cell with, some cell of some grid holds two humans or more."""
    maps, most = srp.reference_maps(run, H, channels)
    rows = np.concatenate(list(maps.values()))
    assert rows.shape == (len(srp.stored_states(run)) * H, 16 * channels)
    assert (rows != 0).any(axis=1).mean() >= 0.25
    if channels > 1 and H > 2:
        assert most >= 2


@pytest.mark.parametrize("channels", [0, 1, 2, 3], ids=["no_maps", "om1", "om2", "om3"])
@pytest.mark.parametrize("H", CROWDS)
def test_push_sarl_episodes_equals_the_host_path(H, channels, dev):
    """Both kinematics, imitation learning and RL, into a fresh memory: every field of every item is what the host path stores.  The
    chunk holds stored goals and collisions, time-outs, episodes of length 1, info == 5 tails of every length and NaN in every row
    past an episode's end."""
    if H == 1 and channels:
        run = _run(1, dev)
        m = DeviceReplayMemory(64)
        with pytest.raises(ValueError):                  # upstream's np.concatenate failure, before the library is asked
            _push(m, run, "holonomic", channels, True)
        assert len(m) == 0 and m.position == 0 and m.as_tensors() is None
        return
    run = _run(H, dev)
    if channels:
        _check_inputs(run, H, channels)
    n = sum(L - 1 for L, o in zip(run["lengths"], run["outcome"]) if o in (2, 3))
    D = 13 + 16 * channels
    for kinematics in KINEMATICS:
        for il in (True, False):
            tuples = _host_tuples(H, kinematics, channels, il, dev)
            assert len(tuples) == n > 0 and tuple(tuples[0][0].shape) == (H, D)
            host, device = ReplayMemory(64), DeviceReplayMemory(64)
            for item in tuples:
                host.push(item)
            assert _push(device, run, kinematics, channels, il, with_host_arrays=(kinematics == "holonomic")) == n
            rp.assert_same_memory(device, host)
            assert [tuple(x.shape) for x in device[0]] == [(H, D), (1,), (1,), (H, D)]
    assert not torch.equal(_host_tuples(H, "holonomic", channels, True, dev)[0][0], _host_tuples(H, "unicycle", channels, True, dev)[0][0])


# capacity, pushes before, clear() after them, pushes after the clear, calls
STATES = {
    "capacity_7": (7, 0, False, 0, 1),                   # 17 tuples: the first ten are overwritten within the call
    "full_position_7": (50, 57, False, 0, 1),
    "cleared_position_ahead": (64, 41, True, 0, 1),      # position 41, nothing stored: appended from item 0
    "cleared_then_three": (64, 62, True, 3, 1),          # three pushes wrap: position 1 behind length 2 -- overwrite, then append
    "two_calls": (30, 5, False, 0, 2),                   # the second call wraps
}


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("H,channels,kinematics,il", [(5, 3, "holonomic", True), (2, 0, "unicycle", False), (33, 2, "unicycle", True)])
def test_ring_states(H, channels, kinematics, il, state, dev):
    capacity, before, clear, after, calls = STATES[state]
    run, D = _run(H, dev), 13 + 16 * channels
    tuples = _host_tuples(H, kinematics, channels, il, dev)
    host, device = ReplayMemory(capacity), DeviceReplayMemory(capacity)
    for i in range(before + after):
        if clear and i == before:
            host.clear(), device.clear()
        item = _filler(i, H, D, dev)
        host.push(item), device.push(item)
    if clear and after == 0:
        host.clear(), device.clear()
    identity = None if device.stacked_capacity_fields() is None else [f.data_ptr() for f in device.stacked_capacity_fields()]
    for _ in range(calls):
        for item in tuples:
            host.push(item)
        assert _push(device, run, kinematics, channels, il) == len(tuples)
        assert device.position == host.position and len(device) == len(host)
    rp.assert_same_memory(device, host)
    if identity is not None:
        assert [f.data_ptr() for f in device.stacked_capacity_fields()] == identity


def test_a_call_that_stores_nothing_and_a_memory_of_other_rows(dev):
    H, D = 5, 61
    host, device = ReplayMemory(16), DeviceReplayMemory(16)
    for i in range(21):
        item = _filler(i, H, D, dev)
        host.push(item), device.push(item)
    for run in (rp.synthetic_run(srp.T, 5, H, outcomes=(4,)), rp.synthetic_run(1, 5, H, outcomes=(3, 2))):
        run["device"] = tuple(torch.as_tensor(run[k]).to(dev) for k in ("robot", "humans", "rewards", "info"))
        assert _push(device, run, "holonomic", 3, True) == 0
        assert _push(device, run, "holonomic", 3, True, with_host_arrays=False) == 0
        rp.assert_same_memory(device, host)
    for channels, crowd in ((2, 5), (0, 5), (3, 2)):     # the memory's shapes are fixed: other rows are refused, nothing moves
        with pytest.raises(ValueError):
            _push(device, _run(crowd, dev), "holonomic", channels, True)
    robot, humans, rewards, info = _run(H, dev)["device"]
    for bad in ((robot[:, :, :8], humans, rewards, info), (robot, humans[..., :4], rewards, info), (robot, humans, rewards[:5], info),
                (robot, humans, rewards, info[:, :7]), (robot[0], humans[0], rewards, info)):
        with pytest.raises(ValueError):
            device.push_sarl_episodes(*bad, "holonomic", rp.STEP_DISCOUNT, True, om=srp.om_of(3))
    with pytest.raises(TypeError):
        device.push_sarl_episodes(robot, humans, rewards, info.long(), "holonomic", rp.STEP_DISCOUNT, True, om=srp.om_of(3))
    rp.assert_same_memory(device, host)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)))


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("H", CROWDS[1:])
def test_stored_rows_against_float64(H, channels, dev):
    """Independent of the device's own row kernels.  The map columns: within one float32 ulp of sarl_cpu.occupancy_maps (float64; 0
    and 1 exactly).  The 13 relation columns: sarl_cpu's operator chain in float32 on the CPU, within the bound
    tests/test_sarl_gpu.py::test_fixture_maps_and_transform_rows applies to `transform` -- 8 ulp of the scene's largest distance."""
    run = _run(H, dev)
    _check_inputs(run, H, channels)
    want_maps, _ = srp.reference_maps(run, H, channels)
    tuples = rp.replay_push(run["info"], run["rewards"], rp.STEP_DISCOUNT, True, 0, 0, 64)["tuples"]
    for kinematics in KINEMATICS:
        device = DeviceReplayMemory(64)
        assert _push(device, run, kinematics, channels, True) == len(tuples)
        state, _, _, nxt = (f.cpu().numpy() for f in device.as_tensors())
        for item, (b, t) in enumerate(tuples):
            for got, step in ((state[item], t), (nxt[item], t + 1)):
                want = want_maps[(step, b)]
                exact = (want == 0) | (want == 1)
                assert np.array_equal(got[:, 13:][exact], want[exact])
                assert (np.abs(got[:, 13:].astype(np.float64) - want) <= ulp32(want)).all()
                rows = cpu.transform(run["robot"][step, b], run["humans"][step, b], kinematics, None).numpy()
                d = max(float(rows[:, 11].max()), float(rows[0, 0]))
                assert (np.abs(got[:, :13] - rows) <= 8 * np.spacing(np.float32(d))).all()


def _guarded(n_floats, guard, sentinel, dev):
    whole = torch.full((n_floats + 2 * guard,), sentinel, dtype=torch.float32, device=dev)
    return whole, whole[guard:guard + n_floats]


@pytest.mark.parametrize("H,channels", [(5, 3), (33, 2), (2, 0), (127, 1)])
def test_stores_stay_inside_the_named_slots(H, channels, dev):
    """The C ABI with fields that are views into larger buffers of a sentinel: after the call every guard element before and behind a
    field is intact, so is every slot no run names, the named slots hold the host path's tuples -- and the same with the workspace
    filled with NaN patterns beforehand."""
    run, D = _run(H, dev), 13 + 16 * channels
    kinematics, il, capacity, position, length = "unicycle", True, 24, 21, 22
    tuples = _host_tuples(H, kinematics, channels, il, dev)
    runs, _, _ = replay_slot_runs(position, length, capacity, len(tuples))
    contents = rp.contents_of_runs(runs, capacity)
    assert len(runs) == 2 and contents.count(-1) == capacity - len(tuples) > 0      # the ring wraps; the slots between are not named
    lib = nat.lib()
    robot, humans, rewards, info = run["device"]
    sentinel, guard = -777.25, 4096
    need = int(lib.rgl_replay_push_workspace_bytes(srp.T, run["B"]))
    results = []
    for fill in (0, 255):
        workspace = torch.full((need + 512,), fill, dtype=torch.uint8, device=dev)
        buffers = [_guarded(capacity * n, guard, sentinel, dev) for n in (H * D, 1, 1, H * D)]
        job = nat.RglReplayPushJob()
        job.robot, job.humans, job.rewards, job.info = robot.data_ptr(), humans.data_ptr(), rewards.data_ptr(), info.data_ptr()
        job.T, job.B, job.H, job.layout, job.kinematics = srp.T, run["B"], H, 99, nat.KINEMATICS[kinematics]
        job.imitation_learning, job.step_discount, job.capacity = int(il), rp.STEP_DISCOUNT, capacity
        for f, (_, view) in enumerate(buffers):
            job.fields[f] = view.data_ptr()
        job.n_runs = len(runs)
        for r, (first, slot, count) in enumerate(runs):
            job.runs[r].first, job.runs[r].slot, job.runs[r].count = first, slot, count
        job.workspace, job.workspace_bytes = workspace.data_ptr(), need
        rows = nat.RglReplaySarlRows()
        if channels:
            rows.cell_num, rows.cell_size, rows.channels = srp.CELL_NUM, srp.CELL_SIZE, channels
        with torch.cuda.device(dev):
            job.stream = None
            rc = lib.rgl_replay_push_sarl_f32(C.byref(job), C.byref(rows))
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((workspace[need:] == fill).all())
        for f, (whole, view) in enumerate(buffers):
            assert bool((whole[:guard] == sentinel).all()) and bool((whole[-guard:] == sentinel).all()), f
            per_slot = view.reshape(capacity, -1)
            for slot, j in enumerate(contents):
                if j < 0:
                    assert bool((per_slot[slot] == sentinel).all()), (f, slot)
                else:
                    assert torch.equal(per_slot[slot], tuples[j][f].reshape(-1)), (f, slot, j)
        results.append([view.clone() for _, view in buffers])
    assert all(torch.equal(a, b) for a, b in zip(*results))


# -- VectorExplorer ------------------------------------------------------------------------------------------------------------------
class _Writer(object):
    def add_scalar(self, *args):
        pass


def _policy(dev, input_dim, enable=True):
    from tests.test_sarl_gpu import make_policy
    pol = make_policy(dev, "holonomic", input_dim, True, "plain")
    if enable:
        pol.enable_training()
    return pol


def _explore(dev, memory, input_dim, enable=True):
    """The scenario of tests/test_sarl_train_gpu.py: four ORCA-driven episodes of twelve steps at the most in a six-metre square."""
    from relationalgraphlearning_amd.orca import OrcaPolicy
    from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig
    pol = _policy(dev, input_dim, enable)
    cfg = SimConfig(time_limit=4, circle_radius=1.0, scenario="square_crossing", square_width=6)
    ex = VectorExplorer(BatchedCrowdSim(dev, cfg, human_policy="orca"), OrcaPolicy(safety_space=0.15), memory=memory, gamma=0.9,
                        target_policy=pol)
    stats = ex.run_k_episodes(4, "train", update_memory=True, imitation_learning=True)
    return pol, ex, stats


@pytest.mark.parametrize("input_dim", [13, 61], ids=["sarl", "om_sarl"])
def test_explorer_routes_a_device_memory_to_the_push(input_dim, dev, monkeypatch):
    calls = []
    original = VectorExplorer.update_memory

    def counting(self, *args, **kwargs):
        calls.append(type(self.memory).__name__)
        return original(self, *args, **kwargs)
    monkeypatch.setattr(VectorExplorer, "update_memory", counting)
    host, device = ReplayMemory(1000), DeviceReplayMemory(1000)
    _, host_ex, want = _explore(dev, host, input_dim)
    assert calls and set(calls) == {"ReplayMemory"}                                 # the host route, as before
    del calls[:]
    _, device_ex, got = _explore(dev, device, input_dim)
    assert calls == []                                                              # one push_sarl_episodes call instead
    assert got == want and device_ex.last_run == host_ex.last_run
    assert len(host) > 0
    rp.assert_same_memory(device, host)
    for i in range(len(host)):
        assert all(torch.equal(a, b) for a, b in zip(host[i], device[i]))
    assert [tuple(x.shape) for x in device[0]] == [(5, input_dim), (1,), (1,), (5, input_dim)]
    if input_dim == 61:
        assert bool((device.as_tensors()[0][:, :, 13:] != 0).any())


def test_explorer_still_refuses_before_enable_training(dev):
    memory = DeviceReplayMemory(1000)
    with pytest.raises(NotImplementedError):
        _explore(dev, memory, 61, enable=False)
    assert len(memory) == 0 and memory.as_tensors() is None


def test_trainer_learns_from_a_device_filled_memory(dev):
    from relationalgraphlearning_amd import VNRLTrainer
    memory = DeviceReplayMemory(1000)
    pol, _, _ = _explore(dev, memory, 61)
    t = VNRLTrainer(pol.model, memory, dev, pol, 16, "Adam", _Writer())
    t.set_learning_rate(1e-3)
    t.update_target_model(pol.model)

    def imitation_loss():
        with torch.no_grad():
            rows, values = memory.as_tensors()[0], memory.as_tensors()[1]
            return float(torch.nn.functional.mse_loss(pol.model(rows), values))
    before = imitation_loss()
    t.optimize_epoch(2)
    after = imitation_loss()
    assert after < before, (before, after)
    assert np.isfinite(t.optimize_batch(2, 0))
