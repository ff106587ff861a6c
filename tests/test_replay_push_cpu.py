"""Host side of the device replay memory (-m "not gpu"): the slot map of a whole call against ReplayMemory.push itself, DeviceReplayMemory's
ring on CPU tensors against ReplayMemory, the numpy replay's values against VectorExplorer.update_memory, and the ABI of the push."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import relationalgraphlearning_amd as rga
from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd.vector_explorer import DeviceReplayMemory, ReplayMemory, replay_slot_runs
from tests import replay_push as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_runs_equal_replay_memory_push_exhaustively():
    """Every capacity 1..7, every (position, length) a ReplayMemory reaches by push / clear sequences -- length 0 with the position
    ahead included -- and n = 0..20 pushes: the trimmed runs leave push j in item i exactly where ReplayMemory.push leaves it, position
    and length move alike, no slot is named twice and there are never more runs than the job struct holds."""
    checked, most = 0, 0
    for capacity in range(1, 8):
        states = rp.reachable_states(capacity)
        assert all((p, 0) in states for p in range(capacity))                     # after clear(): any position, nothing stored
        assert all(0 <= p < capacity and 0 <= n <= capacity for p, n in states)
        for position, length in states:
            for n in range(21):
                runs, position1, length1 = replay_slot_runs(position, length, capacity, n)
                contents, want_position, want_length = rp.simulate_pushes(position, length, capacity, n)
                assert (position1, length1) == (want_position, want_length), (capacity, position, length, n)
                assert rp.contents_of_runs(runs, length1) == contents, (capacity, position, length, n, runs)     # disjoint, too
                assert all(count > 0 and 0 <= first and first + count <= n and 0 <= slot and slot + count <= capacity
                           for first, slot, count in runs), runs
                assert len(runs) <= nat.REPLAY_MAX_RUNS, (capacity, position, length, n, runs)
                most = max(most, len(runs))
                checked += 1
    assert most == nat.REPLAY_MAX_RUNS and checked > 2000                          # the bound is reached: the array is not oversized
    with pytest.raises(ValueError):
        replay_slot_runs(4, 0, 4, 1)
    with pytest.raises(ValueError):
        replay_slot_runs(0, 5, 4, 1)


def _item(i, H=2):
    g = torch.Generator().manual_seed(100 + i)
    return (torch.rand(1, 9, generator=g), torch.rand(H, 5, generator=g), torch.rand(1, generator=g), torch.rand(1, generator=g),
            torch.rand(1, 9, generator=g), torch.rand(H, 5, generator=g))


def _assert_same(dm, rm):
    assert len(dm) == len(rm) and dm.position == rm.position and dm.is_full() == rm.is_full()
    for i in range(len(rm)):
        assert all(torch.equal(a, b) for a, b in zip(dm[i], rm[i])), i
    want, got = rm.as_tensors(), dm.as_tensors()
    if len(rm) == 0:
        assert want is None and got is None and dm.stacked_capacity_fields() is None
        return
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    whole = dm.stacked_capacity_fields()
    assert all(w.shape[0] == dm.capacity and g.data_ptr() == w.data_ptr() for w, g in zip(whole, got))


def test_device_replay_memory_ring_on_cpu_tensors():
    """Capacity 4, eleven pushes with a clear() in the middle: after every operation DeviceReplayMemory holds in item i what
    ReplayMemory holds there (items, as_tensors, len, position, is_full); the stacked tensors are the same objects from the first
    push on, through wrap-around and clear(); other shapes, dtypes or non-tensor items are refused."""
    dm, rm = DeviceReplayMemory(4), ReplayMemory(4)
    assert len(dm) == 0 and dm.as_tensors() is None and dm.stacked_capacity_fields() is None and not dm.is_full()
    identity = None
    for i in range(11):
        if i == 6:                                      # full, position 2: upstream keeps the position, items are appended again
            dm.clear(), rm.clear()
            assert dm.position == rm.position == 2
            _assert_same(dm, rm)
            with pytest.raises(IndexError):
                dm[0]
        dm.push(_item(i)), rm.push(_item(i))
        _assert_same(dm, rm)
        fields = dm.stacked_capacity_fields()
        if identity is None:
            identity = [(id(f), f.data_ptr(), tuple(f.shape)) for f in fields]
        assert [(id(f), f.data_ptr(), tuple(f.shape)) for f in fields] == identity          # never re-allocated, never resized
    assert [tuple(f.shape) for f in dm.stacked_capacity_fields()] == [(4, 1, 9), (4, 2, 5), (4, 1), (4, 1), (4, 1, 9), (4, 2, 5)]
    assert len(dm) == 3 and not dm.is_full()            # two of the five pushes after clear() overwrote items 0 and 1
    with pytest.raises(IndexError):
        dm[3]
    dm.push(_item(11)), rm.push(_item(11))
    _assert_same(dm, rm)
    assert dm.is_full() and len(dm) == 4
    with pytest.raises(IndexError):
        dm[4]
    assert all(torch.equal(a, b) for a, b in zip(dm[-1], rm[-1]))
    # the loaders the trainers build: default collate and pad_batch's sort by crowd size
    batch = next(iter(torch.utils.data.DataLoader(dm, batch_size=4)))
    assert [tuple(x.shape) for x in batch] == [(4, 1, 9), (4, 2, 5), (4, 1), (4, 1), (4, 1, 9), (4, 2, 5)]
    assert all(torch.equal(a, b) for a, b in zip(batch, dm.as_tensors()))
    before = [f.clone() for f in dm.as_tensors()]
    for bad in (_item(0, H=3), tuple(x.double() for x in _item(0)), _item(0)[:4], 7, (1, 2)):
        with pytest.raises(ValueError):
            dm.push(bad)
    assert dm.position == rm.position and all(torch.equal(a, b) for a, b in zip(dm.as_tensors(), before))
    with pytest.raises(ValueError):
        DeviceReplayMemory(0)
    g = DeviceReplayMemory(3)                           # path G's four fields
    g.push((torch.ones(2, 13), torch.zeros(1), torch.ones(1), torch.ones(2, 13)))
    from relationalgraphlearning_amd.trainer import pad_batch
    (states, lengths), values, rewards, _ = next(iter(torch.utils.data.DataLoader(g, batch_size=1, collate_fn=pad_batch)))
    assert tuple(states.shape) == (1, 2, 13) and list(lengths) == [2]
    assert rga.DeviceReplayMemory is DeviceReplayMemory and rga.replay_slot_runs is replay_slot_runs


@pytest.mark.parametrize("imitation_learning", [True, False])
def test_numpy_replay_equals_update_memory(imitation_learning):
    """The helper's lengths, stored flags, offsets, values and slots against the code as it stands: a plain ReplayMemory on CPU tensors
    filled by VectorExplorer.update_memory ("mprl" needs no device), from a ring state after clear() with capacity below N."""
    run = rp.synthetic_run(6, 23, 2, seed=3)
    capacity, position = 13, 9
    host = rp.memory_in_state(position, 0, capacity)
    rp.host_fill(host, run, "mprl", "holonomic", imitation_learning, torch.device("cpu"))
    got = rp.replay_push(run["info"], run["rewards"], rp.STEP_DISCOUNT, imitation_learning, position, 0, capacity)
    assert np.array_equal(got["lengths"], run["lengths"]) and np.array_equal(got["outcome"], run["outcome"])
    assert got["offsets"][-1] == len(got["tuples"]) > capacity
    assert (got["position"], got["length"]) == (host.position, len(host))
    assert not np.isnan(got["values"][0, got["stored"] & (run["lengths"] > 1)]).any()
    for i, j in enumerate(got["contents"]):
        b, t = got["tuples"][j]
        robot, humans, value, reward, next_robot, next_humans = host[i]
        assert got["offsets"][b] + t == j
        assert value.dtype == torch.float32 and value.numpy()[0] == got["values"][t, b]                  # the same float32
        assert imitation_learning or value.numpy()[0] == 0
        assert reward.numpy()[0] == run["rewards"][t, b]
        assert np.array_equal(robot.numpy()[0], run["robot"][t, b]) and np.array_equal(humans.numpy(), run["humans"][t, b])
        assert np.array_equal(next_robot.numpy()[0], run["robot"][t + 1, b]) and np.array_equal(next_humans.numpy(), run["humans"][t + 1, b])
    # the values tell a float32 recursion from the float64 one: some tuple of this run rounds differently
    if imitation_learning:
        other = 0
        for b in np.nonzero(got["stored"])[0]:
            togo = np.float32(0)
            for t in range(int(run["lengths"][b]) - 1, -1, -1):
                togo = run["rewards"][t, b] + np.float32(rp.STEP_DISCOUNT) * togo
                other += int(t < run["lengths"][b] - 1 and togo != got["values"][t, b])
        assert other > 0


def test_replay_push_abi():
    """rgl_replay_push_workspace_bytes / rgl_replay_push_f32: declared in the header and in SIGNATURES within ABI 8, the job struct's
    size as the header implies it, and the argument checks on the host, before any launch (no pointer below is read)."""
    hdr = open(os.path.join(ROOT, "include", "rgl_hip.h")).read()
    for name in ("rgl_replay_push_workspace_bytes", "rgl_replay_push_f32"):
        assert re.search(r"^\s*(?:int|size_t)\s+%s\s*\(" % name, hdr, flags=re.M) and name in nat.SIGNATURES
    assert int(re.search(r"#define RGL_ABI_VERSION (\d+)", hdr).group(1)) == nat.ABI_VERSION == 8
    assert int(re.search(r"#define RGL_REPLAY_MAX_RUNS (\d+)", hdr).group(1)) == nat.REPLAY_MAX_RUNS
    assert int(re.search(r"#define RGL_REPLAY_MAX_FIELDS (\d+)", hdr).group(1)) == nat.REPLAY_MAX_FIELDS == 6
    assert re.search(r"RGL_REPLAY_MPRL = 0, RGL_REPLAY_GCN = 1", hdr) and nat.REPLAY_LAYOUTS == {"mprl": 0, "gcn": 1}
    # LP64: 4 pointers, 6 ints, a double, a long long, 6 pointers, 2 ints, MAX_RUNS runs of 3 long long, pointer + size_t + pointer
    assert ctypes.sizeof(nat.RglReplayRun) == 24
    assert ctypes.sizeof(nat.RglReplayPushJob) == 4 * 8 + 6 * 4 + 8 + 8 + 6 * 8 + 2 * 4 + nat.REPLAY_MAX_RUNS * 24 + 3 * 8
    lib = nat.lib()
    BAD_SHAPE, BAD_MODE, NULL, WORKSPACE = -1, -2, -3, -4
    need = lib.rgl_replay_push_workspace_bytes(6, 300)
    assert need >= 6 * 300 * 4 + 2 * 300 * 4 and need % 256 == 0
    assert lib.rgl_replay_push_workspace_bytes(0, 4) == 0 and lib.rgl_replay_push_workspace_bytes(4, 0) == 0
    assert lib.rgl_replay_push_workspace_bytes(1 << 16, 1 << 16) == 0
    p = 4096                                           # never dereferenced

    def job(**over):
        j = nat.RglReplayPushJob()
        j.robot = j.humans = j.rewards = j.info = p
        j.T, j.B, j.H, j.layout, j.kinematics, j.imitation_learning = 6, 300, 3, 0, 0, 1
        j.step_discount, j.capacity = rp.STEP_DISCOUNT, 16
        for f in range(6):
            j.fields[f] = p
        j.n_runs = 1
        j.runs[0].first, j.runs[0].slot, j.runs[0].count = 0, 0, 16
        j.workspace, j.workspace_bytes = p, need
        for k, v in over.items():
            if k.startswith("run_"):
                setattr(j.runs[0], k[4:], v)
            elif k.startswith("field_"):
                j.fields[int(k[6:])] = v
            else:
                setattr(j, k, v)
        return lib.rgl_replay_push_f32(ctypes.byref(j))

    assert lib.rgl_replay_push_f32(None) == NULL
    for name in ("robot", "humans", "rewards", "info", "workspace", "field_0", "field_5"):
        assert job(**{name: None}) == NULL, name
    assert job(layout=1, field_3=None) == NULL and job(layout=1, field_4=None, field_5=None, workspace_bytes=0) == WORKSPACE
    for over in (dict(T=0), dict(B=0), dict(B=-2), dict(H=0), dict(H=nat.MAX_NODES), dict(capacity=0), dict(T=1 << 16, B=1 << 16)):
        assert job(**over) == BAD_SHAPE, over
    for over in (dict(layout=2), dict(layout=-1), dict(kinematics=2), dict(kinematics=-1)):
        assert job(**over) == BAD_MODE, over
    # a slot map that leaves the memory is refused: whatever `info` holds, the scatter cannot store outside the fields
    for over in (dict(n_runs=-1), dict(n_runs=nat.REPLAY_MAX_RUNS + 1), dict(run_count=17), dict(run_slot=1), dict(run_slot=-1),
                 dict(run_first=-1), dict(run_count=-1)):
        assert job(**over) == BAD_SHAPE, over
    assert job(workspace_bytes=need - 1) == WORKSPACE and job(workspace_bytes=0) == WORKSPACE
    assert job(n_runs=0) == 0                          # nothing survives: no launch, so no device is needed either
    assert job(H=nat.MAX_NODES - 1, n_runs=0) == 0


def test_push_episodes_refuses_what_it_cannot_store():
    """push_episodes checks layout, kinematics and tensors before the library is asked; CPU tensors are refused like everywhere else
    (no CPU path), and nothing is allocated or moved by a refused call."""
    run = rp.synthetic_run(6, 5, 2)
    t = {k: torch.as_tensor(run[k]) for k in ("robot", "humans", "rewards", "info")}
    m = DeviceReplayMemory(8)
    with pytest.raises(nat.NativeLibraryError):
        m.push_episodes(t["robot"], t["humans"], t["rewards"], t["info"], "mprl", "holonomic", 0.9, True)
    with pytest.raises(ValueError):
        m.push_episodes(t["robot"], t["humans"], t["rewards"], t["info"], "sarl", "holonomic", 0.9, True)
    with pytest.raises(ValueError):
        m.push_episodes(t["robot"], t["humans"], t["rewards"], t["info"], "gcn", "bicycle", 0.9, True)
    assert len(m) == 0 and m.position == 0 and m.as_tensors() is None
