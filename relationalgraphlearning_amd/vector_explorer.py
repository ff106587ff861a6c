"""Explorer / replay-memory plumbing for many environments in lock-step.

`VectorExplorer.run_k_episodes` keeps the contract of crowd_nav/utils/explorer.py:21-111 -- same arguments, same five
statistics, same log lines (crowd_nav/utils/plot.py:50-66 parses them) and the same experience tuples pushed into the
replay memory (explorer.py:113-140) -- but runs the k episodes side by side on the device: one `policy.predict_batch`
and one `BatchedCrowdSim.step` per time step for all live environments.  `ReplayMemory` is the reference's ring buffer
(crowd_nav/utils/memory.py) so `MPRLTrainer` / `VNRLTrainer` consume it unchanged through a DataLoader.

Differences that follow from vectorisation (documented, not hidden): episodes of one call are the NEXT k seeded cases
of the phase (the reference draws them one after another from the same counter, so the set is identical; the order
inside the replay memory is episode-major here as well); epsilon-greedy exploration draws its random numbers per
time step for all environments at once, so the random stream differs from k sequential episodes.

`DeviceReplayMemory` keeps the experience as the stacked (capacity, ...) tensors alone and is filled by ONE library call per chunk
of episodes (`push_episodes`, rgl_replay_push_f32): the explorer then records a chunk's states, rewards and info codes into
preallocated (T, B, ...) tensors instead of per-step clones, and the per-tuple loop of `update_memory` does not run.  It stores
the same bits in the same slots as `ReplayMemory` filled by `update_memory` (tests/test_replay_push.py).  For a SARL / OM-SARL target
after `enable_training()` the call is `push_sarl_episodes` (rgl_replay_push_sarl_f32), which builds `SARL.transform`'s rows -- the
rotated features and the occupancy maps -- for the states that land in the memory (tests/test_sarl_replay_push.py).

A policy with `acts_in_velocity = True` (orca.OrcaPolicy, the imitation-learning expert of train.py:143-154) returns (B,2)
velocities from `predict_batch(robot, humans, done=...)`, given the simulator's float64 state; they go to the simulator as
they are and `last_run["actions"]` holds them as (vx, vy) pairs.  Index-returning policies are unaffected.

`exploration="device"` (default "host", the paragraph above) makes a training episode explore with upstream's own stream: numpy
is seeded per case in CrowdSim.reset (crowd_sim.py:185-191), scene generation consumes doubles, and every `predict` continues
that stream with `np.random.random()` and, when it explores, `np.random.choice(n)` (model_predictive_rl.py:208-210,
multi_human_rl.py:34-36).  Every environment then carries its case's MT19937 state on the device, seeded after `reset` from
`sim.scene_seeds` / `sim.scene_draws` (crowd_explore_seed_u32), and one kernel per step makes the draw for every live
environment, picks the action and writes the action row the simulator steps with (crowd_explore_select_f64, csrc/rgl_explore.hip):
an exploring episode of training case k is a function of k, epsilon and the weights, as upstream's is with ORCA or linear humans.
"host" exploration is NOT upstream's stream and not reproducible from the cases.

Nonstop humans (`SimConfig.nonstop_human`): the simulator regenerates arriving humans from the case's stream (`sim.stream`), which
upstream's `predict` also draws from -- one `np.random.random()` per decision in EVERY phase, plus the words of `choice` when it
explores -- so the two consumers share one stream.  With exploration="device" the select kernel draws from `sim.stream` itself and
runs in every phase (epsilon 0 outside `train`: the draw is made, nothing explores); with exploration="host" a step tells the
simulator to skip the one double an index policy's `predict` would have drawn (`policy_draws=1`; 0 for a velocity policy, whose
`predict` draws nothing), so `val` and `test` runs are upstream's in either mode, and `train` with host exploration stays "not
upstream's stream".  A regeneration that reached `scene_max_attempts` raises UnplacedSceneError at the end of its chunk.
"""
import ctypes as C
import logging

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _native as nat
from .actions import as_array
from .nets import _require_device_tensor, _stream
from .rollout import rotate, occupancy_maps
from .sim import UnplacedSceneError

COLLISION, SUCCESS, TIMEOUT = 2, 3, 4          # BatchedCrowdSim info codes
CASE_SIZE = {"train": np.iinfo(np.uint32).max - 2000, "val": 100, "test": 500}     # crowd_sim.py:60-62 defaults


class ReplayMemory(Dataset):
    """Fixed-capacity ring of experience tuples; the oldest entry is overwritten once full (crowd_nav/utils/memory.py).
    Additive: `as_tensors()` -- the experience as one stacked tensor per tuple field, kept up to date incrementally -- which lets
    the trainers gather a batch with one index_select per field instead of collating 100 python tuples (trainer.py)."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.memory = []
        self.position = 0
        self._mirror = None           # per field: (capacity, *item shape) tensor on the items' device
        self._dirty = []              # positions written since the mirror was last brought up to date
        self._unstackable_at = -1     # len(memory) when the items were last found to differ in shape (no stacked view): the
                                      # check is not repeated -- O(n) host work and capacity-sized allocations -- until the ring
                                      # has been cleared or has wrapped far enough to have dropped the odd items

    def push(self, item):
        if self.position < len(self.memory):
            self.memory[self.position] = item
            self._dirty.append(self.position)
        else:
            self.memory.append(item)                 # (after clear() the write position is ahead of the list: upstream's ring)
            self._dirty.append(len(self.memory) - 1)
        self.position = (self.position + 1) % self.capacity

    def is_full(self):
        return len(self.memory) == self.capacity

    def clear(self):
        self.memory = []          # the write position is kept, as upstream does
        self._mirror, self._dirty, self._unstackable_at = None, [], -1

    def __getitem__(self, index):
        return self.memory[index]

    def __len__(self):
        return len(self.memory)

    def as_tensors(self):
        """[field 0 of every item stacked (n, ...), field 1 ..., ...] in item order -- what DataLoader's default collate would make
        of the whole memory -- or None when the items are not tuples of equally shaped tensors (path G's variable crowds).  Only the
        entries pushed since the last call are copied."""
        n = len(self.memory)
        if n == 0:
            return None
        first = self.memory[0]
        if not (isinstance(first, tuple) and all(torch.is_tensor(x) for x in first)):
            return None
        if self._unstackable_at >= 0:
            # mixed shapes were found with this many items: until the ring is full and has been overwritten once more (the odd
            # items may be gone then) the answer cannot change -- no re-allocation, no walk over the items per call
            if not (self.is_full() and len(self._dirty) >= self.capacity):
                if len(self._dirty) > self.capacity:
                    self._dirty = self._dirty[-self.capacity:]
                return None
            self._unstackable_at = -1
        if self._mirror is None or len(self._mirror) != len(first) or any(
                m.shape[1:] != x.shape or m.device != x.device or m.dtype != x.dtype for m, x in zip(self._mirror, first)):
            self._mirror = [torch.empty((self.capacity,) + tuple(x.shape), dtype=x.dtype, device=x.device) for x in first]
            self._dirty = list(range(n))
        dirty = sorted(set(i for i in self._dirty if i < n))
        if dirty:
            for f, m in enumerate(self._mirror):
                rows = [self.memory[i][f] for i in dirty]
                if any(r.shape != m.shape[1:] or r.device != m.device or r.dtype != m.dtype for r in rows):
                    self._mirror, self._dirty, self._unstackable_at = None, [], n
                    return None
                m.index_copy_(0, torch.tensor(dirty, dtype=torch.int64, device=m.device), torch.stack(rows))   # index on the field's device
        self._dirty = []
        return [m[:n] for m in self._mirror]

    def stacked_capacity_fields(self):
        """The tensors `as_tensors()` returns views of, at their full (capacity, ...) extent -- rows >= len(self) are unwritten.
        What a trainer's CAPTURED step gathers from: the extent never changes while the memory grows, so the recorded
        index_select kernels stay valid (indices are always < len(self)).  None when there is no stacked view."""
        if self.as_tensors() is None:
            return None
        return list(self._mirror)


def replay_slot_runs(position, length, capacity, n):
    """Where `n` successive `ReplayMemory.push` calls put their items, given the memory's (position, length, capacity) before the
    first: (runs, position', length').  A run (first, slot, count) says that pushes first .. first + count - 1 land in slots
    slot .. slot + count - 1; the runs are TRIMMED to the pushes that are still there after the last one, so they name disjoint
    slots and a push that a later push of the same n overwrites is in no run.

    push writes at `position` while position < length and appends at index `length` otherwise, then advances position modulo
    capacity.  So n pushes are (a) while the write position is AHEAD of the length (only after clear()): capacity - position
    appends at length, length + 1, ..., until the position wraps to 0; then (b) a ring: slot = position, overwriting below the
    length and appending at it, where the two indices coincide.  With position <= length there is only (b).  Of the ring the
    last min(m, capacity) pushes survive, one run or two when they wrap; the ring after (a) starts at slot 0, so it either does
    not wrap (one run, and the appends of (a) survive from slot max(length, m) on) or has overwritten all of (a): never more
    than nat.REPLAY_MAX_RUNS = 2 runs."""
    position, length, capacity, n = int(position), int(length), int(capacity), int(n)
    if capacity < 1 or not 0 <= position < capacity or not 0 <= length <= capacity or n < 0:
        raise ValueError("no replay memory is in the state (position %d, length %d, capacity %d)" % (position, length, capacity))
    runs = []
    if position > length:
        ahead = min(n, capacity - position)               # (a): appended at length + j
        ring, ring_slot, ring_first = n - ahead, 0, ahead
        lo = max(length, min(ring, capacity))             # the ring that follows covers slots [0, min(ring, capacity))
        if lo < length + ahead:
            runs.append((lo - length, lo, length + ahead - lo))
        new_length = max(length + ahead, min(capacity, ring))
    else:
        ring, ring_slot, ring_first = n, position, 0
        new_length = max(length, min(capacity, position + n))
    kept = min(ring, capacity)                            # (b): the last `kept` pushes of the ring
    first = ring_first + ring - kept
    slot = (ring_slot + ring - kept) % capacity
    head = min(kept, capacity - slot)
    if head:
        runs.append((first, slot, head))
    if kept - head:
        runs.append((first + head, 0, kept - head))
    return runs, (position + n) % capacity, new_length


REPLAY_FIELD_SHAPES = {"mprl": lambda H: ((1, 9), (H, 5), (1,), (1,), (1, 9), (H, 5)),
                       "gcn": lambda H: ((H, 13), (1,), (1,), (H, 13))}


class DeviceReplayMemory(Dataset):
    """`ReplayMemory` for tuples of equally shaped tensors, stored as one (capacity, *shape) tensor per tuple field and nothing
    else: item i is the tuple of row views `field[i]`, `as_tensors()` the [:len] views, `stacked_capacity_fields()` the tensors
    themselves -- allocated by the first push and never replaced, so a captured trainer step keeps gathering from them.  Same
    ring as ReplayMemory (clear() keeps the write position; while it is at or ahead of the length, items are appended): item i
    always holds what item i of a ReplayMemory holds after the same pushes and clears.  The first push fixes shapes, dtype and
    device; anything else afterwards is a ValueError (ReplayMemory remains for ragged items).

    `push(item)` copies one item into its slot on any torch device.  `push_episodes(...)` stores every transition of a batch of
    recorded episodes with one library call (rgl_replay_push_f32: device tensors only), `push_sarl_episodes(...)` the same
    with SARL / OM-SARL's rows (rgl_replay_push_sarl_f32)."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be at least 1")
        self.position = 0
        self._length = 0
        self._fields = None           # per field: (capacity, *item shape)
        self._workspace = None

    # -- storage -------------------------------------------------------------------------------------------------
    def _allocate(self, shapes, dtype, device):
        self._fields = [torch.empty((self.capacity,) + tuple(shape), dtype=dtype, device=device) for shape in shapes]

    def _check(self, shapes, dtype, device):
        have = [tuple(f.shape[1:]) for f in self._fields]
        if have != [tuple(x) for x in shapes] or any(f.dtype != dtype or f.device != device for f in self._fields):
            raise ValueError("this memory holds items of shapes %s (%s on %s), not %s (%s on %s)"
                             % (have, self._fields[0].dtype, self._fields[0].device, [tuple(x) for x in shapes], dtype, device))

    def push(self, item):
        if not (isinstance(item, tuple) and item and all(torch.is_tensor(x) for x in item)):
            raise ValueError("DeviceReplayMemory stores tuples of tensors (ReplayMemory takes anything)")
        shapes, dtype, device = [tuple(x.shape) for x in item], item[0].dtype, item[0].device
        if any(x.dtype != dtype or x.device != device for x in item):
            raise ValueError("the fields of an item must share dtype and device")
        if self._fields is None:
            self._allocate(shapes, dtype, device)
        else:
            self._check(shapes, dtype, device)
        if self.position < self._length:
            slot = self.position
        else:
            slot = self._length                    # (after clear() the write position is ahead of the length: upstream's ring)
            self._length += 1
        for field, x in zip(self._fields, item):
            field[slot].copy_(x)
        self.position = (self.position + 1) % self.capacity

    def is_full(self):
        return self._length == self.capacity

    def clear(self):
        self._length = 0              # the write position is kept, as upstream does; so are the tensors

    def __getitem__(self, index):
        i = int(index)
        if i < 0:
            i += self._length
        if not 0 <= i < self._length:
            raise IndexError("replay memory index out of range")
        return tuple(field[i] for field in self._fields)

    def __len__(self):
        return self._length

    def as_tensors(self):
        """[field 0 of every item (n, ...), field 1 ..., ...] in item order: views, nothing is copied.  None while empty."""
        if self._length == 0:
            return None
        return [field[:self._length] for field in self._fields]

    def stacked_capacity_fields(self):
        """The stored tensors at their full (capacity, ...) extent -- rows >= len(self) are unwritten.  None while empty."""
        if self._length == 0:
            return None
        return list(self._fields)

    # -- a batch of episodes ---------------------------------------------------------------------------------------
    def push_episodes(self, robot, humans, rewards, info, layout, kinematics, step_discount, imitation_learning,
                      lengths=None, outcomes=None):
        """Every transition of B recorded lock-step episodes, as `VectorExplorer.update_memory` pushes them episode by episode.
        robot (T,B,9), humans (T,B,H,5), rewards (T,B) float32 and info (T,B) int32 device tensors: row t is the state the policy
        saw at step t and the reward / BatchedCrowdSim info code that step returned (5 = finished earlier).  layout "mprl":
        items (robot (1,9), humans (H,5), value (1,), reward (1,), next robot, next humans); "gcn": (state (H,13), value, reward,
        next state) with the rows `rotate` makes under `kinematics`.  Episodes that ended in a collision or at the goal are
        stored, L - 1 tuples each, episode-major; value = the float64 discounted return-to-go rounded to float32 (imitation
        learning) or 0.

        lengths / outcomes: per episode the number of steps with info != 5 and the last end code, as host arrays -- the explorer
        has them for its statistics; they only move `position` and `len` and size the slot map.  Without them they are read back
        from `info`, which waits for the device.  Otherwise the call synchronises nothing: three launches on the current stream.
        Returns the number of tuples pushed."""
        if layout not in nat.REPLAY_LAYOUTS:
            raise ValueError("unknown layout %r" % (layout,))

        def call(lib, job):
            job.layout = nat.REPLAY_LAYOUTS[layout]
            return lib.rgl_replay_push_f32(C.byref(job))
        return self._push_recorded(robot, humans, rewards, info, kinematics, step_discount, imitation_learning, lengths, outcomes,
                                   REPLAY_FIELD_SHAPES[layout], call, "rgl_replay_push_f32")

    def push_sarl_episodes(self, robot, humans, rewards, info, kinematics, step_discount, imitation_learning, om=None,
                           lengths=None, outcomes=None):
        """`push_episodes` with the rows SARL / OM-SARL train on (rgl_replay_push_sarl_f32): items (state (H,D), value (1,), reward
        (1,), next state (H,D)), a state being what `SARL.transform` makes of (robot, humans) -- the 13 features of `rotate` under
        `kinematics` and, with om = (cell_num, cell_size, om_channel_size), D = 13 + cell_num^2 om_channel_size, the slots
        `occupancy_maps` gives from the float32 human states behind them: the bits `VectorExplorer.update_memory` stores.  om None:
        D = 13.  Everything else -- the recorded tensors, lengths / outcomes, what synchronises, the return value -- as there."""
        rows = nat.RglReplaySarlRows()
        if om is not None:
            try:
                cell_num, cell_size, channels = om
                ok = (int(cell_num) == cell_num and int(channels) == channels and 1 <= cell_num <= 8 and 1 <= channels <= 3
                      and float(cell_size) > 0.0)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("om must be None or (cell_num 1..8, cell_size > 0, om_channel_size 1..3), not %r" % (om,))
            rows.cell_num, rows.cell_size, rows.channels = int(cell_num), float(cell_size), int(channels)
        D = 13 + rows.cell_num ** 2 * rows.channels

        def shapes(H):
            if om is not None and H < 2:
                # upstream: np.concatenate of an empty list (multi_human_rl.py:125-126)
                raise ValueError("need at least one array to concatenate: occupancy maps of a single human have no other humans")
            return ((H, D), (1,), (1,), (H, D))

        def call(lib, job):
            return lib.rgl_replay_push_sarl_f32(C.byref(job), C.byref(rows))
        return self._push_recorded(robot, humans, rewards, info, kinematics, step_discount, imitation_learning, lengths, outcomes,
                                   shapes, call, "rgl_replay_push_sarl_f32")

    def _push_recorded(self, robot, humans, rewards, info, kinematics, step_discount, imitation_learning, lengths, outcomes,
                       field_shapes, call, entry):
        """What the pushes of recorded episodes share: the argument checks, the slot runs, the workspace and the job.  field_shapes(H)
        gives the item's field shapes (and refuses an H the layout cannot take); call(lib, job) makes the library call `entry`."""
        if kinematics not in nat.KINEMATICS:
            raise ValueError("unknown kinematics %r" % (kinematics,))
        robot = _require_device_tensor(robot, "recorded robot states")
        humans = _require_device_tensor(humans, "recorded human states")
        rewards = _require_device_tensor(rewards, "recorded rewards")
        if not (torch.is_tensor(info) and info.dtype == torch.int32 and info.device == robot.device):
            raise TypeError("info must be an int32 tensor on the states' device")
        info = info.contiguous()
        if robot.dim() != 3 or humans.dim() != 4:
            raise ValueError("robot must be (T, B, 9) and humans (T, B, H, 5)")
        T, B, H = int(humans.shape[0]), int(humans.shape[1]), int(humans.shape[2])
        if (tuple(robot.shape) != (T, B, 9) or tuple(humans.shape) != (T, B, H, 5) or tuple(rewards.shape) != (T, B)
                or tuple(info.shape) != (T, B) or humans.device != robot.device or rewards.device != robot.device):
            raise ValueError("robot (T,B,9), humans (T,B,H,5), rewards (T,B) and info (T,B) must agree and share a device")
        shapes = field_shapes(H)
        if lengths is None or outcomes is None:
            host = info.cpu().numpy()
            lengths = (host != 5).sum(0)
            outcomes = np.zeros(B, np.int64)
            for t in range(T):
                ended = (host[t] >= COLLISION) & (host[t] <= TIMEOUT)
                outcomes = np.where(ended, host[t], outcomes)
        lengths, outcomes = np.asarray(lengths).astype(np.int64), np.asarray(outcomes).astype(np.int64)
        if lengths.shape != (B,) or outcomes.shape != (B,):
            raise ValueError("lengths and outcomes must have one entry per episode")
        stored = ((outcomes == COLLISION) | (outcomes == SUCCESS)) & (lengths > 1)
        n = int((lengths[stored] - 1).sum())
        if self._fields is None:
            self._allocate(shapes, torch.float32, robot.device)
        else:
            self._check(shapes, torch.float32, robot.device)
        runs, position, length = replay_slot_runs(self.position, self._length, self.capacity, n)
        lib = nat.lib()
        nbytes = int(lib.rgl_replay_push_workspace_bytes(T, B))
        if self._workspace is None or self._workspace.numel() < nbytes or self._workspace.device != robot.device:
            self._workspace = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=robot.device)
        if nat.poison_workspaces():
            self._workspace.fill_(255)               # tests: NaN bit patterns wherever a kernel reads what this call did not write
        job = nat.RglReplayPushJob()
        job.robot, job.humans, job.rewards, job.info = robot.data_ptr(), humans.data_ptr(), rewards.data_ptr(), info.data_ptr()
        job.T, job.B, job.H = T, B, H
        job.kinematics = nat.KINEMATICS[kinematics]
        job.imitation_learning, job.step_discount, job.capacity = int(bool(imitation_learning)), float(step_discount), self.capacity
        for f, field in enumerate(self._fields):
            job.fields[f] = field.data_ptr()
        job.n_runs = len(runs)
        for r, (first, slot, count) in enumerate(runs):
            job.runs[r].first, job.runs[r].slot, job.runs[r].count = first, slot, count
        job.workspace, job.workspace_bytes = self._workspace.data_ptr(), self._workspace.numel()
        with torch.cuda.device(robot.device):
            job.stream = _stream()
            rc = call(lib, job)
        nat.check(rc, entry)
        self.position, self._length = position, length
        return n


def discounted_statistics(rewards, lengths, step_discount):
    """rewards (T,B) (zeros after an episode's end), lengths (B,) -> per episode (cumulative discounted reward,
    mean over its steps of the discounted return-to-go), as explorer.py:78-85 computes them.
    step_discount = gamma ** (time_step * v_pref)."""
    rewards = np.asarray(rewards, np.float64)
    T, B = rewards.shape
    togo = np.zeros((T + 1, B))
    for t in range(T - 1, -1, -1):                       # return-to-go G_t = r_t + d * G_{t+1}
        togo[t] = rewards[t] + step_discount * togo[t + 1]
    cumulative = togo[0].copy()
    valid = np.arange(T)[:, None] < np.asarray(lengths)[None, :]
    avg_return = np.where(valid, togo[:T], 0.0).sum(0) / np.maximum(np.asarray(lengths), 1)
    return cumulative, avg_return


def _mean(values):
    values = list(values)
    return sum(values) / len(values) if values else 0


class VectorExplorer(object):
    def __init__(self, sim, policy, device=None, writer=None, memory=None, gamma=None, target_policy=None,
                 case_size=None, max_batch=4096, exploration="host"):
        if exploration not in ("host", "device"):
            raise ValueError("exploration must be 'host' or 'device', not %r" % (exploration,))
        self.exploration = exploration
        self._explore = None                    # exploration="device", train phase: the chunk's stream states and outputs
        self.sim = sim
        self.policy = policy                    # the acting policy (needs predict_batch)
        self.device = device or sim.device
        self.writer = writer
        self.memory = memory
        self.gamma = gamma
        self.target_policy = target_policy
        self.statistics = None
        self.case_size = dict(CASE_SIZE, **(case_size or {}))
        self.case_counter = {"train": 0, "val": 0, "test": 0}
        self.max_batch = int(max_batch)
        self.last_run = None                    # per-episode arrays of the most recent call

    # -- episodes ------------------------------------------------------------------------------------------------
    def _next_cases(self, phase, k):
        cases = [(self.case_counter[phase] + i) % self.case_size[phase] for i in range(k)]
        self.case_counter[phase] = (self.case_counter[phase] + k) % self.case_size[phase]
        return cases

    def _act(self, robot32, humans32, phase, n_actions):
        if getattr(self.policy, "acts_in_velocity", False):
            return self.policy.predict_batch(self.sim.robot, self.sim.humans, roots_are_joint_states=True, done=self.sim.done)
        idx, _ = self.policy.predict_batch(robot32, humans32, roots_are_joint_states=True)
        if self._explore is not None:
            return self._select_on_device(idx, n_actions)
        idx = idx.long()
        eps = getattr(self.policy, "epsilon", None)
        if phase == "train" and eps:
            B = robot32.shape[0]
            explore = torch.as_tensor(np.random.random(B) < eps, device=idx.device)
            rand_idx = torch.as_tensor(np.random.randint(0, n_actions, B), device=idx.device)
            idx = torch.where(explore, rand_idx, idx)
        return idx

    def _seed_exploration(self, table, phase="train"):
        """The chunk's stream states, continued from where scene generation left each case's stream, and the select kernel's
        outputs (one buffer per chunk; `explored` is recorded per step).  A nonstop simulator's own streams are used as they
        are -- its regenerations read what follows each decision -- and outside `train` the draw is made with epsilon 0."""
        sim = self.sim
        if sim.scene_seeds is None or sim.scene_draws is None:
            raise ValueError("exploration='device' needs a simulator reset from seeded cases: loaded states carry no stream")
        B, dev = sim.B, sim.device
        if getattr(sim.cfg, "nonstop_human", False):
            state = sim.stream
        else:
            state = torch.empty(B, nat.EXPLORE_STATE_WORDS, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                rc = nat.lib().crowd_explore_seed_u32(sim.scene_seeds.data_ptr(), sim.scene_draws.data_ptr(), B, state.data_ptr(), _stream())
            nat.check(rc, "crowd_explore_seed_u32")
        eps = getattr(self.policy, "epsilon", None)
        return {"state": state, "table": table, "epsilon": 0.0 if eps is None or phase != "train" else float(eps), "explored": [],
                "action": torch.empty(B, 2, dtype=torch.float64, device=dev)}

    def _select_on_device(self, greedy, n_actions):
        """One decision of every live environment on its own stream (crowd_explore_select_f64): the chosen indices; the action
        rows are left in self._explore["action"] for the step."""
        ex, sim = self._explore, self.sim
        greedy = greedy.to(torch.int32).contiguous()
        chosen = torch.empty_like(greedy)
        explored = torch.empty_like(greedy)
        job = nat.CrowdExploreJob()
        job.greedy, job.done, job.table, job.state = greedy.data_ptr(), sim.done.data_ptr(), ex["table"].data_ptr(), ex["state"].data_ptr()
        job.chosen, job.action, job.explored = chosen.data_ptr(), ex["action"].data_ptr(), explored.data_ptr()
        job.epsilon, job.B, job.n_actions = ex["epsilon"], sim.B, int(n_actions)
        with torch.cuda.device(sim.device):
            job.stream = _stream()
            rc = nat.lib().crowd_explore_select_f64(C.byref(job))
        nat.check(rc, "crowd_explore_select_f64")
        ex["explored"].append(explored)
        return chosen

    def _run_chunk(self, phase, cases, keep_states):
        sim, policy = self.sim, self.policy
        robot32, humans32 = sim.reset(phase, cases)
        B = sim.B
        self._explore = None
        nonstop = bool(getattr(sim.cfg, "nonstop_human", False))
        velocity = bool(getattr(policy, "acts_in_velocity", False))
        if velocity:
            policy.check_kinematics(sim.kinematics)
            table = None
        else:
            if policy.action_space is None:
                policy.build_action_space(sim.cfg.robot_v_pref)
            table = torch.tensor(as_array(policy.action_space), dtype=torch.float64, device=sim.device)
            # val / test: no draw is observable and no kernel runs -- unless nonstop humans read the stream after each decision
            if self.exploration == "device" and (phase == "train" or nonstop):
                self._explore = self._seed_exploration(table, phase)
        # nonstop humans: what the step skips on the stream for the decision's draw, where the select kernel has not made it there
        step_kw = {"policy_draws": 0 if (velocity or self._explore is not None) else 1} if nonstop else {}
        max_steps = int(round(sim.cfg.time_limit / sim.cfg.time_step)) + 2
        outcome = torch.zeros(B, dtype=torch.int32, device=sim.device)
        rewards, infos, dmins, states, actions = [], [], [], [], []
        # a memory that takes whole chunks (DeviceReplayMemory.push_episodes): the states, rewards and info codes are recorded
        # into (max_steps, B, ...) tensors -- the simulator writes rewards / info / dmin in place -- instead of per-step clones
        record = None
        if keep_states and hasattr(self.memory, "push_sarl_episodes" if self._sarl_target() else "push_episodes") and (
                not self._sarl_target() or self.target_policy.training_enabled()):
            record = (torch.empty((max_steps,) + tuple(robot32.shape), dtype=torch.float32, device=sim.device),
                      torch.empty((max_steps,) + tuple(humans32.shape), dtype=torch.float32, device=sim.device),
                      torch.empty(max_steps, B, dtype=torch.float32, device=sim.device),
                      torch.empty(max_steps, B, dtype=torch.int32, device=sim.device),
                      torch.empty(max_steps, B, dtype=torch.float64, device=sim.device))
        for _ in range(max_steps):
            if not bool((sim.done == 0).any()):
                break
            t = len(infos)
            if record is not None:
                record[0][t].copy_(robot32)
                record[1][t].copy_(humans32)
            elif keep_states:
                states.append((robot32.clone(), humans32.clone()))
            idx = self._act(robot32, humans32, phase, None if velocity else table.shape[0])
            if velocity:
                act = idx
            elif self._explore is not None:
                act = self._explore["action"]                # the select kernel's rows: table[idx], bit for bit
            else:
                act = table[idx]
            (robot32, humans32), reward, _, info = sim.step(act,
                                                            out=None if record is None else tuple(r[t] for r in record[2:]),
                                                            **step_kw)
            if velocity:
                idx = idx.clone()                        # the policy may hand out one buffer per call
            actions.append(idx)
            rewards.append(reward)
            infos.append(info)
            dmins.append(sim.last_dmin)
            ended = (info >= COLLISION) & (info <= TIMEOUT)
            outcome = torch.where(ended, info, outcome)
        info_t = torch.stack(infos).cpu().numpy()                    # (T,B); 5 = finished earlier
        if nonstop:
            capped = torch.nonzero(sim.nonstop_status).flatten().tolist()
            if capped:
                raise UnplacedSceneError("%d of %d %s episodes had a nonstop human that found no place within scene_max_attempts = %d "
                                         "attempts: cases %s.  Raise SimConfig.scene_max_attempts."
                                         % (len(capped), B, phase, int(sim.cfg.scene_max_attempts), [cases[b] for b in capped]),
                                         [(phase, cases[b]) for b in capped])
        live = info_t != 5
        lengths = live.sum(0)
        reward_t = np.where(live, torch.stack(rewards).cpu().numpy().astype(np.float64), 0.0)
        return {"outcome": outcome.cpu().numpy(), "time": sim.time.cpu().numpy().copy(), "lengths": lengths,
                "rewards": reward_t, "info": info_t, "dmin": torch.stack(dmins).cpu().numpy(),
                "states": states, "actions": actions,
                "explored": None if self._explore is None else self._explore["explored"],
                "recorded": None if record is None else tuple(r[:len(infos)] for r in record[:4])}

    def run_k_episodes(self, k, phase, update_memory=False, imitation_learning=False, episode=None, epoch=None,
                       print_failure=False):
        if update_memory and getattr(self.target_policy, "name", None) == "LSTM-RL":
            # evaluation only: the recurrent value network has no backward pass, and nothing fills a memory with its sorted rows
            raise NotImplementedError("LSTM-RL training is not provided: the replay memory does not store LSTM-RL's sorted rows and "
                                      "the value network has no backward pass")
        if update_memory and self._sarl_target():
            if not self.target_policy.training_enabled():
                # opt-in, like the network's backward pass: SARL's replay rows carry the occupancy maps behind the 13 relation features
                raise NotImplementedError("SARL training is not provided until policy.enable_training() is called: the replay memory "
                                          "then stores SARL's %d-wide rows" % self.target_policy.input_dim())
            if self.memory is None or self.gamma is None:
                raise ValueError('Memory or gamma value is not set!')
        self.policy.set_phase(phase)
        cases = self._next_cases(phase, k)
        time_limit = self.sim.cfg.time_limit
        step_discount = pow(self.gamma if self.gamma is not None else 0.9,
                            self.sim.cfg.time_step * self.sim.cfg.robot_v_pref)
        success_times, collision_times, timeout_times = [], [], []
        collision_cases, timeout_cases, min_dist = [], [], []
        cumulative_rewards, average_returns = [], []
        discomfort = 0
        per_episode = {"case": [], "outcome": [], "time": [], "length": [], "actions": []}
        if self.exploration == "device":
            per_episode["explored"] = []                 # per episode: 0 / 1 per decision (all 0 where no stream is drawn from)
        for lo in range(0, k, self.max_batch):
            chunk = cases[lo:lo + self.max_batch]
            run = self._run_chunk(phase, chunk, keep_states=update_memory)
            if (run["outcome"] == 0).any():
                raise ValueError('Invalid end signal from environment')
            cum, avg_ret = discounted_statistics(run["rewards"], run["lengths"], step_discount)
            velocity = bool(getattr(self.policy, "acts_in_velocity", False))
            acts = torch.stack(run["actions"]).cpu().numpy() if run["actions"] else np.zeros((0, len(chunk)), np.int64)
            took = torch.stack(run["explored"]).cpu().numpy() if run["explored"] else None
            for b in range(len(chunk)):
                i = lo + b
                code = int(run["outcome"][b])
                if code == SUCCESS:
                    success_times.append(float(run["time"][b]))
                elif code == COLLISION:
                    collision_cases.append(i)
                    collision_times.append(float(run["time"][b]))
                else:
                    timeout_cases.append(i)
                    timeout_times.append(time_limit)
                cumulative_rewards.append(float(cum[b]))
                average_returns.append(float(avg_ret[b]))
                per_episode["case"].append(chunk[b])
                per_episode["outcome"].append(code)
                per_episode["time"].append(float(run["time"][b]))
                per_episode["length"].append(int(run["lengths"][b]))
                if velocity:
                    per_episode["actions"].append([(float(a[0]), float(a[1])) for a in acts[:int(run["lengths"][b]), b]])
                else:
                    per_episode["actions"].append([int(a) for a in acts[:int(run["lengths"][b]), b]])
                if "explored" in per_episode:
                    n = int(run["lengths"][b])
                    per_episode["explored"].append([0] * n if took is None else [int(x) for x in took[:n, b]])
            danger = run["info"] == 1
            discomfort += int(danger.sum())
            min_dist.extend(run["dmin"][danger].tolist())
            if update_memory and run["recorded"] is not None:
                self._push_chunk(run, imitation_learning)
            elif update_memory:
                for b in range(len(chunk)):
                    if int(run["outcome"][b]) in (SUCCESS, COLLISION):       # positive or negative experience only
                        T = int(run["lengths"][b])
                        self.update_memory([(s[0][b:b + 1], s[1][b]) for s in run["states"][:T]],
                                           [a[b] for a in run["actions"][:T]],
                                           [float(r) for r in run["rewards"][:T, b]], imitation_learning)
        success, collision, timeout = len(success_times), len(collision_times), len(timeout_times)
        assert success + collision + timeout == k
        success_rate, collision_rate = success / k, collision / k
        avg_nav_time = sum(success_times) / len(success_times) if success_times else time_limit

        extra_info = '' if episode is None else 'in episode {} '.format(episode)
        extra_info = extra_info + '' if epoch is None else extra_info + ' in epoch {} '.format(epoch)
        logging.info('{:<5} {}has success rate: {:.2f}, collision rate: {:.2f}, nav time: {:.2f}, total reward: {:.4f},'
                     ' average return: {:.4f}'.format(phase.upper(), extra_info, success_rate, collision_rate,
                                                      avg_nav_time, _mean(cumulative_rewards), _mean(average_returns)))
        if phase in ['val', 'test']:
            total_time = sum(success_times + collision_times + timeout_times)
            logging.info('Frequency of being in danger: %.2f and average min separate distance in danger: %.2f',
                         discomfort / total_time, _mean(min_dist))
        if print_failure:
            logging.info('Collision cases: ' + ' '.join([str(x) for x in collision_cases]))
            logging.info('Timeout cases: ' + ' '.join([str(x) for x in timeout_cases]))

        self.last_run = dict(per_episode, cumulative_reward=cumulative_rewards, average_return=average_returns,
                             discomfort_steps=discomfort, min_dist=min_dist)
        self.statistics = (success_rate, collision_rate, avg_nav_time, _mean(cumulative_rewards), _mean(average_returns))
        return self.statistics

    # -- replay memory -------------------------------------------------------------------------------------------
    def _transform(self, state):
        """(robot (1,9), humans (H,5)) -> what `target_policy.transform(JointState)` returns for that state."""
        if self.target_policy.name == 'ModelPredictiveRL':
            return state
        robot, humans = state
        joint = torch.cat([robot.expand(humans.shape[0], 9), humans], dim=1).contiguous()
        return rotate(joint, self.target_policy.kinematics)

    def _sarl_target(self):
        """The target policy is SARL / OM-SARL: its replay rows carry the occupancy maps (push_sarl_episodes; the host loop of
        update_memory for a memory without it)."""
        return getattr(self.target_policy, "name", None) in ("SARL", "OM-SARL")

    def _sarl_rows(self, states):
        """(T, H, D) rows of an episode's T states, each what `SARL.transform` makes of it: ONE rotate over the T x H pairs and,
        with maps, ONE sarl_occupancy_maps_f32 over the T crowds (from the float32 states, widened on the device)."""
        pol = self.target_policy
        robots = torch.cat([s[0] for s in states], dim=0)                    # (T, 9)
        humans = torch.stack([s[1] for s in states], dim=0).contiguous()      # (T, H, 5)
        T, H = humans.shape[0], humans.shape[1]
        joint = torch.cat([robots[:, None, :].expand(T, H, 9), humans], dim=2).reshape(T * H, 14).contiguous()
        rows = rotate(joint, pol.kinematics).reshape(T, H, 13)
        if pol.with_om:
            rows = torch.cat([rows, occupancy_maps(humans, pol.cell_num, pol.cell_size, pol.om_channel_size)], dim=2)
        return rows

    def _push_chunk(self, run, imitation_learning):
        """What the update_memory loop of run_k_episodes stores for one chunk, as one `memory.push_episodes` call
        (`push_sarl_episodes` for a SARL / OM-SARL target)."""
        if self.memory is None or self.gamma is None:
            raise ValueError('Memory or gamma value is not set!')
        step_discount = pow(self.gamma, self.sim.cfg.time_step * self.sim.cfg.robot_v_pref)
        mprl = self.target_policy.name == 'ModelPredictiveRL'
        robot, humans, rewards, info = run["recorded"]
        if self._sarl_target():
            pol = self.target_policy
            self.memory.push_sarl_episodes(robot, humans, rewards, info, pol.kinematics, step_discount, imitation_learning,
                                           om=(pol.cell_num, pol.cell_size, pol.om_channel_size) if pol.with_om else None,
                                           lengths=run["lengths"], outcomes=run["outcome"])
            return
        self.memory.push_episodes(robot, humans, rewards, info, "mprl" if mprl else "gcn",
                                  getattr(self.target_policy, "kinematics", None) or "holonomic", step_discount,
                                  imitation_learning, lengths=run["lengths"], outcomes=run["outcome"])

    def update_memory(self, states, actions, rewards, imitation_learning=False):
        """One finished episode: states[i] = (robot (1,9), humans (H,5)) fp32 device tensors (`policy.last_state`)."""
        if self.memory is None or self.gamma is None:
            raise ValueError('Memory or gamma value is not set!')
        step_discount = pow(self.gamma, self.sim.cfg.time_step * self.sim.cfg.robot_v_pref)
        n = len(states)
        togo = [0.0] * (n + 1)
        for t in range(n - 1, -1, -1):
            togo[t] = rewards[t] + step_discount * togo[t + 1]
        mprl = self.target_policy.name == 'ModelPredictiveRL'
        sarl_rows = self._sarl_rows(states) if self._sarl_target() and n > 1 else None
        for i in range(n - 1):                                   # the last state has no successor: not stored
            if imitation_learning:
                value = togo[i]                                  # discounted return from step i
            else:
                value = 0                                        # RL: the trainer bootstraps from the target network
            if sarl_rows is not None:
                state, next_state = sarl_rows[i], sarl_rows[i + 1]
            else:
                state, next_state = self._transform(states[i]), self._transform(states[i + 1])
            value = torch.tensor([value], dtype=torch.float32, device=self.device)
            reward = torch.tensor([rewards[i]], dtype=torch.float32, device=self.device)
            if mprl:
                self.memory.push((state[0], state[1], value, reward, next_state[0], next_state[1]))
            else:
                self.memory.push((state, value, reward, next_state))

    def log(self, tag_prefix, global_step):
        """TensorBoard scalars under the reference's tag names (explorer.py:142-148)."""
        for tag, value in zip(("success_rate", "collision_rate", "time", "reward", "avg_return"), self.statistics):
            self.writer.add_scalar("%s/%s" % (tag_prefix, tag), value, global_step)
