"""The SARL / OM-SARL replay push (csrc/rgl_replay.hip: rgl_replay_push_sarl_f32, DeviceReplayMemory.push_sarl_episodes), test
infrastructure: recorded chunks whose crowds stand inside one another's occupancy grids, the host path the push must equal
(`VectorExplorer.update_memory` for a SARL target: one `rotate` and one `occupancy_maps` per episode, one `memory.push` per tuple)
and the float64 maps of tests/sarl_cpu.py for the states a chunk stores."""
import types

import numpy as np
import torch

from relationalgraphlearning_amd.vector_explorer import COLLISION, SUCCESS, ReplayMemory, VectorExplorer
from tests import replay_push as rp
from tests import sarl_cpu as cpu

T = 6
CELL_NUM, CELL_SIZE = 4, 1.0


def om_of(channels):
    return None if not channels else (CELL_NUM, CELL_SIZE, channels)


def chunk_size(H):
    """Episodes of the chunk of a crowd size: 8 (every pairing below) for small crowds, 3 where the float64 reference walks
    thousands of pairs per state in python -- a goal of full length, a collision at step 2 and a time-out of length 1."""
    return 8 if H <= 33 else 3


def crowded_run(H, seed=0):
    """rp.synthetic_run(T, B, H) -- lengths 6, 2, 1, 3, 5, 6, 2, 1; goal, collision, time-out, goal, goal, collision, time-out,
    goal: stored goals and collisions, time-outs that are not stored, stored outcomes of length 1 (no tuple), info == 5 tails of 0 to
    5 steps, NaN in every row past an episode's end -- with the humans of the live steps placed as sarl_cpu.scenes places them:
    around one point, most of them inside one another's 4 m grids, nobody closer than 0.35 m to anybody."""
    B = chunk_size(H)
    run = rp.synthetic_run(T, B, H, seed=seed)
    rng = np.random.RandomState(4201 + 31 * H + seed)
    spread = max(1.1, 0.33 * np.sqrt(H))
    for b in range(B):
        for t in range(int(run["lengths"][b])):
            centre = rng.uniform(-2, 2, 2)
            placed = []
            for h in range(H):
                while True:
                    q = centre + rng.uniform(-spread, spread, 2)
                    if all(np.hypot(*(q - o)) > 0.35 for o in placed):
                        break
                placed.append(q)
            run["humans"][t, b, :, 0:2] = np.asarray(placed, np.float32)
    return run


def stored_states(run):
    """[(t, b)] of the states that land in a memory large enough: states 0 .. L - 1 of every stored episode with L > 1."""
    out = []
    for b in range(run["B"]):
        L = int(run["lengths"][b])
        if int(run["outcome"][b]) in (SUCCESS, COLLISION) and L > 1:
            out.extend((t, b) for t in range(L))
    return out


_MAPS = {}


def reference_maps(run, H, channels):
    """({(t, b): (H, 16 channels) float32}, most humans in one cell of one human's grid) from sarl_cpu.occupancy_maps on the float64
    copies of the recorded float32 states, the count from the coordinates it reports (whose floors pick the cells); computed once per
    (H, channels) for the run of seed 0."""
    key = (H, channels)
    if key not in _MAPS:
        maps, most = {}, 0
        for t, b in stored_states(run):
            coords = []
            maps[(t, b)] = cpu.occupancy_maps(run["humans"][t, b].astype(np.float64), CELL_NUM, CELL_SIZE, channels, coords=coords)
            cells = np.floor(np.asarray(coords).reshape(H, H - 1, 2))                 # [i][other human][x, y]
            inside = ((cells >= 0) & (cells < CELL_NUM)).all(axis=2)
            index = np.where(inside, CELL_NUM * cells[..., 1] + cells[..., 0], -1).astype(np.int64)
            for i in range(H):
                if inside[i].any():
                    most = max(most, int(np.bincount(index[i][inside[i]]).max()))
        _MAPS[key] = (maps, most)
    return _MAPS[key]


def sarl_target(kinematics, om):
    """What update_memory and _push_chunk read of a SARL / OM-SARL target policy."""
    return types.SimpleNamespace(name="SARL" if om is None else "OM-SARL", kinematics=kinematics, with_om=om is not None,
                                 cell_num=om[0] if om else CELL_NUM, cell_size=om[1] if om else CELL_SIZE,
                                 om_channel_size=om[2] if om else 3, training_enabled=lambda: True)


def host_tuples(run, kinematics, om, imitation_learning, device):
    """What run_k_episodes' update_memory loop pushes for the recorded chunk, in push order."""
    sim = types.SimpleNamespace(cfg=types.SimpleNamespace(time_step=rp.TIME_STEP, robot_v_pref=rp.V_PREF), device=device)
    memory = ReplayMemory(1 << 20)
    ex = VectorExplorer(sim, None, device=device, memory=memory, gamma=rp.GAMMA, target_policy=sarl_target(kinematics, om))
    robot, humans = torch.as_tensor(run["robot"]).to(device), torch.as_tensor(run["humans"]).to(device)
    reward_t = np.where(run["info"] != 5, run["rewards"].astype(np.float64), 0.0)
    for b in range(run["B"]):
        if int(run["outcome"][b]) in (SUCCESS, COLLISION):
            L = int(run["lengths"][b])
            ex.update_memory([(robot[t][b:b + 1], humans[t][b]) for t in range(L)], [None] * L,
                             [float(r) for r in reward_t[:L, b]], imitation_learning)
    return list(memory.memory)
