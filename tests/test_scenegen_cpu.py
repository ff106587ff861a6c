"""The ground the device scene generator stands on, checked without a GPU: the plain-integer restatement of numpy's legacy
stream and of sim.generate_scene (tests/scenegen_cpu.py, which csrc/rgl_scenegen.hip is written from) against numpy and the
host generator, the default attempt cap against the attempt counts those cases need, the knife-edge list, and the new entry
point's host-side argument checks."""
import ctypes

import numpy as np
import pytest

from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd import sim as simmod
from relationalgraphlearning_amd.sim import SimConfig
from tests import scenegen_cpu as sg

# (configuration name, phase, case) of circle_crossing cases whose smallest |distance - margin| over all clearance tests is below
# KNIFE_EDGE_GAP: a last-bit difference between the device's and the host libm's cos / sin may flip a rejection there, so the
# GPU comparison leaves them out by name.  Expected empty (a gap below 1e-9 has probability of order 1e-9 per test); the smallest
# gap over all circle cases is 3.6e-7 (19-human circle).
KNIFE_EDGE_GAP = 1e-9
KNIFE_EDGES = ()

SEEDS = (0, 1, 999, 1000, 2000, 2 ** 32 - 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_seeding_equals_numpy_state(seed):
    kind, key, pos = np.random.RandomState(seed).get_state()[:3]
    rs = sg.MT19937(seed)
    assert kind == "MT19937" and pos == 624 == rs.pos
    assert [int(w) for w in key] == rs.mt


@pytest.mark.parametrize("seed", SEEDS)
def test_stream_equals_numpy_bit_for_bit(seed):
    ref, rs = np.random.RandomState(seed), sg.MT19937(seed)
    want = ref.random_sample(2500)                                     # 5000 words: eight twists
    got = np.array([rs.random_sample() for _ in range(2500)])
    assert np.array_equal(want.view(np.uint64), got.view(np.uint64))
    for lo, hi in ((0.5, 1.5), (0.3, 0.5)) * 50:
        assert ref.uniform(lo, hi) == rs.uniform(lo, hi)
    assert rs.draws == 2600


def _walk(name, cfg):
    rows = []
    for phase, case in sg.cases_of(cfg):
        host = sg.host_scene_with_draws(cfg, phase, case)
        mine = sg.generate_scene_restated(cfg, phase, case)
        for a, b in zip(host[:4], mine[:4]):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, phase, case)
        assert host[4] == mine[4]["draws"], (name, phase, case)
        rows.append((phase, case, mine[4]))
    return rows


@pytest.mark.parametrize("name,cfg", sg.configurations(), ids=[n for n, _ in sg.configurations()])
def test_restatement_equals_host_generator_and_stays_under_the_cap(name, cfg):
    rows = _walk(name, cfg)
    worst = max(st["max_attempts"] for _, _, st in rows)
    print("%s: %d cases, draws max %d, attempts of one human max %d, smallest gap %.3e"
          % (name, len(rows), max(st["draws"] for _, _, st in rows), worst, min(st["min_gap"] for _, _, st in rows)))
    assert cfg.scene_max_attempts == simmod.SCENE_MAX_ATTEMPTS == 8 * simmod.SCENE_MAX_ATTEMPTS_MEASURED
    assert worst <= simmod.SCENE_MAX_ATTEMPTS_MEASURED, "the measured maximum beside the constant is out of date"
    assert all(st["status"] == 0 and st["max_attempts"] < simmod.SCENE_MAX_ATTEMPTS for _, _, st in rows)
    knife = tuple((name, phase, case) for phase, case, st in rows if st["min_gap"] < KNIFE_EDGE_GAP)
    if cfg.scenario == "circle_crossing":
        assert knife == tuple(k for k in KNIFE_EDGES if k[0] == name)
        assert len(knife) <= 0.01 * len(rows)
    assert all(k[0].startswith("circle") for k in KNIFE_EDGES)            # the square has no transcendental: nothing is left out


def test_restated_cap_flags_and_stops():
    cfg = SimConfig(scenario="circle_crossing", human_num=15, randomize_attributes=True)
    stats = [sg.generate_scene_restated(cfg, "test", k, max_attempts=300)[4] for k in range(8)]
    assert [st["status"] for st in stats] == [1, 1, 1, 1, 1, 1, 0, 1]        # what the GPU test's cap case relies on: a mix
    assert all(st["draws"] <= 15 * (2 + 3 * 300) for st in stats)
    free = sg.generate_scene_restated(cfg, "test", 6)
    capped = sg.generate_scene_restated(cfg, "test", 6, max_attempts=300)
    assert all(np.array_equal(a, b) for a, b in zip(free[:4], capped[:4])) and free[4]["max_attempts"] <= 300


def test_config_defaults_leave_the_host_generator_in_charge():
    cfg = SimConfig()
    assert cfg.scene_generator == "host" and cfg.scene_max_attempts == simmod.SCENE_MAX_ATTEMPTS

    class Bag(object):
        pass
    c = Bag()
    c.env, c.reward, c.sim, c.humans, c.robot = Bag(), Bag(), Bag(), Bag(), Bag()
    c.env.time_limit, c.env.time_step, c.env.randomize_attributes = 30, 0.25, False
    c.reward.success_reward, c.reward.collision_penalty = 1, -0.25
    c.reward.discomfort_dist, c.reward.discomfort_penalty_factor = 0.2, 0.5
    c.sim.test_scenario, c.sim.square_width, c.sim.circle_radius, c.sim.human_num = "square_crossing", 20, 4, 5
    c.sim.centralized_planning = True
    c.humans.radius, c.humans.v_pref, c.robot.radius, c.robot.v_pref, c.robot.visible = 0.3, 1, 0.3, 1, False
    got = SimConfig.from_env_config(c)
    assert got.scene_generator == "host" and got.scene_max_attempts == simmod.SCENE_MAX_ATTEMPTS


def test_entry_point_is_exported_and_checks_its_arguments_on_the_host():
    lib = nat.lib()
    assert "crowd_generate_scenes_f64" in nat.SIGNATURES
    cfg = simmod._scene_config(SimConfig())
    assert (cfg.scenario, cfg.max_attempts, cfg.circle_radius, cfg.square_width) == (0, simmod.SCENE_MAX_ATTEMPTS, 4.0, 20.0)
    p = ctypes.c_void_p(16)                      # never dereferenced: every call below is refused before a launch

    def call(c, seeds=p, B=1, H=5, robot=p, draws=p):
        return lib.crowd_generate_scenes_f64(c, seeds, B, H, robot, p, p, p, p, draws, None)
    assert call(None) == -3 and call(ctypes.byref(cfg), seeds=None) == -3
    assert call(ctypes.byref(cfg), robot=None) == -3 and call(ctypes.byref(cfg), draws=None) == -3
    assert call(ctypes.byref(cfg), H=0) == -1 and call(ctypes.byref(cfg), H=nat.MAX_NODES) == -1
    assert call(ctypes.byref(cfg), B=0) == -1
    cfg.max_attempts = 0
    assert call(ctypes.byref(cfg)) == -1
    cfg.max_attempts, cfg.scenario = 10, 2
    assert call(ctypes.byref(cfg)) == -2
    with pytest.raises(NotImplementedError):
        simmod._scene_config(SimConfig(scenario="line_crossing"))
    with pytest.raises(ValueError):
        simmod.generate_scenes_device(SimConfig(), "test", [0], "cpu", on_unplaced="ignore")
