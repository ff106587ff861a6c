"""The device scene generator (csrc/rgl_scenegen.hip) against the host generator sim.generate_scene -- which tests/test_sim.py
pins to the reference's scenes -- on every configuration and case of tests/scenegen_cpu.py, through the public path
(BatchedCrowdSim.reset, VectorExplorer) and at its attempt cap.

Bounds.  square_crossing has no transcendental: everything equals the host's bit for bit.  circle_crossing: radii and v_pref bit
for bit; px = R * cos(angle) + noise (py likewise, goals their negations) within K * 2**-52 * (R + v_pref_max / 2), where K rests
on the device's float64 sin / cos against the host libm's.  ROCm ships no accuracy table for them, so K is measured: the device
functions on the accepted angles of these very cases (30 180 angles, tools/scenegen_sincos.py) deviate from numpy's by at most
SINCOS_DEVIATION units of 2**-52; K is twice that plus one unit each for the multiply and the add.
"""
import numpy as np
import pytest
import torch

from relationalgraphlearning_amd.sim import (BatchedCrowdSim, SimConfig, UnplacedSceneError, generate_scene,
                                             generate_scenes_device)
from tests import scenegen_cpu as sg
from tests.test_scenegen_cpu import KNIFE_EDGES

pytestmark = pytest.mark.gpu

SINCOS_DEVIATION = 0.5           # measured maximum of |device - numpy| over sin and cos, in units of 2**-52 (profiles/scenegen.txt)
K = 2 * SINCOS_DEVIATION + 2


def bound(cfg):
    v_pref_max = 1.5 if cfg.randomize_attributes else cfg.human_v_pref
    return K * 2.0 ** -52 * (cfg.circle_radius + v_pref_max / 2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _compare(name, cfg, host, got, what):
    """host, got: (robot, humans, goals, vpref) arrays of one case."""
    hr, hh, hg, hv = host
    gr, gh, gg, gv = got
    assert np.array_equal(_bits(hr), _bits(gr)), (name, what, "robot")
    assert np.array_equal(_bits(hv), _bits(gv)), (name, what, "v_pref")
    assert np.array_equal(_bits(hh[:, 2:]), _bits(gh[:, 2:])), (name, what, "velocity and radius")
    if cfg.scenario == "square_crossing":
        assert np.array_equal(_bits(hh), _bits(gh)) and np.array_equal(_bits(hg), _bits(gg)), (name, what)
        return 0.0
    err = max(float(np.abs(hh[:, :2] - gh[:, :2]).max()), float(np.abs(hg - gg).max()))
    assert err <= bound(cfg), (name, what, err, bound(cfg))
    return err


@pytest.mark.parametrize("name,cfg", sg.configurations(), ids=[n for n, _ in sg.configurations()])
def test_device_scenes_equal_the_host_generator(dev, name, cfg):
    left_out = set((p, k) for n, p, k in KNIFE_EDGES if n == name)
    worst, n_cases = 0.0, 0
    for phase, cases in sg.by_phase(sg.cases_of(cfg)).items():
        cases = [k for k in cases if (phase, k) not in left_out]
        robot, humans, goals, vpref, status, draws = (t.cpu().numpy() for t in generate_scenes_device(cfg, phase, cases, dev))
        assert status.dtype == np.int32 and draws.dtype == np.int32
        assert int(status.sum()) == 0, (name, phase, [cases[b] for b in np.nonzero(status)[0]])
        host = [sg.host_scene_with_draws(cfg, phase, k) for k in cases]
        host_draws = np.array([h[4] for h in host])
        assert np.array_equal(draws, host_draws), (name, phase, [cases[b] for b in np.nonzero(draws != host_draws)[0]][:8])
        for b, k in enumerate(cases):
            worst = max(worst, _compare(name, cfg, host[b][:4], (robot[b], humans[b], goals[b], vpref[b]), (phase, k)))
        n_cases += len(cases)
    print("%s: %d cases, largest position difference %.3e (bound %.3e)" % (name, n_cases, worst, bound(cfg)))


def _f32_close(a, b, cfg):
    """float32 views of two float64 values within bound(cfg): equal, or the two neighbours the values straddle."""
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    if cfg.scenario == "square_crossing":
        return np.array_equal(a, b)
    return bool((np.abs(a - b) <= bound(cfg) + np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))).all())


@pytest.mark.parametrize("scenario,h", [("square_crossing", 4), ("circle_crossing", 5)])
def test_reset_with_the_device_generator(dev, scenario, h):
    cfg = SimConfig(scenario=scenario, human_num=h)
    cases = list(range(300, 364)) + [sg.TRAIN_SIZE - 1]
    host = BatchedCrowdSim(dev, cfg)
    r_h, h_h = (t.clone() for t in host.reset("train", cases))
    sim = BatchedCrowdSim(dev, cfg)
    r_d, h_d = sim.reset("train", cases, generator="device")
    assert r_d.dtype == torch.float32 and h_d.shape == (len(cases), h, 5)
    assert _f32_close(r_h, r_d, cfg) and _f32_close(h_h, h_d, cfg)
    assert sim._scene_cache == {} and len(host._scene_cache) == len(cases)
    assert sim.human_goals.shape == (len(cases), h, 2) and sim.human_vpref.shape == (len(cases), h)
    assert float(sim.time.abs().max()) == 0.0 and int(sim.done.sum()) == 0
    # the switch on the configuration does the same without the argument
    via_cfg = BatchedCrowdSim(dev, SimConfig(scenario=scenario, human_num=h, scene_generator="device"))
    r_c, h_c = via_cfg.reset("train", cases)
    assert torch.equal(r_c, r_d) and torch.equal(h_c, h_d) and via_cfg._scene_cache == {}
    assert torch.equal(via_cfg.humans, sim.humans) and torch.equal(via_cfg.human_goals, sim.human_goals)
    with pytest.raises(ValueError):
        sim.reset("train", cases, generator="gpu")


class _Target(object):
    name = "ModelPredictiveRL"


def _explore(dev, cfg_kw, generator):
    from relationalgraphlearning_amd import ReplayMemory, VectorExplorer
    from relationalgraphlearning_amd.orca import OrcaPolicy
    mem = ReplayMemory(100000)
    sim = BatchedCrowdSim(dev, SimConfig(scene_generator=generator, **cfg_kw), human_policy="orca")
    ex = VectorExplorer(sim, OrcaPolicy(safety_space=0.15), memory=mem, gamma=0.9, target_policy=_Target())
    ex.run_k_episodes(64, "train", update_memory=True, imitation_learning=True)
    return ex, mem


def test_vector_explorer_square_crossing_is_identical_with_either_generator(dev):
    kw = dict(scenario="square_crossing", human_num=4)
    (ex_h, mem_h), (ex_d, mem_d) = _explore(dev, kw, "host"), _explore(dev, kw, "device")
    assert ex_d.sim._scene_cache == {} and len(ex_h.sim._scene_cache) == 64
    assert ex_h.last_run["case"] == ex_d.last_run["case"] == list(range(64))
    assert ex_h.last_run["outcome"] == ex_d.last_run["outcome"] and ex_h.last_run["length"] == ex_d.last_run["length"]
    assert ex_h.last_run["actions"] == ex_d.last_run["actions"]
    assert len(mem_h) == len(mem_d) > 0
    for a, b in zip(mem_h.memory, mem_d.memory):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_vector_explorer_circle_crossing_agrees_between_generators(dev):
    kw = dict(scenario="circle_crossing", human_num=5)
    (ex_h, mem_h), (ex_d, mem_d) = _explore(dev, kw, "host"), _explore(dev, kw, "device")
    assert ex_h.last_run["outcome"] == ex_d.last_run["outcome"] and ex_h.last_run["length"] == ex_d.last_run["length"]
    assert len(mem_h) == len(mem_d) > 0
    cfg, first = ex_h.sim.cfg, 0
    for outcome, length in zip(ex_h.last_run["outcome"], ex_h.last_run["length"]):
        if outcome in (2, 3):                         # stored episodes, length - 1 items each: compare each one's first state
            if length > 1:
                a, b = mem_h[first], mem_d[first]
                assert _f32_close(a[0], b[0], cfg) and _f32_close(a[1], b[1], cfg)
            first += length - 1
    assert first == len(mem_h)


def test_the_attempt_cap_flags_exactly_the_cases_the_restatement_flags(dev):
    cap, cases = 300, list(range(8))                  # 600 to 1 800 draws a case (at most 15 * (2 + 3 * 300)); case 6 is placed
    cfg = SimConfig(scenario="circle_crossing", human_num=15, randomize_attributes=True, scene_max_attempts=cap)
    want = [sg.generate_scene_restated(cfg, "test", k, max_attempts=cap)[4] for k in cases]
    flagged = [k for k, st in zip(cases, want) if st["status"]]
    assert flagged and len(flagged) < len(cases), flagged           # the cap is exercised and so is the comparison
    with pytest.raises(UnplacedSceneError) as e:
        generate_scenes_device(cfg, "test", cases, dev)
    assert e.value.cases == [("test", k) for k in flagged]
    assert str(flagged) in str(e.value) and "circle_crossing" in str(e.value) and "scene_max_attempts = 300" in str(e.value)
    with pytest.raises(UnplacedSceneError):
        BatchedCrowdSim(dev, cfg).reset("test", cases, generator="device")
    keep = [k for k in cases if k not in flagged]
    robot, humans, goals, vpref, status, draws = (t.cpu().numpy() for t in generate_scenes_device(cfg, "test", keep, dev))
    assert int(status.sum()) == 0
    for b, k in enumerate(keep):
        host = sg.host_scene_with_draws(cfg, "test", k)            # finishes: it makes the draws the restatement made
        assert draws[b] == host[4] == want[cases.index(k)]["draws"]
        _compare("circle-H15-rand", cfg, host[:4], (robot[b], humans[b], goals[b], vpref[b]), ("test", k))


def test_unplaced_cases_can_go_to_the_host_generator(dev):
    base = SimConfig(scenario="circle_crossing", human_num=19)
    cases = list(range(6))
    need = [sg.generate_scene_restated(base, "test", k)[4]["max_attempts"] for k in cases]
    cap = sorted(need)[len(need) // 2] - 1            # below some cases' attempt maximum, not below every one's
    cfg = SimConfig(scenario="circle_crossing", human_num=19, scene_max_attempts=cap)
    flagged = [k for k, m in zip(cases, need) if m > cap]
    assert cap >= 1 and 0 < len(flagged) < len(cases)
    with pytest.raises(UnplacedSceneError) as e:
        generate_scenes_device(cfg, "test", cases, dev)
    assert e.value.cases == [("test", k) for k in flagged]
    robot, humans, goals, vpref, status, _ = (t.cpu().numpy() for t in generate_scenes_device(cfg, "test", cases, dev, on_unplaced="host"))
    assert [k for k, s in zip(cases, status) if s] == flagged
    for b, k in enumerate(cases):
        host = generate_scene(base, "test", k)
        if k in flagged:                              # the host's own arrays
            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(host, (robot[b], humans[b], goals[b], vpref[b])))
        else:
            _compare("circle-H19-fixed", cfg, host, (robot[b], humans[b], goals[b], vpref[b]), ("test", k))
