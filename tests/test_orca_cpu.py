"""ORCA without a GPU: properties of the float32 restatement (tests/orca_cpu.py) that the device kernel is held to bit for bit,
hand cases, the reference's wrapper semantics recorded in tests/golden/orca.npz, the fixture's generator, and the host-side
argument checks of crowd_orca_humans_f64 / crowd_orca_robot_f64."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from relationalgraphlearning_amd import _native as nat
from tests import golden_io as gio
from tests import orca_cpu as oc
from tests.golden import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def random_agent_set(rng, kind):
    """(pos, vel, radius float32 lists, pref, max_speed) with agent 0 the one under test."""
    n = {"sparse": rng.randint(2, 6), "crowd": rng.randint(12, 25), "collide": rng.randint(2, 8),
         "infeasible": rng.randint(6, 14)}[kind]
    spread = {"sparse": 4.0, "crowd": 3.0, "collide": 0.9, "infeasible": 1.6}[kind]
    p = rng.uniform(-spread, spread, (n, 2))
    v = rng.uniform(-1.2, 1.2, (n, 2))
    if kind == "infeasible":                     # a ring closing in on agent 0 from every side
        ang = np.linspace(0, 2 * np.pi, n - 1, endpoint=False) + rng.uniform(0, 1)
        d = rng.uniform(0.7, 1.2, n - 1)
        p[1:] = np.stack([np.cos(ang), np.sin(ang)], 1) * d[:, None]
        p[0] = 0
        v[1:] = -np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(0.5, 1.5, (n - 1, 1))
    r = rng.uniform(0.2, 0.45, n)
    pos = [oc.v2(*x) for x in p]
    vel = [oc.v2(*x) for x in v]
    rad = [f32(x) for x in r]
    pref = oc.v2(*rng.uniform(-1.5, 1.5, 2))
    max_speed = f32(rng.choice([1.0, rng.uniform(0.3, 1.5)]))
    return pos, vel, rad, pref, max_speed


def violations(lines, pts):
    """Signed distance beyond each half-plane (> 0: violated) for points pts (M,2), float64: (M, lines)."""
    P = np.array([[float(l[0][0]), float(l[0][1])] for l in lines])
    D = np.array([[float(l[1][0]), float(l[1][1])] for l in lines])
    diff = P[None, :, :] - pts[:, None, :]
    return D[None, :, 0] * diff[:, :, 1] - D[None, :, 1] * diff[:, :, 0]


def test_restatement_properties_on_random_agent_sets():
    rng = np.random.RandomState(7)
    kinds = ["sparse"] * 600 + ["crowd"] * 500 + ["collide"] * 500 + ["infeasible"] * 400
    seen = {"lp3": 0, "cutoff": 0, "left": 0, "right": 0, "collision": 0, "full": 0}
    for kind in kinds:
        pos, vel, rad, pref, ms = random_agent_set(rng, kind)
        info = {}
        v = oc.new_velocity(pos, vel, rad, 0, pref, ms, 0.25, 10.0, 10, 5.0, info)
        for b in info["branches"]:
            seen[b] += 1
        seen["full"] += len(info["neighbours"]) == 10 and len(pos) > 11
        vv = np.array([float(v[0]), float(v[1])])
        m = float(ms)
        ang = rng.uniform(0, 2 * np.pi, 3000)
        rad_s = m * np.sqrt(rng.uniform(0, 1, 3000))
        samples = np.stack([rad_s * np.cos(ang), rad_s * np.sin(ang)], 1)
        if not info["lines"]:
            continue
        viol_v = violations(info["lines"], vv[None])[0]
        viol_s = violations(info["lines"], samples)
        if not info["lp3"]:
            assert viol_v.max() <= 1e-5, (kind, viol_v.max())
            assert np.hypot(*vv) <= m + 1e-6
            feasible = samples[(viol_s <= 0).all(1)]
            pr = np.array([float(pref[0]), float(pref[1])])
            if len(feasible):
                assert np.hypot(*(feasible - pr).T).min() >= np.hypot(*(vv - pr)) - 1e-5, kind
        else:
            seen["lp3"] += 1
            # (no speed bound here: a projected line of two nearly parallel lines can lie far outside the disk, and in float32
            # such a line's circle intersection is only as good as the cancellation in its discriminant -- RVO2's own numerics)
            assert max(viol_v.max(), 0.0) <= np.maximum(viol_s.max(1), 0.0).min() + 1e-5, kind
    assert all(c > 20 for c in seen.values()), seen       # every branch, full neighbour lists and LP3 were exercised


def test_no_neighbours_returns_the_clipped_preferred_velocity():
    pos, vel, rad = [oc.v2(0, 0), oc.v2(30, 0)], [oc.v2(0.3, 0), oc.v2(0, 0)], [f32(0.31), f32(0.31)]
    inside = oc.v2(0.3, -0.4)
    assert oc.new_velocity(pos, vel, rad, 0, inside, f32(1), 0.25) == inside          # the other agent is beyond neighbor_dist
    far = oc.v2(3.0, 4.0)
    v = oc.new_velocity(pos, vel, rad, 0, far, f32(1), 0.25)
    assert v == oc.scale(f32(1), oc.normalize(far)) and abs(np.hypot(float(v[0]), float(v[1])) - 1) < 1e-6
    assert oc.new_velocity(pos[:1], vel[:1], rad[:1], 0, far, f32(2), 0.25) == oc.scale(f32(2), oc.normalize(far))


def test_symmetric_head_on_pair_gives_mirrored_velocities():
    pos, vel, rad = [oc.v2(-2, 0.1), oc.v2(2, -0.1)], [oc.v2(1, 0), oc.v2(-1, 0)], [f32(0.31), f32(0.31)]
    v0 = oc.new_velocity(pos, vel, rad, 0, oc.v2(1, 0), f32(1), 0.25)
    v1 = oc.new_velocity(pos, vel, rad, 1, oc.v2(-1, 0), f32(1), 0.25)
    assert v0 == (-v1[0], -v1[1])
    assert v0 != oc.v2(1, 0) and float(v0[1]) != 0.0           # they swerve instead of walking into each other


def orca_cases():
    return [str(c).split("|") for c in gio.load("orca")["orca_cases"]]


@pytest.mark.parametrize("case", orca_cases(), ids=lambda c: c[0])
def test_fixture_velocities_follow_the_entry_points_semantics(case):
    """Every recorded step: the restatement, assembled as crowd_orca_humans_f64 / crowd_orca_robot_f64 assemble the agents,
    gives the velocities the reference's CrowdSim got from its (r)vo2 wrapper -- agent order, radii, preferred velocities,
    visibility, `[:-1]` and max_speed are the entry points'."""
    g = gio.load("orca")
    tag, visible, centralized, driver, safety = case[0], case[5] == "1", case[6] == "1", case[8], float(case[9])
    k = "orca.%s." % tag
    R, Hs = g[k + "robot"], g[k + "humans"]
    for i in range(len(g[k + "info"])):
        hv = oc.humans_velocities(R[i], Hs[i][:, :5], Hs[i][:, 5:7], Hs[i][:, 7], visible, centralized=centralized)
        assert np.array_equal(hv, g[k + "human_vel"][i]), (tag, i)
        if driver == "orca":
            rv = oc.robot_velocity(R[i], Hs[i][:, :5], safety_space=safety)
            assert np.array_equal(rv, g[k + "robot_vel"][i]), (tag, i)


@pytest.mark.reference
@pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the upstream reference")
def test_fixture_generator_reproduces_orca_npz(tmp_path):
    out = str(tmp_path / "orca.npz")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_orca.py"), out], check=True, env=env,
                   cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    new, old = dict(np.load(out)), gio.load("orca")
    assert set(new) == set(old)
    for name in old:
        assert new[name].dtype == old[name].dtype and np.array_equal(new[name], old[name]), name


def test_orca_params_layout_and_defaults():
    assert ctypes.sizeof(nat.CrowdOrcaParams) == 4 * 8 + 3 * 4 + 4          # 4 B tail padding to the double alignment
    from relationalgraphlearning_amd.orca import OrcaParams, ORCA, CentralizedORCA, register
    p = OrcaParams().native()
    assert (p.time_step, p.neighbor_dist, p.time_horizon, p.safety_space, p.max_neighbors, p.max_speed_rule) == (0.25, 10, 5, 0, 10, 0)
    assert OrcaParams().native(centralized=False).max_speed_rule == 1
    o = ORCA()
    for name, val in (("name", "ORCA"), ("trainable", False), ("multiagent_training", True), ("kinematics", "holonomic"),
                      ("safety_space", 0), ("neighbor_dist", 10), ("max_neighbors", 10), ("time_horizon", 5),
                      ("time_horizon_obst", 5), ("radius", 0.3), ("max_speed", 1), ("time_step", None)):
        assert getattr(o, name) == val, name
    factory = {"orca": None}
    register(factory)
    assert factory["orca"] is ORCA and factory["centralized_orca"] is CentralizedORCA


def test_host_argument_checks_of_the_orca_entry_points():
    lib = nat.lib()
    p = nat.CrowdOrcaParams(0.25, 10.0, 5.0, 0.0, 10, 0, 0)
    fake = ctypes.c_void_p(0x1000)              # never dereferenced: every call below fails its host checks before a launch
    hum = lib.crowd_orca_humans_f64
    rob = lib.crowd_orca_robot_f64
    assert hum(None, fake, fake, fake, None, None, 4, 5, 0, fake, None) == -3
    assert hum(ctypes.byref(p), None, fake, fake, None, None, 4, 5, 0, fake, None) == -3
    assert hum(ctypes.byref(p), fake, fake, None, None, None, 4, 5, 0, fake, None) == -3
    assert hum(ctypes.byref(p), fake, fake, fake, None, None, 4, 5, 0, None, None) == -3
    assert hum(ctypes.byref(p), fake, fake, fake, None, None, 0, 5, 0, fake, None) == -1
    assert hum(ctypes.byref(p), fake, fake, fake, None, None, 4, 0, 0, fake, None) == -1
    assert rob(None, fake, fake, None, 4, 5, fake, None) == -3
    assert rob(ctypes.byref(p), fake, None, None, 4, 5, fake, None) == -3
    assert rob(ctypes.byref(p), fake, fake, None, 4, 5, None, None) == -3
    assert rob(ctypes.byref(p), fake, fake, None, 0, 5, fake, None) == -1
    assert rob(ctypes.byref(p), fake, fake, None, 4, 0, fake, None) == -1
    for bad in (-1, nat.CROWD_ORCA_MAX_NEIGHBORS + 1):
        q = nat.CrowdOrcaParams(0.25, 10.0, 5.0, 0.0, bad, 0, 0)
        assert hum(ctypes.byref(q), fake, fake, fake, None, None, 4, 5, 0, fake, None) == -1
        assert rob(ctypes.byref(q), fake, fake, None, 4, 5, fake, None) == -1
    q = nat.CrowdOrcaParams(0.25, 10.0, 5.0, 0.0, 10, 1, 0)           # decentralized: v_pref is each human's max_speed
    assert hum(ctypes.byref(q), fake, fake, fake, None, None, 4, 5, 0, fake, None) == -3
    q.max_speed_rule = 2
    assert hum(ctypes.byref(q), fake, fake, fake, fake, None, 4, 5, 0, fake, None) == -2


def test_sim_config_reads_visibility_and_planning_and_orca_refuses_a_unicycle_robot():
    from relationalgraphlearning_amd.sim import SimConfig, BatchedCrowdSim
    from relationalgraphlearning_amd.orca import OrcaPolicy
    c = SimConfig()
    assert c.robot_visible is False and c.centralized_planning is True
    ns = types.SimpleNamespace
    envc = ns(env=ns(time_limit=30, time_step=0.25, randomize_attributes=False),
              reward=ns(success_reward=1, collision_penalty=-0.25, discomfort_dist=0.2, discomfort_penalty_factor=0.5),
              sim=ns(test_scenario="circle_crossing", square_width=20, circle_radius=4, human_num=5, centralized_planning=False),
              humans=ns(radius=0.3, v_pref=1, visible=True), robot=ns(radius=0.3, v_pref=1, visible=True))
    c2 = SimConfig.from_env_config(envc)                         # the reference's EnvConfig attribute names
    assert c2.robot_visible is True and c2.centralized_planning is False
    with pytest.raises(ValueError):
        OrcaPolicy().check_kinematics("unicycle")
    OrcaPolicy().check_kinematics("holonomic")
    BatchedCrowdSim("cpu", human_policy="orca")                # constructible without a device; stepping needs one
    with pytest.raises(ValueError):
        BatchedCrowdSim("cpu", human_policy="socialforce")


def test_docs_no_longer_call_orca_out_of_scope():
    hdr = open(os.path.join(ROOT, "include", "rgl_hip.h")).read()
    sim_src = open(os.path.join(ROOT, "relationalgraphlearning_amd", "sim.py")).read()
    assert "out of scope" not in hdr.split("Batched crowd simulator")[1].split("enum")[0]
    assert "ORCA (external rvo2) is out of scope" not in sim_src
    assert "crowd_orca_humans_f64" in hdr and "orca.register(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
