"""SARL / OM-SARL without a GPU: the float64 restatement (tests/sarl_cpu.py) against what upstream recorded in
tests/golden/sarl.npz, the conditions the GPU tests rely on, the module's state dict, the ABI and the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd import SARL, SarlValueNetwork, register
from relationalgraphlearning_amd.config import policy_config
from relationalgraphlearning_amd.state import FullState, ObservableState, JointState
from tests import sarl_cpu as cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cpu.fixture_cases()


def _policy(**over):
    pol = SARL()
    pol.configure(policy_config("sarl", **over))
    pol.set_phase("test")
    pol.set_device(torch.device("cpu"))
    pol.time_step = cpu.DT
    return pol


def test_fixture_covers_the_cases_the_issue_names():
    assert {c["H"] for c in CASES} >= {2, 5, 7, 20} and {c["kinematics"] for c in CASES} == {"holonomic", "unicycle"}
    assert {c["input_dim"] for c in CASES} == {13, 29, 45, 61} and {c["with_global_state"] for c in CASES} == {True, False}
    assert {c["weights"] for c in CASES} == {"plain", "sharp"}
    tags = {c["tag"] for c in CASES}
    assert {"resting", "shared", "outside"} <= tags
    resting = cpu.case_arrays([c for c in CASES if c["tag"] == "resting"][0]["idx"])["humans"]
    assert (resting[1, 2:4] == 0).all()
    assert str(cpu.fixture()["single_human_error"]) == "ValueError"
    assert os.path.getsize(cpu.GOLDEN) < 1 << 20


@pytest.mark.parametrize("c", CASES, ids=[c["tag"] for c in CASES])
def test_restatement_against_upstream(c):
    a = cpu.case_arrays(c["idx"])
    om = cpu.om_of(c["input_dim"])
    sd = cpu.weight_set(c["weights"], c["input_dim"], c["with_global_state"])
    # the rows and maps are the same float32 / float64 operator chains as upstream's: equal, not close
    assert np.array_equal(cpu.transform(a["robot"], a["humans"], c["kinematics"], om).numpy(), a["transform"])
    r = cpu.search(a["robot"], a["humans"], c["kinematics"], sd, c["with_global_state"], om)
    if om is not None:
        assert np.array_equal(r["maps"], a["maps_next"])
    # upstream's float32 network against float64: within the deviation the bounds are built from (pinned below)
    dv, da = cpu.REFERENCE_DEVIATION[c["weights"]]
    assert np.abs(r["action_values"] - a["action_values"]).max() <= dv
    assert r["best"] == int(a["chosen"])
    assert np.abs(r["attention"][r["best"]] - a["attention"]).max() <= da
    assert abs(float(a["attention"].sum()) - 1) < 1e-6
    # the restatement in float32 sums the same terms in another order (all 81 actions in one product): the rule the device is held to
    r32 = cpu.search(a["robot"], a["humans"], c["kinematics"], sd, c["with_global_state"], om, dtype=torch.float32)
    assert np.abs(r32["action_values"] - r["action_values"]).max() <= cpu.value_bound(c["weights"]) and r32["best"] == int(a["chosen"])


@pytest.mark.parametrize("weights", ["plain", "sharp"])
def test_reference_deviation_is_what_the_bounds_say(weights):
    """Upstream's own float32 forward against the float64 restatement over the fixture cases: 2.55e-8 / 2.36e-8 on the action values
    (|V| up to 0.28), 2.40e-8 / 6.51e-7 on the attention weights (default / sharp).  The device is allowed four times that."""
    dv, da = cpu.measured_deviation(weights)
    want_v, want_a = cpu.REFERENCE_DEVIATION[weights]
    assert 0.97 * want_v <= dv <= want_v and 0.97 * want_a <= da <= want_a
    assert cpu.value_bound(weights) == 4 * want_v and cpu.attention_bound(weights) == 4 * want_a


def test_no_fixture_coordinate_sits_on_a_cell_boundary():
    for c in CASES:
        if c["input_dim"] == 13:
            continue
        a = cpu.case_arrays(c["idx"])
        for humans in (a["humans"], cpu.propagate_humans(a["humans"])):
            coords = []
            cpu.occupancy_maps(humans, *cpu.om_of(c["input_dim"]), coords=coords)
            coords = np.asarray(coords)
            assert np.abs(coords - np.round(coords)).min() > 1e-9


def test_map_quirks():
    # humans 1 and 2 share cell (2, 2) = 10 of human 0's grid
    c = [c for c in CASES if c["tag"] == "shared"][0]
    humans = cpu.propagate_humans(cpu.case_arrays(c["idx"])["humans"])
    m3 = cpu.occupancy_maps(humans, 4, 1.0, 3)
    assert m3.shape == (5, 48) and (m3[:, 33:] == 0).all() and m3[0, 20] != 0            # slots above 2 * 15 + 2 stay zero
    m2 = cpu.occupancy_maps(humans, 4, 1.0, 2)
    # two channels, slot 20 = the mean vx of the two humans in cell 10: both move as human 0 does, 0.5 along its heading
    assert m2.shape == (5, 32) and abs(m2[0, 20] - 0.5) < 1e-7 and abs(m2[0, 21]) < 1e-7
    m1 = cpu.occupancy_maps(humans, 4, 1.0, 1)
    assert set(np.unique(m1)) <= {0.0, 1.0} and m1[0, 10] == 1.0
    # three channels: the cells k and k + 1 share slot 2k + 2 -- a vy averaged with a 1
    h = np.array([[0.0, 0.0, 1.0, 0.0, 0.3], [0.5, 0.5, 0.0, 0.5, 0.3], [1.5, 0.5, 0.0, 0.0, 0.3]])
    m = cpu.occupancy_maps(h, 4, 1.0, 3)           # human 1 in cell 10 (vy 0.5), human 2 in cell 11
    assert m[0, 20] == 1.0 and m[0, 22] == np.float32((0.5 + 1.0) / 2)
    out = [c for c in CASES if c["tag"] == "outside"][0]
    mo = cpu.occupancy_maps(cpu.case_arrays(out["idx"])["humans"], 4, 1.0, 3)
    assert (mo[3] == 0).all() and (mo[4] == 0).all()                                    # nobody inside the far humans' grids
    with pytest.raises(ValueError):
        cpu.occupancy_maps(h[:1], 4, 1.0, 3)


def test_sharp_weights_spread_the_attention():
    sharp = [cpu.case_arrays(c["idx"])["attention"] for c in CASES if c["weights"] == "sharp"]
    assert any(a.max() > 0.5 for a in sharp) and any(a.min() < 0.05 for a in sharp)


@pytest.mark.parametrize("weights", ["plain", "sharp"])
@pytest.mark.parametrize("H", [2, 5, 7, 20])
def test_gaps_of_the_gpu_scenes_exceed_the_bound(H, weights):
    """The GPU test compares decisions where best and second action are more than twice the value bound apart; at most one root in
    twenty may fall below the bound itself.  Checked here in float64 for a SAMPLE of what the GPU test runs: the first twenty roots
    of its B = 40 seed per H, both weight sets, input_dim 61 with the global state.  Its other seeds (B = 1, 3, 64 and the large
    launches) and variants are not replayed on the CPU -- a root costs 81 python-built scenes here; for those the GPU test's own
    count of left-out roots, taken on float64 values of the device's rows, is the assertion."""
    sd = cpu.weight_set(weights, 61, True)
    B = 20
    kin = "unicycle" if (H + 61) % 2 else "holonomic"
    robot, humans = cpu.scenes(1000 * H + 40, 40, H, kin)
    small = sum(cpu.gap(cpu.search(robot[b], humans[b], kin, sd, True, cpu.om_of(61))["action_values"]) < cpu.value_bound(weights)
                for b in range(B))
    assert small <= 1


def test_state_dict_layout_and_round_trip():
    pol = _policy()
    assert pol.name == "OM-SARL" and pol.input_dim() == 61 and pol.trainable
    sd = pol.model.state_dict()
    want = cpu.weight_set("plain")
    assert list(sd) == list(want) and all(tuple(sd[k].shape) == tuple(want[k].shape) for k in sd)
    pol.model.load_state_dict(want)
    assert all(torch.equal(pol.get_state_dict()[k], want[k]) for k in want)
    for over, name, dim in (({"sarl__with_om": False}, "SARL", 13), ({"om__om_channel_size": 1}, "OM-SARL", 29),
                            ({"om__om_channel_size": 2}, "OM-SARL", 45)):
        p = _policy(**over)
        assert (p.name, p.input_dim(), p.model.mlp1[0].in_features) == (name, dim, dim)
    assert _policy(sarl__with_global_state=False).model.attention[0].in_features == 100
    assert isinstance(pol.model, SarlValueNetwork) and register({})["sarl"] is SARL


def test_abi_declares_the_sarl_entry_points():
    hdr = open(os.path.join(ROOT, "include", "rgl_hip.h")).read()
    names = {"sarl_occupancy_maps_f32", "sarl_value_workspace_bytes", "sarl_value_f32", "sarl_predict_workspace_bytes", "sarl_predict_f32"}
    assert names <= set(nat.SIGNATURES) and names <= set(re.findall(r"^\s*(?:int|size_t)\s+(\w+)\s*\(", hdr, flags=re.M))
    assert int(re.search(r"#define RGL_SARL_MAX_HUMANS (\d+)", hdr).group(1)) == nat.SARL_MAX_HUMANS >= 20
    assert nat.ABI_VERSION == 8
    mlp = ctypes.sizeof(nat.RglMlp)
    assert ctypes.sizeof(nat.SarlPlanner) == 4 * mlp + 4 * 4 + 8 + 2 * 4 + 2 * 8 + 3 * 8
    handle = ctypes.CDLL(nat.LIB_PATH)
    assert all(hasattr(handle, n) for n in names)
    # host-side refusals of the library: no device is touched before them
    lib = nat.lib()
    pl = nat.SarlPlanner()
    assert lib.sarl_value_workspace_bytes(ctypes.byref(pl)) == 0 and lib.sarl_predict_workspace_bytes(ctypes.byref(pl), 1, 5) == 0
    assert lib.sarl_predict_f32(None, None, None, 1, 5, None, 0, None, None, None, None, None) == -3
    assert lib.sarl_occupancy_maps_f32(None, 1, 1, 1, 0.0, 4, 1.0, 3, 1, None) == -1          # H = 1: bad shape, nothing launched
    assert lib.sarl_occupancy_maps_f32(None, 1, 1, 2, 0.0, 4, 1.0, 4, 1, None) == -2


def test_refusals():
    pol = _policy()
    pol.build_action_space(1.0)
    robot, humans = cpu.scenes(3, 1, 1)
    one = JointState(FullState(*robot[0].tolist()), [ObservableState(*h) for h in humans[0].tolist()])
    with pytest.raises(ValueError):                         # H = 1 with maps: upstream's np.concatenate, on the host
        pol.predict(one)
    with pytest.raises(ValueError):
        pol.build_occupancy_maps(one.human_states)
    robot, humans = cpu.scenes(3, 1, 3)
    three = JointState(FullState(*robot[0].tolist()), [ObservableState(*h) for h in humans[0].tolist()])
    pol.query_env = True
    with pytest.raises(NotImplementedError, match="query_env"):
        pol.predict(three)
    pol.query_env = False
    # an empty crowd goes to the greedy action and leaves an empty attention list
    action = pol.predict(JointState(three.robot_state, []))
    assert pol.get_attention_weights() == [] and action in pol.action_space
    # grad mode: no silent autograd (checked before the device is asked for anything)
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="training is not provided"):
        pol.model(torch.zeros(1, 3, 61))
    with pytest.raises(nat.NativeLibraryError):             # and no CPU path
        with torch.no_grad():
            pol.model(torch.zeros(1, 3, 61))
    # SARL replay rows are not stored
    from relationalgraphlearning_amd.vector_explorer import VectorExplorer
    ex = VectorExplorer(None, pol, device=torch.device("cpu"), target_policy=pol)
    with pytest.raises(NotImplementedError, match="SARL"):
        ex.run_k_episodes(1, "train", update_memory=True)
