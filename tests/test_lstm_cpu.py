"""LSTM-RL / OM-LSTM-RL without a GPU: the float64 restatement (tests/lstm_cpu.py) against what upstream recorded in
tests/golden/lstm.npz, the measured bounds, the conditions the GPU tests rely on, the module's state dict, the ABI and the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd import LstmRL, LstmSearch, LstmValueNetwork, register
from relationalgraphlearning_amd.config import policy_config
from relationalgraphlearning_amd.state import FullState, ObservableState, JointState
from tests import lstm_cpu as cpu
from tests import sarl_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cpu.fixture_cases()
LINEAR = 0.25       # |z| below which a gate counts as in its linear range: tanh(z) is within 2 % of z


def _policy(**over):
    pol = LstmRL()
    pol.configure(policy_config("lstm_rl", **over))
    pol.set_phase("test")
    pol.set_device(torch.device("cpu"))
    pol.time_step = cpu.DT
    return pol


def _joint_state(robot, humans):
    return JointState(FullState(*np.asarray(robot).tolist()), [ObservableState(*h) for h in np.asarray(humans).tolist()])


def test_fixture_covers_the_cases_the_issue_names():
    search, net, bulk = cpu.fixture_cases("search"), cpu.fixture_cases("net"), cpu.fixture_cases("bulk")
    assert {(c["H"], c["interact"], c["weights"]) for c in bulk} == {(H, im, w) for H in (5, 20) for im in (True, False)
                                                                     for w in ("plain", "saturated")}
    assert {c["H"] for c in search} >= {1, 2, 5, 20} and {c["kinematics"] for c in search} == {"holonomic", "unicycle"}
    assert {(c["input_dim"], c["interact"]) for c in search} == {(D, im) for D in (13, 29, 45, 61) for im in (True, False)}
    assert {c["weights"] for c in search} == {c["weights"] for c in net} == {"plain", "saturated"}
    for im in (True, False):
        forms = [cpu.case_lengths(cpu.case_arrays(c["idx"])) for c in net if c["interact"] == im]
        assert None in forms                                                             # without lengths
        assert any(f is not None and all(a > b for a, b in zip(f, f[1:])) and f[-1] == 1 for f in forms)     # strictly decreasing H..1
        assert any(f is not None and len(set(f)) == 1 for f in forms)                    # all equal
    assert os.path.getsize(cpu.GOLDEN) < 1 << 20
    assert all(v.dtype.kind in "fiU" for v in cpu.fixture().values())                    # arrays and short tags only


@pytest.mark.parametrize("c", cpu.fixture_cases("search"), ids=[c["tag"] for c in cpu.fixture_cases("search")])
def test_search_restatement_against_upstream(c):
    a = cpu.case_arrays(c["idx"])
    om = cpu.om_of(c["input_dim"])
    sd = cpu.weight_set(c["weights"], c["input_dim"], c["interact"])
    r = cpu.search(a["robot"], a["humans"], c["kinematics"], sd, c["interact"], om)
    assert r["order"].tolist() == a["order"].tolist()                                    # the sort, tie included
    # the rows and maps of the sorted state are the same float32 / float64 operator chains as upstream's: equal, not close
    assert np.array_equal(sarl_cpu.transform(a["robot"], r["humans"], c["kinematics"], om).numpy(), a["transform"])
    assert np.abs(r["action_values"] - a["action_values"]).max() <= cpu.REFERENCE_DEVIATION[c["weights"]]
    assert cpu.gap(a["action_values"]) > 2 * cpu.value_bound(c["weights"]) and r["best"] == int(a["chosen"])
    # the restatement in float32 sums the same terms in another order: the rule the device is held to
    r32 = cpu.search(a["robot"], a["humans"], c["kinematics"], sd, c["interact"], om, dtype=torch.float32)
    assert np.abs(r32["action_values"] - r["action_values"]).max() <= cpu.value_bound(c["weights"]) and r32["best"] == int(a["chosen"])


@pytest.mark.parametrize("c", cpu.fixture_cases("bulk"), ids=[c["tag"] for c in cpu.fixture_cases("bulk")])
def test_bulk_restatement_against_upstream(c):
    """The first roots of the scenes the GPU test searches at B = 40, as upstream searched them: the sort and, where the best two
    action values are more than twice the bound apart, the decision."""
    sd = cpu.weight_set(c["weights"], c["input_dim"], c["interact"])
    batch = cpu.root_batch(cpu.gpu_seed(c["H"], cpu.BULK_B), cpu.BULK_B, c["H"], c["kinematics"])
    vals, best = cpu.batch_search(batch, c["input_dim"], c["interact"], c["weights"])
    roots = cpu.bulk_roots(c)
    assert len(roots) == cpu.BULK_ROOTS and int(cpu.case_arrays(c["idx"])["seed"]) == cpu.gpu_seed(c["H"], cpu.BULK_B)
    for r, a in enumerate(roots):
        assert np.array_equal(a["robot"], batch["robot"][r]) and batch["order"][r].tolist() == a["order"].tolist()
        assert np.abs(vals[r] - a["action_values"]).max() <= cpu.REFERENCE_DEVIATION[c["weights"]]
        assert cpu.gap(vals[r]) <= 2 * cpu.value_bound(c["weights"]) or best[r] == int(a["chosen"])


@pytest.mark.parametrize("c", cpu.fixture_cases("net"), ids=[c["tag"] for c in cpu.fixture_cases("net")])
def test_network_restatement_against_upstream(c):
    a = cpu.case_arrays(c["idx"])
    sd = cpu.weight_set(c["weights"], c["input_dim"], c["interact"])
    lengths = cpu.case_lengths(a)
    v = cpu.value_network(a["rows"], sd, c["interact"], lengths).numpy()
    assert np.abs(v - a["value"]).max() <= cpu.REFERENCE_DEVIATION[c["weights"]]
    if lengths is not None:
        # a sequence cut at length n is the sequence of its first n rows: pack_padded_sequence's hn
        for s, n in enumerate(lengths):
            alone = cpu.value_network(a["rows"][s:s + 1, :n], sd, c["interact"]).numpy()
            assert abs(alone[0] - v[s]) < 1e-12          # float64 products of another batch shape: a few ulps of 0.1 at the most


@pytest.mark.parametrize("weights", ["plain", "saturated"])
def test_reference_deviation_is_what_the_bounds_say(weights):
    """Upstream's own float32 forward (torch CPU) against the float64 restatement over the fixture cases: 3.13e-8 (default
    initialisation) / 2.96e-7 (saturated) on values of magnitude up to 0.2.  The device is allowed four times that.  The error has
    a long tail -- a gate whose pre-activation cancels to the linear range from terms of several hundred -- which is why the fixture
    measures it on the GPU test's own scenes too (its bulk cases: 128 roots, 10 368 values)."""
    dv = cpu.measured_deviation(weights)
    print("%s: upstream float32 stands %.4e from float64" % (weights, dv))
    want = cpu.REFERENCE_DEVIATION[weights]
    assert 0.97 * want <= dv <= want
    assert cpu.value_bound(weights) == 4 * want


def test_sort_is_stable_and_decreasing():
    tie = [c for c in CASES if c["tag"] == "tie"][0]
    a = cpu.case_arrays(tie["idx"])
    d = cpu.distances(a["robot"], a["humans"])
    assert d[1] == d[3] and a["order"].tolist() == [4, 0, 1, 3, 2]                       # upstream keeps 1 in front of 3
    assert cpu.sort_order(a["robot"], a["humans"]) == [4, 0, 1, 3, 2]
    # the same tie in float32: every coordinate of the pair is a small dyadic number
    assert np.array_equal(a["humans"][[1, 3], :2].astype(np.float32).astype(np.float64), a["humans"][[1, 3], :2])
    robot = np.zeros(9)
    humans = np.zeros((6, 5))
    humans[:, 0] = [1, 2, 1, 2, 3, 1]
    assert cpu.sort_order(robot, humans) == [4, 1, 3, 0, 2, 5]


@pytest.mark.parametrize("H", cpu.GPU_H)
def test_gpu_scenes_meet_the_cap_and_the_saturation_conditions(H):
    """For every (seed, B, H, variant, weight set) the GPU search test runs, in float64 alone: at most (B + 19) // 20 roots have
    their best two action values within twice the bound (the GPU test exempts exactly those from the decision check, under the same
    cap), and the saturated set really saturates there -- some gate pre-activations beyond 100, others in the linear range -- while
    the default initialisation stays moderate."""
    for B in sorted(set(cpu.GPU_B)):
        for D, im in cpu.gpu_variants(H):
            batch = cpu.root_batch(cpu.gpu_seed(H, B), B, H, cpu.gpu_kinematics(H, D, im))
            for weights in ("plain", "saturated"):
                ex = {}
                vals, best = cpu.batch_search(batch, D, im, weights, ex)
                assert np.isfinite(vals).all() and (best >= 0).all()
                small = sum(cpu.gap(v) <= 2 * cpu.value_bound(weights) for v in vals)
                assert small <= (B + 19) // 20, (H, B, D, im, weights, small)
                if weights == "saturated":
                    assert ex["max"] > 100 and ex["min"] < LINEAR, (H, B, D, im, ex)
                else:
                    assert ex["max"] < 20, (H, B, D, im, ex)


def test_state_dict_layout_and_round_trip():
    pol = _policy()
    assert pol.name == "LSTM-RL" and pol.input_dim() == 13 and pol.trainable and isinstance(pol.model, LstmValueNetwork)
    want = cpu.weight_set("plain", 13, True)
    sd = pol.model.state_dict()
    assert sorted(sd) == sorted(want) == sorted(cpu.state_dict_keys(True))
    assert all(tuple(sd[k].shape) == tuple(want[k].shape) for k in sd)
    pol.model.load_state_dict(want)
    assert all(torch.equal(pol.get_state_dict()[k], want[k]) for k in want)
    assert isinstance(pol.model.lstm, torch.nn.LSTM) and pol.model.lstm.batch_first
    for over, dim in (({"lstm_rl__with_om": True}, 61), ({"lstm_rl__with_om": True, "om__om_channel_size": 1}, 29),
                      ({"lstm_rl__with_om": True, "om__om_channel_size": 2}, 45)):
        p = _policy(**over)
        assert (p.name, p.input_dim(), p.model.mlp1[0].in_features) == ("LSTM-RL", dim, dim)        # upstream keeps the name with maps
        p1 = _policy(lstm_rl__with_interaction_module=False, **over)
        assert sorted(p1.model.state_dict()) == sorted(cpu.state_dict_keys(False))
        assert tuple(p1.model.lstm.weight_ih_l0.shape) == (200, dim)
        p1.model.load_state_dict(cpu.weight_set("saturated", dim, False))
    assert register({})["lstm_rl"] is LstmRL and LstmSearch.__name__ == "LstmSearch"
    bag = policy_config("lstm_rl").lstm_rl
    assert (bag.global_state_dim, bag.mlp1_dims, bag.mlp2_dims, bag.multiagent_training, bag.with_om, bag.with_interaction_module) == \
        (50, [150, 100, 100, 50], [150, 100, 100, 1], True, False, True)


def _fake_planner(D=61, interact=True, hidden=50, head=(56, 150, 100, 100, 1), mlp1=None, mode="f32"):
    """An LstmPlanner whose device pointers are the address 64: enough for the library's host-side checks, which read none."""
    def desc(dims):
        m = nat.RglMlp()
        m.n_layers = len(dims) - 1
        for l, d in enumerate(dims):
            m.dims[l] = d
        for l in range(len(dims) - 1):
            m.weight[l] = m.bias[l] = 64
        return m
    pl = nat.LstmPlanner()
    pl.mlp1 = desc(mlp1 or (D, 150, 100, 100, 50))
    pl.mlp = desc(head)
    pl.weight_ih = pl.weight_hh = pl.bias_ih = pl.bias_hh = 64
    pl.with_interaction_module, pl.lstm_hidden_dim = int(interact), hidden
    pl.om_channel_size, pl.cell_num, pl.cell_size = (D - 13) // 16, 4, 1.0
    pl.kinematics, pl.num_actions, pl.contraction_dtype = 0, 81, nat.CONTRACTION_DTYPES[mode]
    pl.time_step, pl.gamma, pl.actions = 0.25, 0.9, 64
    return pl


def test_abi_declares_the_lstm_entry_points():
    hdr = open(os.path.join(ROOT, "include", "rgl_hip.h")).read()
    names = {"lstm_value_workspace_bytes", "lstm_value_f32", "lstm_predict_workspace_bytes", "lstm_predict_f32"}
    assert names <= set(nat.SIGNATURES) and names <= set(nat.ADDITIVE)
    assert names <= set(re.findall(r"^\s*(?:int|size_t)\s+(\w+)\s*\(", hdr, flags=re.M))
    assert nat.ABI_VERSION == 8 and int(re.search(r"#define RGL_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert nat.lib().rgl_abi_version() == 8
    mlp = ctypes.sizeof(nat.RglMlp)
    assert ctypes.sizeof(nat.LstmPlanner) == 2 * mlp + 4 * 8 + 4 * 4 + 8 + 4 * 4 + 3 * 8
    handle = ctypes.CDLL(nat.LIB_PATH)
    assert all(hasattr(handle, n) for n in names)
    import relationalgraphlearning_amd as pkg
    assert {"LstmValueNetwork", "LstmRL", "LstmSearch"} <= set(pkg.__all__)


def test_library_refusals_before_any_launch():
    """Everything here is decided on the host: no call below reaches a launch (the planners' pointers are not device memory)."""
    lib = nat.lib()
    by = ctypes.byref
    assert lib.lstm_value_workspace_bytes(by(nat.LstmPlanner())) == 0 and lib.lstm_predict_workspace_bytes(by(nat.LstmPlanner()), 1, 5) == 0
    assert lib.lstm_predict_f32(None, None, None, None, None, 1, 5, None, 0, None, None, None, None, None) == -3
    for D in (13, 29, 45, 61):
        for im in (True, False):
            pl = _fake_planner(D, im)
            need = lib.lstm_value_workspace_bytes(by(pl))
            assert need > 0
            assert lib.lstm_predict_workspace_bytes(by(pl), 2, 127) > need
            assert lib.lstm_predict_workspace_bytes(by(pl), 2, 128) == 0                            # H = 128
            assert (lib.lstm_predict_workspace_bytes(by(pl), 2, 1) == 0) == (D != 13)               # maps with a single human
            assert lib.lstm_value_f32(by(pl), 64, None, None, None, None, 5, 128, D, 1, 64, need, 64, None) == -1
            assert lib.lstm_value_f32(by(pl), 64, None, None, None, None, 5, 0, D, 1, 64, need, 64, None) == -1
            assert lib.lstm_value_f32(by(pl), 64, None, None, None, None, 5, 3, D + 16, 1, 64, need, 64, None) == -1     # not the planner's D
            assert lib.lstm_value_f32(by(pl), 64, None, None, None, None, 5, 3, D, 1, 64, need - 1, 64, None) == -4      # RGL_ERR_WORKSPACE
            assert lib.lstm_value_f32(by(pl), None, 64, None, None, None, 5, 3, D, 1, 64, need, 64, None) == -3          # no hum7
            assert lib.lstm_value_f32(by(pl), None, 64, 64, 64, None, 6, 3, D, 4, 64, need, 64, None) == -1              # 6 scenes, 4 per root
            short = lib.lstm_predict_workspace_bytes(by(pl), 2, 5) - 1
            assert lib.lstm_predict_f32(by(pl), 64, 64, None, None, 2, 5, 64, short, 64, 64, None, None, None) == -4
    # shapes outside the list
    assert lib.lstm_value_workspace_bytes(by(_fake_planner(hidden=64))) == 0
    assert lib.lstm_value_workspace_bytes(by(_fake_planner(head=(56, 150, 100, 1)))) == 0
    assert lib.lstm_value_workspace_bytes(by(_fake_planner(head=(56, 128, 100, 100, 1)))) == 0
    assert lib.lstm_value_workspace_bytes(by(_fake_planner(mlp1=(61, 150, 100, 100, 64)))) == 0
    assert lib.lstm_value_workspace_bytes(by(_fake_planner(interact=False, mlp1=(61, 150, 100, 100, 64)))) > 0     # mlp1 is not read
    wide = _fake_planner()
    wide.cell_num = 5                                                                               # D = 88
    assert lib.lstm_value_workspace_bytes(by(wide)) == 0
    # f32 only: any other contraction mode is RGL_ERR_BAD_MODE, as for SARL
    for mode in ("f16", "bf16x6"):
        pl = _fake_planner(mode=mode)
        assert lib.lstm_value_workspace_bytes(by(pl)) == 0
        assert lib.lstm_value_f32(by(pl), 64, None, None, None, None, 5, 3, 61, 1, 64, 1 << 20, 64, None) == -2
        assert lib.lstm_predict_f32(by(pl), 64, 64, None, None, 2, 5, 64, 1 << 24, 64, 64, None, None, None) == -2
    with pytest.raises(ValueError, match="f32"):
        LstmSearch(None, np.zeros((81, 2)), contraction_dtype="bf16x6")


def test_refusals():
    pol = _policy(lstm_rl__with_om=True)
    pol.build_action_space(1.0)
    robot, humans = cpu.scenes(3, 1, 1)
    with pytest.raises(ValueError):                         # H = 1 with maps: upstream's np.concatenate, on the host
        pol.predict(_joint_state(robot[0], humans[0]))
    with pytest.raises(ValueError):
        pol.build_occupancy_maps(_joint_state(robot[0], humans[0]).human_states)
    robot, humans = cpu.scenes(3, 1, 3)
    three = _joint_state(robot[0], humans[0])
    pol.query_env = True
    with pytest.raises(NotImplementedError, match="query_env"):
        pol.predict(three)
    with pytest.raises(NotImplementedError, match="query_env"):
        pol.predict_batch(torch.zeros(1, 9), torch.zeros(1, 3, 5))
    pol.query_env = False
    # predict sorts the humans in place before anything else, as upstream does
    assert [cpu.distances(robot[0], [[h.px, h.py]])[0] for h in three.human_states] == sorted(cpu.distances(robot[0], humans[0]), reverse=True)
    # an empty crowd goes to the greedy action
    assert pol.predict(JointState(three.robot_state, [])) in pol.action_space
    with pytest.raises(AttributeError):
        pol.get_matrix_A()
    # lengths: every entry in 1..H, non-increasing, one per sequence -- checked on the host, before the device is asked for anything
    rows = torch.zeros(3, 4, 61)
    for bad in ([4, 3], [4, 3, 0], [5, 4, 3], [3, 4, 4], torch.tensor([4, 2, 3])):
        with torch.no_grad(), pytest.raises(ValueError):
            pol.model((rows, bad))
    with torch.no_grad(), pytest.raises(ValueError):
        pol.model(torch.zeros(3, 4, 13))                    # not this network's row width
    # grad mode: no silent autograd (checked before the device is asked for anything)
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="training is not provided"):
        pol.model(rows)
    with pytest.raises(nat.NativeLibraryError):             # and no CPU path
        with torch.no_grad():
            pol.model((rows, [4, 4, 2]))
    # training is the next step: the explorer names what is missing
    from relationalgraphlearning_amd.vector_explorer import VectorExplorer
    ex = VectorExplorer(None, pol, device=torch.device("cpu"), target_policy=pol)
    with pytest.raises(NotImplementedError, match="LSTM-RL training"):
        ex.run_k_episodes(1, "train", update_memory=True)
