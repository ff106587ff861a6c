"""LSTM-RL / OM-LSTM-RL on the MI355X: the recurrent value networks, the distance sort, the one-step search and the policy around
them, against the float64 restatement of tests/lstm_cpu.py and against what upstream recorded in tests/golden/lstm.npz.

The value bound is not a constant of ours: upstream's own float32 forward (torch CPU, the fixture) stands 3.13e-8 (default
initialisation) / 2.96e-7 (saturated LSTM tensors) from the float64 restatement over the fixture cases (|V| up to 0.2), and the device
-- the same float32 sums in another order, MFMA in blocks of four -- is allowed four times that (lstm_cpu.value_bound;
tests/test_lstm_cpu.py pins the measurement, and shows that the scenes used here leave at most one root in twenty undecided)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import lstm_cpu as cpu
from tests.test_sarl_gpu import device_rows, ulp32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_policy(dev, kinematics, input_dim, interact, weights):
    from relationalgraphlearning_amd import LstmRL
    from relationalgraphlearning_amd.config import policy_config
    om = cpu.om_of(input_dim)
    pol = LstmRL()
    pol.configure(policy_config("lstm_rl", action_space__kinematics=kinematics, lstm_rl__with_om=om is not None,
                                lstm_rl__with_interaction_module=interact, om__om_channel_size=om[2] if om else 3))
    pol.set_phase("test")
    pol.set_device(dev)
    pol.time_step = cpu.DT
    pol.model.load_state_dict({k: v.to(dev) for k, v in cpu.weight_set(weights, input_dim, interact).items()})
    return pol


def joint_state(robot, humans):
    from relationalgraphlearning_amd.state import FullState, ObservableState, JointState
    return JointState(FullState(*np.asarray(robot).tolist()), [ObservableState(*h) for h in np.asarray(humans).tolist()])


def check_search(dev, pol, sd, kin, input_dim, interact, weights, H, B):
    """One search of B roots (humans in their GIVEN order) against float64 on the rows the device prepared from the sorted humans;
    returns (worst deviation, action values, best, order)."""
    om = cpu.om_of(input_dim)
    bound = cpu.value_bound(weights)
    batch = cpu.root_batch(cpu.gpu_seed(H, B), B, H, kin)      # the restatement's sort and rewards, computed once per (H, B)
    robot = batch["robot"]
    search = pol.gcn_search()
    r64, h64 = torch.tensor(robot, device=dev), torch.tensor(batch["humans"], device=dev)
    dev_vals, dev_best = search.search(r64.float(), h64.float(), roots64=(r64, h64))
    vals, best = dev_vals.cpu().numpy().astype(np.float64), dev_best.cpu().numpy()
    best_value = search.last_best_value.cpu().numpy()
    assert np.array_equal(search.last_order.cpu().numpy(), batch["order"])
    rows, reward = device_rows(dev, r64, torch.tensor(batch["humans_sorted"], device=dev), kin, om)
    A = reward.shape[1]
    v64 = cpu.value_network(rows.cpu(), sd, interact).numpy()
    with torch.no_grad():                                                   # the module's forward on the same rows
        v_mod = pol.model(rows).cpu().numpy()[:, 0].astype(np.float64)
    err_mod = np.abs(v_mod - v64).max()
    reward = reward.cpu().numpy()
    decided = [cpu.decide(reward[b], v64[b * A:(b + 1) * A], robot[b, 7]) for b in range(B)]
    want = np.stack([d[0] for d in decided])
    err = np.abs(vals - want).max()
    print("H %d D %d module %d %s B %d: |value - float64| module %.2e search %.2e (bound %.2e)"
          % (H, input_dim, interact, weights, B, err_mod, err, bound))
    assert np.isfinite(vals).all() and np.isfinite(v_mod).all() and err_mod <= bound and err <= bound
    left_out = 0
    for b in range(B):
        idx = decided[b][1]
        if cpu.gap(want[b]) > 2 * bound:
            assert best[b] == idx
            assert best_value[b] == np.float32(vals[b, idx])
        else:
            left_out += 1
    assert left_out <= (B + 19) // 20
    return max(err, err_mod), dev_vals, dev_best, search.last_order


@pytest.mark.parametrize("weights", ["plain", "saturated"])
@pytest.mark.parametrize("H,input_dim,interact", [(H, D, im) for H in cpu.GPU_H for D, im in cpu.gpu_variants(H)])
def test_value_network_and_search_against_float64(dev, monkeypatch, H, input_dim, interact, weights):
    """B = 1 (81 scenes: five tiles and one scene), 3 (a partial last tile), 40, then 3 again through ONE search object, every
    workspace filled with NaN patterns before every call (RGL_DEBUG_POISON_WORKSPACES).  B = 40 is 203 tiles, fewer than the
    workgroups a launch may start, so it runs twice: as it is, and with the grid capped at 37 workgroups (RGL_SARL_GRID_CAP), where
    every workgroup walks five or six tiles, and must give the same bits.  H = 1 is one step (no recurrent product); the saturated set
    at H = 20 is the longest run of gates beyond +-100."""
    monkeypatch.setenv("RGL_DEBUG_POISON_WORKSPACES", "1")
    kin = cpu.gpu_kinematics(H, input_dim, interact)
    pol = make_policy(dev, kin, input_dim, interact, weights)
    sd = cpu.weight_set(weights, input_dim, interact)
    pol.build_action_space(1.0)
    worst = 0.0
    for B in cpu.GPU_B:
        w, vals, best, order = check_search(dev, pol, sd, kin, input_dim, interact, weights, H, B)
        worst = max(worst, w)
        if B == 40:
            monkeypatch.setenv("RGL_SARL_GRID_CAP", "37")
            _, vals2, best2, order2 = check_search(dev, pol, sd, kin, input_dim, interact, weights, H, B)
            monkeypatch.delenv("RGL_SARL_GRID_CAP")
            assert torch.equal(vals, vals2) and torch.equal(best, best2) and torch.equal(order, order2)
    from tests.conftest import PARITY_REPORT
    PARITY_REPORT.append("lstm H %d D %d module %d %s: worst |value - float64| %.2e of %.2e allowed"
                         % (H, input_dim, interact, weights, worst, cpu.value_bound(weights)))


@pytest.mark.parametrize("weights", ["plain", "saturated"])
@pytest.mark.parametrize("interact", [True, False])
def test_lengths(dev, monkeypatch, interact, weights):
    """`lengths` against float64 and against upstream's pack_padded_sequence (the fixture's network cases: none, H..1, all equal),
    then on 243 device-prepared sequences of 20 rows with non-increasing lengths that cross tile borders; all lengths equal to H give
    the bits of no lengths at all."""
    monkeypatch.setenv("RGL_DEBUG_POISON_WORKSPACES", "1")
    bound = cpu.value_bound(weights)
    for c in cpu.fixture_cases("net"):
        if c["interact"] != interact or c["weights"] != weights:
            continue
        a = cpu.case_arrays(c["idx"])
        pol = make_policy(dev, "holonomic", c["input_dim"], interact, weights)
        sd = cpu.weight_set(weights, c["input_dim"], interact)
        rows, lengths = torch.tensor(a["rows"], device=dev), cpu.case_lengths(a)
        with torch.no_grad():
            got = pol.model(rows if lengths is None else (rows, torch.IntTensor(lengths))).cpu().numpy()[:, 0].astype(np.float64)
        v64 = cpu.value_network(a["rows"], sd, interact, lengths).numpy()
        print("%s: |value - float64| %.2e, |value - upstream| %.2e" % (c["tag"], np.abs(got - v64).max(), np.abs(got - a["value"]).max()))
        assert np.isfinite(got).all() and np.abs(got - v64).max() <= bound
        # device and upstream each stand within their share of float64: four parts and one part of the bound
        assert np.abs(got - a["value"]).max() <= 1.25 * bound
        if lengths is not None and len(set(lengths)) == 1:
            with torch.no_grad():
                assert torch.equal(pol.model(rows), pol.model((rows, lengths)))
    H, B, D = 20, 3, 61
    pol = make_policy(dev, "holonomic", D, interact, weights)
    sd = cpu.weight_set(weights, D, interact)
    batch = cpu.root_batch(cpu.gpu_seed(H, B), B, H, "holonomic")
    r64 = torch.tensor(batch["robot"], device=dev)
    rows, _ = device_rows(dev, r64, torch.tensor(batch["humans_sorted"], device=dev), "holonomic", cpu.om_of(D))
    S = rows.shape[0]
    lengths = sorted(np.random.RandomState(5).randint(1, H + 1, S).tolist(), reverse=True)
    assert lengths[0] == H and lengths[-1] == 1 and len(set(lengths[:16])) > 1
    with torch.no_grad():
        got = pol.model((rows, lengths)).cpu().numpy()[:, 0].astype(np.float64)
        same = torch.equal(pol.model(rows), pol.model((rows, torch.full((S,), H, dtype=torch.int32))))
    v64 = cpu.value_network(rows.cpu(), sd, interact, lengths).numpy()
    assert np.isfinite(got).all() and np.abs(got - v64).max() <= bound and same


@pytest.mark.parametrize("interact", [True, False])
def test_saturated_gates_stay_finite(dev, monkeypatch, interact):
    """The saturated set at H = 20: gate pre-activations beyond +-100 (the restatement reports them on the device's own rows) next
    to gates in their linear range.  A sigmoid or tanh written as a quotient of two overflowing exponentials gives NaN here."""
    monkeypatch.setenv("RGL_DEBUG_POISON_WORKSPACES", "1")
    H, B, D = 20, 3, 61
    pol = make_policy(dev, "holonomic", D, interact, "saturated")
    sd = cpu.weight_set("saturated", D, interact)
    batch = cpu.root_batch(cpu.gpu_seed(H, B), B, H, "holonomic")
    r64 = torch.tensor(batch["robot"], device=dev)
    rows, _ = device_rows(dev, r64, torch.tensor(batch["humans_sorted"], device=dev), "holonomic", cpu.om_of(D))
    ex = {}
    v64 = cpu.value_network(rows.cpu(), sd, interact, extremes=ex).numpy()
    assert ex["max"] > 100 and ex["min"] < 0.25
    with torch.no_grad():
        got = pol.model(rows).cpu().numpy()[:, 0].astype(np.float64)
    assert np.isfinite(got).all() and np.abs(got - v64).max() <= cpu.value_bound("saturated")
    # far beyond: rows scaled until e^|z| overflows float32 in every gate that is not exactly zero
    with torch.no_grad():
        far = pol.model(rows * 1e4).cpu().numpy()
    assert np.isfinite(far).all()


def test_a_root_without_a_finite_value_gives_minus_one(dev):
    pol = make_policy(dev, "holonomic", 13, True, "plain")
    pol.build_action_space(1.0)
    robot, humans = cpu.scenes(77, 3, 5)
    robot[1, 7] = np.nan                                    # v_pref: a feature of every row, and the discount's exponent
    r64, h64 = torch.tensor(robot, device=dev), torch.tensor(humans, device=dev)
    search = pol.gcn_search()
    vals, best = search.search(r64.float(), h64.float(), roots64=(r64, h64))
    vals, best = vals.cpu().numpy(), best.cpu().numpy()
    assert np.isnan(vals[1]).all() and best[1] == -1 and search.last_best_value.cpu().numpy()[1] == 0
    assert np.isfinite(vals[[0, 2]]).all() and (best[[0, 2]] >= 0).all()
    assert np.array_equal(search.last_order.cpu().numpy(), np.stack([cpu.sort_order(robot[b], humans[b]) for b in range(3)]))


def test_fixture_cases_through_the_policy(dev):
    for c in cpu.fixture_cases("search"):
        a = cpu.case_arrays(c["idx"])
        om = cpu.om_of(c["input_dim"])
        bound = cpu.value_bound(c["weights"])
        pol = make_policy(dev, c["kinematics"], c["input_dim"], c["interact"], c["weights"])
        js = joint_state(a["robot"], a["humans"])
        given = list(js.human_states)
        action = pol.predict(js)
        # the state is left sorted as upstream leaves it, tie included
        assert [given.index(h) for h in js.human_states] == a["order"].tolist(), c["tag"]
        table = cpu.action_table(c["kinematics"])
        assert tuple(float(x) for x in action) == tuple(table[int(a["chosen"])]), c["tag"]
        dv = np.abs(np.asarray(pol.action_values) - a["action_values"]).max()
        print("%s: |action value - upstream| %.2e" % (c["tag"], dv))
        assert dv <= 1.25 * bound
        assert pol.gcn_search().last_order.cpu().numpy().tolist() == [list(range(c["H"]))]      # predict's own sort came first
        # transform on the sorted state: two float32 evaluations of a cos + b sin, as in tests/test_sarl_gpu.py
        rows = pol.transform(js).cpu().numpy()
        assert rows.shape == a["transform"].shape == (c["H"], c["input_dim"]) and pol.input_dim() == c["input_dim"]
        d = max(float(a["transform"][:, 11].max()), float(a["transform"][0, 0]))
        assert (np.abs(rows[:, :13] - a["transform"][:, :13]) <= 8 * np.spacing(np.float32(d))).all()
        if om is not None:
            want = a["transform"][:, 13:]
            exact = (want == 0) | (want == 1)
            assert np.array_equal(rows[:, 13:][exact], want[exact])
            assert (np.abs(rows[:, 13:].astype(np.float64) - want) <= ulp32(want)).all()
        # predict_batch sorts on the device: the humans in their given order, the same decision
        r64, h64 = torch.tensor(a["robot"][None], device=dev), torch.tensor(a["humans"][None], device=dev)
        best, value = pol.predict_batch(r64.float(), h64.float())
        assert int(best[0]) == int(a["chosen"]) and pol.gcn_search().last_order.cpu().numpy().tolist() == [a["order"].tolist()]
        assert abs(float(value[0]) - a["action_values"][int(a["chosen"])]) <= 1.25 * bound


def test_checkpoint_round_trip(dev, tmp_path):
    for interact in (True, False):
        pol = make_policy(dev, "holonomic", 61, interact, "saturated")
        path = os.path.join(str(tmp_path), "lstm%d.pth" % interact)
        pol.save_model(path)
        assert sorted(torch.load(path)) == sorted(cpu.state_dict_keys(interact))        # upstream's keys
        other = make_policy(dev, "holonomic", 61, interact, "plain")
        robot, humans = cpu.scenes(31, 5, 5)
        r, h = torch.tensor(robot, device=dev).float(), torch.tensor(humans, device=dev).float()
        want_best, want_value = pol.predict_batch(r, h)
        before = other.predict_batch(r, h)[1].clone()
        other.load_model(path)
        best, value = other.predict_batch(r, h)
        assert torch.equal(best, want_best) and torch.equal(value, want_value) and not torch.equal(before, value)


@pytest.mark.parametrize("interact", [True, False])
def test_limits_and_workspace(dev, interact):
    """H = 127 (gcn_prepare_f32's limit), D = 13, B = 1 through the raw ABI on a workspace of exactly the reported size with a guard
    region behind it: the values match float64, the guard keeps its pattern, and one byte less is RGL_ERR_WORKSPACE."""
    from relationalgraphlearning_amd import _native as nat
    from relationalgraphlearning_amd.nets import _stream
    H, B, D = 127, 1, 13
    pol = make_policy(dev, "holonomic", D, interact, "plain")
    pol.build_action_space(1.0)
    sd = cpu.weight_set("plain", D, interact)
    robot, humans = cpu.scenes(9000, B, H)
    order = np.stack([cpu.sort_order(robot[b], humans[b]) for b in range(B)])
    r64, h64 = torch.tensor(robot, device=dev), torch.tensor(humans, device=dev)
    r32, h32 = r64.float(), h64.float()
    lib = nat.lib()
    search = pol.gcn_search()
    GUARD = 4096
    with torch.cuda.device(dev):
        pl = search.planner(dev, H, B)
        need = lib.lstm_predict_workspace_bytes(C.byref(pl), B, H)
        assert need > 0 and lib.lstm_predict_workspace_bytes(C.byref(pl), B, H + 1) == 0
        ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        vals = torch.empty(B, 81, device=dev)
        best = torch.empty(B, dtype=torch.int32, device=dev)
        got_order = torch.empty(B, H, dtype=torch.int32, device=dev)
        args = (C.byref(pl), r32.data_ptr(), h32.data_ptr(), r64.data_ptr(), h64.data_ptr(), B, H, ws.data_ptr())
        tail = (vals.data_ptr(), best.data_ptr(), None, got_order.data_ptr(), _stream())
        assert lib.lstm_predict_f32(*args, need - 1, *tail) == -4
        torch.cuda.synchronize(dev)
        assert bool((ws == 0xA5).all())                                     # the refusal wrote nothing
        nat.check(lib.lstm_predict_f32(*args, need, *tail), "lstm_predict_f32")
        torch.cuda.synchronize(dev)
        assert bool((ws[need:] == 0xA5).all())
        assert np.array_equal(got_order.cpu().numpy(), order)
        rows, reward = device_rows(dev, r64, torch.tensor(np.stack([humans[b][order[b]] for b in range(B)]), device=dev), "holonomic", None)
        v64 = cpu.value_network(rows.cpu(), sd, interact).numpy()
        want, idx = cpu.decide(reward.cpu().numpy()[0], v64, robot[0, 7])
        err = np.abs(vals.cpu().numpy()[0].astype(np.float64) - want).max()
        print("H 127 module %d: |value - float64| %.2e" % (interact, err))
        assert err <= cpu.value_bound("plain")
        assert cpu.gap(want) <= 2 * cpu.value_bound("plain") or int(best[0]) == idx
        # the value call alone: its workspace is the packed weights, whatever S and H
        vneed = lib.lstm_value_workspace_bytes(C.byref(pl))
        vws = torch.full((vneed + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        value = torch.empty(rows.shape[0], device=dev)
        vargs = (C.byref(pl), rows.data_ptr(), None, None, None, None, rows.shape[0], H, D, 1, vws.data_ptr())
        assert lib.lstm_value_f32(*vargs, vneed - 1, value.data_ptr(), _stream()) == -4
        nat.check(lib.lstm_value_f32(*vargs, vneed, value.data_ptr(), _stream()), "lstm_value_f32")
        torch.cuda.synchronize(dev)
        assert bool((vws[vneed:] == 0xA5).all())
        assert np.abs(value.cpu().numpy().astype(np.float64) - v64).max() <= cpu.value_bound("plain")
    robot, humans = cpu.scenes(6, 1, nat.SARL_MAX_HUMANS + 1)
    with pytest.raises(nat.NativeLibraryError, match="BAD_SHAPE"):
        pol.predict_batch(torch.tensor(robot, device=dev).float(), torch.tensor(humans, device=dev).float())
    maps = make_policy(dev, "holonomic", 61, interact, "plain")
    robot, humans = cpu.scenes(5, 2, 1)
    with pytest.raises(ValueError):                                         # maps of a single human: upstream's np.concatenate
        maps.predict_batch(torch.tensor(robot, device=dev).float(), torch.tensor(humans, device=dev).float())
    pol.model.mlp[0].weight.requires_grad_(True)
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="training"):
        pol.model(torch.zeros(1, 2, D, device=dev))


def test_search_replayed_from_a_captured_graph(dev):
    """One lstm_predict_f32 recorded into a graph and replayed twice: the bits of the eager call."""
    pol = make_policy(dev, "holonomic", 61, True, "plain")
    pol.build_action_space(1.0)
    robot, humans = cpu.scenes(41, 6, 5)
    r64, h64 = torch.tensor(robot, device=dev), torch.tensor(humans, device=dev)
    r32, h32 = r64.float(), h64.float()
    search = pol.gcn_search()
    want_vals, want_best = search.search(r32, h32, roots64=(r64, h64))
    want = [want_vals.clone(), want_best.clone(), search.last_best_value.clone(), search.last_order.clone()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        search.search(r32, h32, roots64=(r64, h64))           # warm-up of the capture recipe
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vals, best = search.search(r32, h32, roots64=(r64, h64))
        best_value, order = search.last_best_value, search.last_order
    for _ in range(2):
        for t in (vals, best, best_value, order):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, ref in zip((vals, best, best_value, order), want):
            assert torch.equal(got, ref)


def test_episodes_through_the_explorer(dev):
    from relationalgraphlearning_amd import register
    from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig, run_episodes
    from relationalgraphlearning_amd.vector_explorer import VectorExplorer
    assert register({})["lstm_rl"].__name__ == "LstmRL"
    pol = make_policy(dev, "holonomic", 61, True, "plain")
    assert pol.name == "LSTM-RL"
    cfg = SimConfig(time_limit=4)
    ref = run_episodes(BatchedCrowdSim(dev, cfg), pol, "test", range(4), gamma=0.9)
    ex = VectorExplorer(BatchedCrowdSim(dev, cfg), pol, gamma=0.9, target_policy=pol)
    stats = ex.run_k_episodes(4, "test")
    assert len(stats) == 5 and all(np.isfinite(s) for s in stats)
    assert np.array_equal(np.array(ex.last_run["outcome"]), ref["outcome"]) and ref["unfinished"] == 0
    with pytest.raises(NotImplementedError, match="LSTM-RL training"):
        ex.run_k_episodes(2, "val", update_memory=True)
