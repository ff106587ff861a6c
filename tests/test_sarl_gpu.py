"""SARL / OM-SARL on the MI355X: the occupancy maps, the attention value network, the one-step search and the policy around them,
against the float64 restatement of tests/sarl_cpu.py and against what upstream recorded in tests/golden/sarl.npz.

The value bound is not a constant of ours: upstream's own float32 forward (torch CPU, the fixture's action_values) stands
2.55e-8 (default weights) / 2.36e-8 (sharp attention) from the float64 restatement over the fixture cases (|V| up to 0.28), and the
device -- the same float32 sums in another order, MFMA in blocks of four -- is allowed four times that (sarl_cpu.value_bound;
tests/test_sarl_cpu.py pins the measurement).  The attention weights take the same rule with their own measurement."""
import os

import numpy as np
import pytest
import torch

from tests import sarl_cpu as cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_policy(dev, kinematics, input_dim, with_global_state, weights):
    from relationalgraphlearning_amd import SARL
    from relationalgraphlearning_amd.config import policy_config
    om = cpu.om_of(input_dim)
    pol = SARL()
    pol.configure(policy_config("sarl", action_space__kinematics=kinematics, sarl__with_om=om is not None,
                                sarl__with_global_state=with_global_state, om__om_channel_size=om[2] if om else 3))
    pol.set_phase("test")
    pol.set_device(dev)
    pol.time_step = cpu.DT
    pol.model.load_state_dict({k: v.to(dev) for k, v in cpu.weight_set(weights, input_dim, with_global_state).items()})
    return pol


def device_rows(dev, r64, h64, kinematics, om):
    """The (B A, H, D) float32 rows the search's value kernel reads, from the device's own first steps."""
    from relationalgraphlearning_amd.rollout import prepare_scenes, occupancy_maps
    B, H = h64.shape[0], h64.shape[1]
    table = cpu.action_table(kinematics)
    self6, hum7, reward = prepare_scenes(r64.float(), h64.float(), table, kinematics, cpu.DT, roots64=(r64, h64))
    A = table.shape[0]
    parts = [self6[:, None, :].expand(B * A, H, 6), hum7]
    if om is not None:
        maps = occupancy_maps(h64, om[0], om[1], om[2], time_step=cpu.DT)
        parts.append(maps[:, None].expand(B, A, H, maps.shape[2]).reshape(B * A, H, -1))
    return torch.cat(parts, dim=2).contiguous(), reward.reshape(B, A)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)))


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("H", [2, 5, 7, 20])
def test_maps_match_the_restatement(dev, H, channels):
    from relationalgraphlearning_amd.rollout import occupancy_maps
    _, humans = cpu.scenes(900 + H, 12, H)
    extra = [cpu.case_arrays(c["idx"])["humans"] for c in cpu.fixture_cases() if c["H"] == H and c["input_dim"] != 13]
    humans = np.concatenate([humans] + [e[None] for e in extra])
    for dt in (0.0, cpu.DT):
        got = occupancy_maps(torch.tensor(humans, device=dev), 4, 1.0, channels, time_step=dt).cpu().numpy()
        want = np.stack([cpu.occupancy_maps(cpu.propagate_humans(h, dt), 4, 1.0, channels) for h in humans])
        assert got.shape == want.shape == (humans.shape[0], H, 16 * channels)
        exact = (want == 0) | (want == 1)
        assert np.array_equal(got[exact], want[exact])
        assert (np.abs(got.astype(np.float64) - want) <= ulp32(want)).all()
        assert (want != 0).any()


def test_fixture_maps_and_transform_rows(dev):
    from relationalgraphlearning_amd.state import FullState, ObservableState, JointState
    for c in cpu.fixture_cases():
        a = cpu.case_arrays(c["idx"])
        pol = make_policy(dev, c["kinematics"], c["input_dim"], c["with_global_state"], c["weights"])
        js = JointState(FullState(*a["robot"].tolist()), [ObservableState(*h) for h in a["humans"].tolist()])
        rows = pol.transform(js).cpu().numpy()
        assert rows.shape == a["transform"].shape == (c["H"], c["input_dim"]) and pol.input_dim() == c["input_dim"]
        # the relation features are path G's (pinned bit for bit by its own tests): here two float32 evaluations of a cos + b sin
        # with |a|, |b| up to the largest distance d of the scene, each a few roundings of size ulp(d) off the exact value
        d = max(float(a["transform"][:, 11].max()), float(a["transform"][0, 0]))
        assert (np.abs(rows[:, :13] - a["transform"][:, :13]) <= 8 * np.spacing(np.float32(d))).all()
        if c["input_dim"] != 13:
            want = a["transform"][:, 13:]
            exact = (want == 0) | (want == 1)
            assert np.array_equal(rows[:, 13:][exact], want[exact])
            assert (np.abs(rows[:, 13:].astype(np.float64) - want) <= ulp32(want)).all()
            got = pol.build_occupancy_maps(js.human_states).cpu().numpy()
            assert np.array_equal(got, rows[:, 13:])


VARIANTS = [(61, True), (45, True), (29, True), (13, True), (61, False), (45, False), (29, False), (13, False)]


def check_search(dev, pol, sd, kin, input_dim, with_global_state, weights, H, B, seed):
    """One search of B roots against float64 on the rows the device prepared; returns (worst deviation, action values, best)."""
    om = cpu.om_of(input_dim)
    bound, att_bound = cpu.value_bound(weights), cpu.attention_bound(weights)
    search = pol.gcn_search()
    robot, humans = cpu.scenes(seed, B, H, kin)
    r64, h64 = torch.tensor(robot, device=dev), torch.tensor(humans, device=dev)
    dev_vals, dev_best = search.search(r64.float(), h64.float(), roots64=(r64, h64))
    vals, best = dev_vals.cpu().numpy().astype(np.float64), dev_best.cpu().numpy()
    att = search.last_attention.cpu().numpy()
    best_value = search.last_best_value.cpu().numpy()
    rows, reward = device_rows(dev, r64, h64, kin, om)
    A = reward.shape[1]
    v64, a64 = cpu.value_network(rows.cpu(), sd, with_global_state, torch.float64)
    with torch.no_grad():                                                   # the module's forward on the same rows
        v_mod = pol.model(rows).cpu().numpy()[:, 0].astype(np.float64)
    err_mod = np.abs(v_mod - v64.numpy()).max()
    assert np.abs(pol.model.attention_weights - a64[0].numpy()).max() <= att_bound
    reward = reward.cpu().numpy()
    decided = [cpu.decide(reward[b], v64[b * A:(b + 1) * A].numpy(), robot[b, 7]) for b in range(B)]
    want = np.stack([d[0] for d in decided])
    err = np.abs(vals - want).max()
    print("H %d D %d global %d %s B %d: |value - float64| module %.2e search %.2e (bound %.2e)"
          % (H, input_dim, with_global_state, weights, B, err_mod, err, bound))
    assert np.isfinite(vals).all() and err_mod <= bound and err <= bound
    left_out = 0
    for b in range(B):
        idx = decided[b][1]
        if cpu.gap(want[b]) > 2 * bound:
            assert best[b] == idx
            assert np.abs(att[b] - a64[b * A + idx].numpy()).max() <= att_bound
            assert best_value[b] == np.float32(vals[b, idx])
        else:
            left_out += 1
    assert left_out <= (B + 19) // 20
    return max(err, err_mod), dev_vals, dev_best, search.last_attention


@pytest.mark.parametrize("weights", ["plain", "sharp"])
@pytest.mark.parametrize("input_dim,with_global_state", VARIANTS)
@pytest.mark.parametrize("H", [2, 5, 7, 20])
def test_value_network_and_search_against_float64(dev, monkeypatch, H, input_dim, with_global_state, weights):
    """B = 1 (81 scenes: five tiles and one scene), 3 (a partial last tile), 40, then 3 again through ONE search object, every
    workspace filled with NaN patterns before every call (RGL_DEBUG_POISON_WORKSPACES).  B = 40 is 203 tiles, fewer than the
    workgroups a launch may start at any H, so it runs twice: as it is, and with the grid capped at 37 workgroups
    (RGL_SARL_GRID_CAP), where every workgroup walks five or six tiles -- the parking slots reused, the closing barrier, the waves'
    turns at the tail -- and must give the same bits.  H = 20 adds B = 64 (324 tiles on its 256 workgroups)."""
    monkeypatch.setenv("RGL_DEBUG_POISON_WORKSPACES", "1")
    kin = "unicycle" if (H + input_dim) % 2 else "holonomic"
    pol = make_policy(dev, kin, input_dim, with_global_state, weights)
    sd = cpu.weight_set(weights, input_dim, with_global_state)
    pol.build_action_space(1.0)
    worst = 0.0
    for B in [1, 3, 40, 3] + ([64] if H == 20 else []):
        w, vals, best, att = check_search(dev, pol, sd, kin, input_dim, with_global_state, weights, H, B, 1000 * H + B)
        worst = max(worst, w)
        if B == 40:
            monkeypatch.setenv("RGL_SARL_GRID_CAP", "37")
            w2, vals2, best2, att2 = check_search(dev, pol, sd, kin, input_dim, with_global_state, weights, H, B, 1000 * H + B)
            monkeypatch.delenv("RGL_SARL_GRID_CAP")
            assert torch.equal(vals, vals2) and torch.equal(best, best2) and torch.equal(att, att2)
    from tests.conftest import PARITY_REPORT
    PARITY_REPORT.append("sarl H %d D %d global %d %s: worst |value - float64| %.2e of %.2e allowed"
                         % (H, input_dim, with_global_state, weights, worst, cpu.value_bound(weights)))


@pytest.mark.parametrize("H,B,input_dim,with_global_state", [(2, 410, 61, True), (5, 210, 45, False), (7, 110, 29, True),
                                                             (5, 210, 61, True)])
def test_launches_larger_than_the_grid(dev, monkeypatch, H, B, input_dim, with_global_state):
    """More tiles than the launch starts workgroups, with no switch set: 2 048 / 1 024 / 512 workgroups at H = 2 / 5 / 7 (one wave
    each at 2 and 5, four waves and two workgroups per CU at 7) against 2 076 / 1 064 / 557 tiles."""
    monkeypatch.setenv("RGL_DEBUG_POISON_WORKSPACES", "1")
    assert (B * 81 + 15) // 16 > 256 * min(8 if H < 7 else 2, (160 * 1024) // (H * 7424))
    pol = make_policy(dev, "holonomic", input_dim, with_global_state, "plain")
    pol.build_action_space(1.0)
    check_search(dev, pol, cpu.weight_set("plain", input_dim, with_global_state), "holonomic", input_dim, with_global_state, "plain",
                 H, B, 5000 + H)


def test_predict_reproduces_the_fixture_decisions(dev):
    from relationalgraphlearning_amd.state import FullState, ObservableState, JointState
    for c in cpu.fixture_cases():
        a = cpu.case_arrays(c["idx"])
        pol = make_policy(dev, c["kinematics"], c["input_dim"], c["with_global_state"], c["weights"])
        js = JointState(FullState(*a["robot"].tolist()), [ObservableState(*h) for h in a["humans"].tolist()])
        action = pol.predict(js)
        bound, att_bound = cpu.value_bound(c["weights"]), cpu.attention_bound(c["weights"])
        assert cpu.gap(a["action_values"]) > 2 * bound                      # a condition on the fixture, met by every case
        table = cpu.action_table(c["kinematics"])
        assert tuple(float(x) for x in action) == tuple(table[int(a["chosen"])]), c["tag"]
        dv = np.abs(np.asarray(pol.action_values) - a["action_values"]).max()
        da = np.abs(pol.get_attention_weights() - a["attention"]).max()
        print("%s: |action value - upstream| %.2e, |attention - upstream| %.2e" % (c["tag"], dv, da))
        # device and upstream each stand within their share of float64: four parts and one part of the bound
        assert dv <= 1.25 * bound and da <= 1.25 * att_bound
        assert pol.get_attention_weights().shape == (c["H"],)


def test_refusals_on_the_device(dev):
    from relationalgraphlearning_amd import _native as nat
    pol = make_policy(dev, "holonomic", 61, True, "plain")
    robot, humans = cpu.scenes(5, 2, 1)
    assert str(cpu.fixture()["single_human_error"]) == "ValueError"
    with pytest.raises(ValueError):
        pol.predict_batch(torch.tensor(robot, device=dev).float(), torch.tensor(humans, device=dev).float())
    robot, humans = cpu.scenes(6, 1, nat.SARL_MAX_HUMANS + 1)
    with pytest.raises(nat.NativeLibraryError, match="BAD_SHAPE"):
        pol.predict_batch(torch.tensor(robot, device=dev).float(), torch.tensor(humans, device=dev).float())
    plain = make_policy(dev, "holonomic", 13, True, "plain")          # no maps: a single human is fine
    robot, humans = cpu.scenes(5, 2, 1)
    best, value = plain.predict_batch(torch.tensor(robot, device=dev).float(), torch.tensor(humans, device=dev).float())
    assert (best.cpu().numpy() >= 0).all() and np.isfinite(value.cpu().numpy()).all()
    pol.model.mlp1[0].weight.requires_grad_(True)
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="training"):
        pol.model(torch.zeros(1, 2, 61, device=dev))


def test_checkpoint_round_trip(dev, tmp_path):
    pol = make_policy(dev, "holonomic", 61, True, "sharp")
    path = os.path.join(str(tmp_path), "sarl.pth")
    pol.save_model(path)
    sd = torch.load(path)
    assert sorted(sd) == sorted("%s.%s" % (l, p) for l in cpu.LAYERS for p in ("weight", "bias"))
    other = make_policy(dev, "holonomic", 61, True, "plain")
    robot, humans = cpu.scenes(31, 5, 5)
    r, h = torch.tensor(robot, device=dev).float(), torch.tensor(humans, device=dev).float()
    want_best, want_value = pol.predict_batch(r, h)
    before = other.predict_batch(r, h)[1].clone()
    other.load_model(path)
    best, value = other.predict_batch(r, h)
    assert torch.equal(best, want_best) and torch.equal(value, want_value) and not torch.equal(before, value)


def test_episodes_through_the_explorer(dev):
    from relationalgraphlearning_amd import register
    from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig, run_episodes
    from relationalgraphlearning_amd.vector_explorer import VectorExplorer
    assert register({})["sarl"].__name__ == "SARL"
    pol = make_policy(dev, "holonomic", 61, True, "plain")
    assert pol.name == "OM-SARL"
    cfg = SimConfig(time_limit=4)
    ref = run_episodes(BatchedCrowdSim(dev, cfg), pol, "test", range(4), gamma=0.9)
    ex = VectorExplorer(BatchedCrowdSim(dev, cfg), pol, gamma=0.9, target_policy=pol)
    stats = ex.run_k_episodes(4, "test")
    assert len(stats) == 5 and all(np.isfinite(s) for s in stats)
    assert np.array_equal(np.array(ex.last_run["outcome"]), ref["outcome"]) and ref["unfinished"] == 0
    with pytest.raises(NotImplementedError, match="SARL"):
        ex.run_k_episodes(2, "val", update_memory=True)
