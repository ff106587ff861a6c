"""SARL / OM-SARL for 21..127 humans on the MI355X: the value kernel's form that parks in the workspace against the LDS form (same
bits at the crowd sizes both run) and against float64 (tests/sarl_dense.py: the roots, the float64 search, the bound of each case),
the maps kernel at those crowd sizes, the refusals and episodes through the explorer."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sarl_cpu as cpu
from tests import sarl_dense as dense
from tests.test_sarl_gpu import make_policy, device_rows, ulp32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def value_workspace(pol, S, H):
    """(bytes sarl_value_f32 wants for S scenes of H humans, bytes of the packed weights alone)."""
    from relationalgraphlearning_amd import _native as nat
    pl = pol.model.fill_planner(nat.SarlPlanner())
    lib = nat.lib()
    return lib.sarl_value_workspace_bytes_for(ctypes.byref(pl), S, H), lib.sarl_value_workspace_bytes(ctypes.byref(pl))


@pytest.mark.parametrize("input_dim", [13, 61])
@pytest.mark.parametrize("with_global_state", [True, False])
@pytest.mark.parametrize("H", [2, 5, 7, 20])
def test_global_form_gives_the_bits_of_the_lds_form(dev, monkeypatch, H, with_global_state, input_dim):
    """Three roots (243 scenes: sixteen tiles, the last of three scenes) through the search, predict_batch and the module's forward:
    as the launch chooses (LDS), with RGL_SARL_PARK=global, and with the grid capped at two workgroups on top, where each walks
    eight tiles over its one region.  Every workspace carries NaN patterns before every call."""
    monkeypatch.setenv("RGL_DEBUG_POISON_WORKSPACES", "1")
    monkeypatch.delenv("RGL_SARL_PARK", raising=False)
    kin = "unicycle" if (H + input_dim) % 2 else "holonomic"
    pol = make_policy(dev, kin, input_dim, with_global_state, "sharp" if H % 2 else "plain")
    pol.build_action_space(1.0)
    robot, humans = cpu.scenes(8000 + H, 3, H, kin)
    r64, h64 = torch.tensor(robot, device=dev), torch.tensor(humans, device=dev)
    rows, _ = device_rows(dev, r64, h64, kin, cpu.om_of(input_dim))

    def run():
        search = pol.gcn_search()
        vals, best = search.search(r64.float(), h64.float(), roots64=(r64, h64))
        out = [vals.clone(), best.clone(), search.last_attention.clone(), search.last_best_value.clone()]
        out += [t.clone() for t in pol.predict_batch(r64.float(), h64.float())]
        with torch.no_grad():
            out.append(pol.model(rows).clone())
        out.append(torch.tensor(pol.model.attention_weights))
        return out

    want = run()
    assert all(bool(torch.isfinite(t.float()).all()) for t in want)
    need, packed = value_workspace(pol, rows.shape[0], H)
    assert need == packed
    monkeypatch.setenv("RGL_SARL_PARK", "global")
    need, packed = value_workspace(pol, rows.shape[0], H)
    assert need >= packed + 16 * H * 29 * 256
    got = run()
    monkeypatch.setenv("RGL_SARL_GRID_CAP", "2")
    capped = run()
    for a, b, c in zip(want, got, capped):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("weights", ["plain", "sharp"])
@pytest.mark.parametrize("H", dense.DENSE_H)
def test_dense_crowds_against_float64(dev, monkeypatch, H, weights):
    """Two roots (162 scenes: eleven tiles, the last of two scenes) per row width and global-state setting.  The search's action
    values and the selected action's attention weights against tests/sarl_cpu.search in float64, and the module's forward on that
    search's own rows; a case's bound is the larger of the small crowds' bound and four times the float32 restatement's distance from
    float64 on the case's scenes.  Decisions are compared where the two best actions are more than twice the bound apart; at most
    one root in ten of a parametrisation may fall below that (tests/test_sarl_dense_cpu.py holds the restatement to the same)."""
    monkeypatch.setenv("RGL_DEBUG_POISON_WORKSPACES", "1")
    monkeypatch.delenv("RGL_SARL_PARK", raising=False)
    left_out = total = 0
    worst_value = worst_attention = 0.0
    for input_dim in dense.INPUT_DIMS:
        for with_global_state in (True, False):
            kin = dense.kinematics_of(H, input_dim)
            roots = dense.case(H, input_dim, with_global_state, weights)
            value_bound, attention_bound = dense.bounds(weights, roots)
            pol = make_policy(dev, kin, input_dim, with_global_state, weights)
            pol.build_action_space(1.0)
            robot, humans = dense.roots(H, input_dim)
            r64, h64 = torch.tensor(robot, device=dev), torch.tensor(humans, device=dev)
            search = pol.gcn_search()
            dev_vals, dev_best = search.search(r64.float(), h64.float(), roots64=(r64, h64))
            vals, best = dev_vals.cpu().numpy().astype(np.float64), dev_best.cpu().numpy()
            att = search.last_attention.cpu().numpy().astype(np.float64)
            rows = torch.cat([r["rows"] for r in roots]).to(dev)
            with torch.no_grad():
                v_mod = pol.model(rows).cpu().numpy()[:, 0].astype(np.float64)
            err_mod = float(np.abs(v_mod - np.concatenate([r["value"] for r in roots])).max())
            err_att0 = float(np.abs(pol.model.attention_weights - roots[0]["attention"][0]).max())
            err = float(np.abs(vals - np.stack([r["action_values"] for r in roots])).max())
            err_att = 0.0
            for b, r in enumerate(roots):
                total += 1
                if cpu.gap(r["action_values"]) > 2 * value_bound:
                    assert best[b] == r["best"]
                    err_att = max(err_att, float(np.abs(att[b] - r["attention"][r["best"]]).max()))
                else:
                    left_out += 1
            print("H %d D %d global %d %s: |value - float64| module %.2e search %.2e (bound %.2e), |attention - float64| module %.2e "
                  "search %.2e (bound %.2e)" % (H, input_dim, with_global_state, weights, err_mod, err, value_bound, err_att0, err_att,
                                                attention_bound))
            assert np.isfinite(vals).all() and np.isfinite(v_mod).all()
            assert err_mod <= value_bound and err <= value_bound
            assert err_att0 <= attention_bound and err_att <= attention_bound
            worst_value, worst_attention = max(worst_value, err, err_mod), max(worst_attention, err_att, err_att0)
    assert 10 * left_out <= total
    from tests.conftest import PARITY_REPORT
    PARITY_REPORT.append("sarl dense H %d %s: worst |value - float64| %.2e, |attention - float64| %.2e, %d of %d decisions left out"
                         % (H, weights, worst_value, worst_attention, left_out, total))


def test_more_tiles_than_workgroups(dev, monkeypatch):
    """104 roots of 21 humans are 527 tiles on the 512 workgroups a launch of the global form starts at most: fifteen workgroups walk
    a second tile over their region.  The same bits with the grid capped at 37 workgroups (fourteen or fifteen tiles each), and for
    the first three roots launched alone (sixteen workgroups, a tile each)."""
    monkeypatch.setenv("RGL_DEBUG_POISON_WORKSPACES", "1")
    monkeypatch.delenv("RGL_SARL_PARK", raising=False)
    H, B = 21, 104
    assert (B * 81 + 15) // 16 > 512
    pol = make_policy(dev, "holonomic", 61, True, "plain")
    pol.build_action_space(1.0)
    robot, humans = cpu.scenes(9021, B, H)
    r64, h64 = torch.tensor(robot, device=dev), torch.tensor(humans, device=dev)

    def run(n):
        search = pol.gcn_search()
        vals, best = search.search(r64[:n].float(), h64[:n].float(), roots64=(r64[:n].contiguous(), h64[:n].contiguous()))
        return vals.clone(), best.clone(), search.last_attention.clone()

    natural = run(B)
    assert bool(torch.isfinite(natural[0]).all()) and bool((natural[1] >= 0).all())
    monkeypatch.setenv("RGL_SARL_GRID_CAP", "37")
    capped = run(B)
    monkeypatch.delenv("RGL_SARL_GRID_CAP")
    alone = run(3)
    for a, b, c in zip(natural, capped, alone):
        assert torch.equal(a, b) and torch.equal(a[:3], c)


def crowded_and_far(H, seed):
    """Three crowds of H humans: seeded; humans 1 and 2 of crowd 1 in one cell of human 0's grid, moving with it; the last two humans
    of crowd 2 a hundred metres from everybody."""
    _, humans = cpu.scenes(seed, 3, H)
    humans[1, 0] = [0.0, 0.0, 0.5, 0.0, 0.3]
    humans[1, 1] = [0.30, 0.35, 0.5, 0.0, 0.3]
    humans[1, 2] = [0.65, 0.70, 0.5, 0.0, 0.3]
    humans[2, H - 2, :2] = [100.0, 100.0]
    humans[2, H - 1, :2] = [-100.0, 80.0]
    return humans


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("H", [21, 50, 127])
def test_maps_of_dense_crowds(dev, H, channels):
    from relationalgraphlearning_amd.rollout import occupancy_maps
    humans = crowded_and_far(H, 900 + H)
    for dt in (0.0, cpu.DT):
        moved = [cpu.propagate_humans(h, dt) for h in humans]
        coords = []
        want = np.stack([cpu.occupancy_maps(h, 4, 1.0, channels, coords=coords if k == 1 else None) for k, h in enumerate(moved)])
        cells = np.floor(np.asarray(coords[:4]).reshape(2, 2))             # humans 1 and 2 in human 0's frame
        assert (cells[0] == cells[1]).all() and (cells >= 0).all() and (cells < 4).all()
        assert (want[2, H - 2:] == 0).all() and (want[2, :H - 2] != 0).any()
        got = occupancy_maps(torch.tensor(humans, device=dev), 4, 1.0, channels, time_step=dt).cpu().numpy()
        assert got.shape == want.shape == (3, H, 16 * channels)
        exact = (want == 0) | (want == 1)
        assert np.array_equal(got[exact], want[exact])
        assert (np.abs(got.astype(np.float64) - want) <= ulp32(want)).all()


def test_refusals_of_dense_crowds(dev, monkeypatch):
    from relationalgraphlearning_amd import _native as nat
    monkeypatch.delenv("RGL_SARL_PARK", raising=False)
    pol = make_policy(dev, "holonomic", 61, True, "plain")
    assert nat.SARL_MAX_HUMANS == 127
    robot, humans = cpu.scenes(6, 1, 128)
    with pytest.raises(nat.NativeLibraryError, match="BAD_SHAPE"):
        pol.predict_batch(torch.tensor(robot, device=dev).float(), torch.tensor(humans, device=dev).float())
    with torch.no_grad(), pytest.raises(nat.NativeLibraryError, match="BAD_SHAPE"):
        pol.model(torch.zeros(1, 128, 61, device=dev))
    robot, humans = cpu.scenes(5, 2, 1)
    with pytest.raises(ValueError):
        pol.predict_batch(torch.tensor(robot, device=dev).float(), torch.tensor(humans, device=dev).float())
    # the C ABI: 21 humans with the workspace that was enough for 20
    S, H = 16, 21
    need, packed = value_workspace(pol, S, H)
    assert need >= packed + H * 29 * 256
    pl = pol.model.fill_planner(nat.SarlPlanner())
    rows = torch.zeros(S, H, 61, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    value, att = torch.empty(S, device=dev), torch.empty(S, H, device=dev)
    lib = nat.lib()
    args = (ctypes.byref(pl), rows.data_ptr(), None, None, None, S, 1, H, ws.data_ptr())
    for given in (packed, need - 1):
        assert lib.sarl_value_f32(*args, given, value.data_ptr(), att.data_ptr(), None) == -4
    assert nat.ERRORS[-4] == "RGL_ERR_WORKSPACE"
    torch.cuda.synchronize()
    assert lib.sarl_value_f32(*args, need, value.data_ptr(), att.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(value).all()) and bool((att.sum(dim=1) - 1).abs().max() < 1e-5)


def test_episodes_among_25_humans(dev, monkeypatch):
    from relationalgraphlearning_amd.sim import BatchedCrowdSim, SimConfig
    from relationalgraphlearning_amd.vector_explorer import VectorExplorer
    monkeypatch.delenv("RGL_SARL_PARK", raising=False)
    pol = make_policy(dev, "holonomic", 61, True, "plain")
    assert pol.name == "OM-SARL"

    def episodes(human_num, radius):
        cfg = SimConfig(time_limit=4, human_num=human_num, circle_radius=radius)
        ex = VectorExplorer(BatchedCrowdSim(dev, cfg, human_policy="linear"), pol, gamma=0.9, target_policy=pol)
        stats = ex.run_k_episodes(4, "test")
        assert len(stats) == 5 and all(np.isfinite(s) for s in stats)
        assert len(ex.last_run["outcome"]) == 4 and all(int(o) in (2, 3, 4) for o in ex.last_run["outcome"])
        return [int(o) for o in ex.last_run["outcome"]], ex.last_run["actions"]

    episodes(25, 8)
    want = episodes(5, 4)
    monkeypatch.setenv("RGL_SARL_PARK", "global")
    assert episodes(5, 4) == want
