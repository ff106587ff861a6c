"""The host replay of the search's bookkeeping (tests/search_bookkeeping.py) against the oracle, bit for bit.

The replay is what the GPU tests of tests/test_search_bookkeeping.py hold the kernels to; here it is pinned to the oracle -- which
is itself pinned to the reference's fixtures (tests/test_oracle_golden.py) -- on every planning and root-clip fixture case and on
deeper / wider searches over the fixture scenes: fed the oracle's per-level arrays it must give the oracle's one-step values, kept
actions (in the oracle's order), root values, best value and best action with no tolerance.
"""
import numpy as np
import pytest
import torch

from oracle import rgl_oracle as orc
from tests import golden_io as gio
from tests import search_bookkeeping as sb


def _replay_of_oracle_levels(levels, cfg, groups):
    A = levels[0]["reward"].shape[1]
    lv = [{"reward": e["reward"].numpy(), "child_value": e["child_value"].numpy(), "child_robot": e["child_robot"].numpy(),
           "humans_next": e["next_humans"].numpy(), "reward_clip": e["reward_clip"].numpy() if "reward_clip" in e else None}
          for e in levels]
    W = cfg.planning_width if cfg.do_action_clip else A
    return sb.replay(lv, orc._normalized_gamma(cfg), cfg.planning_depth, W, cfg.do_action_clip, cfg.sparse_search, groups)


def _check_against_oracle(robot, humans, params, cfg, roots64=None):
    with torch.no_grad():
        oa, ov, orv, okept, levels = orc.mprl_predict_batched(robot, humans, params, cfg, return_levels=True, roots64=roots64)
    _, groups = orc.mprl_action_space(cfg, cfg.v_pref)
    rep = _replay_of_oracle_levels(levels, cfg, groups)
    for l, (got, want) in enumerate(zip(rep["levels"], levels)):
        assert want["value1"].dtype == torch.float32
        assert np.array_equal(sb.bits(got["value1"]), sb.bits(want["value1"].numpy())), ("value1", l)
        assert np.array_equal(got["keep"], want["keep"].numpy()), ("keep", l)        # ordered: select_top orders its rows
        if l + 1 < len(levels):                                                          # the parents the oracle expanded next
            assert got["next_robot"].shape[0] == levels[l + 1]["reward"].shape[0]
    assert np.array_equal(sb.bits(rep["root_values"]), sb.bits(orv.numpy()))
    assert np.array_equal(rep["root_kept"], okept.numpy())
    assert np.array_equal(rep["best_action"], oa.numpy())
    assert np.array_equal(sb.bits(rep["best_value"]), sb.bits(ov.numpy()))
    assert (rep["best_slot"] >= 0).all()
    return rep, levels


@pytest.mark.parametrize("c", gio.plan_cases(), ids=lambda c: c["tag"])
def test_replay_reproduces_the_oracle_on_the_planning_fixture(c):
    pl = gio.load("planning")
    cfg = orc.OracleConfig(planning_depth=c["D"], planning_width=c["w"], do_action_clip=c["clip"], sparse_search=c["sparse"],
                           linear_state_predictor=(c["variant"] == "linear"))
    R = torch.tensor(pl["plan.scene.%s.robot" % c["scene"]].astype(np.float32))
    Hh = torch.tensor(pl["plan.scene.%s.humans" % c["scene"]].astype(np.float32))
    rep, _ = _check_against_oracle(R, Hh, gio.oracle_params(c["flavour"], 2, c["variant"]), cfg)
    # and the reference's own recorded decision
    assert np.array_equal(rep["best_action"], pl["plan.%s.action" % c["tag"]])


@pytest.mark.parametrize("c", gio.root_clip_cases(), ids=lambda c: c["tag"])
def test_replay_reproduces_the_oracle_on_the_root_clip_fixture(c):
    """Joint-state roots given in float64: the selection reads `reward_clip`, the root values read `reward`."""
    rc = gio.load("root_clip")
    cfg = orc.OracleConfig(planning_depth=c["D"], planning_width=c["w"], do_action_clip=True, sparse_search=c["sparse"],
                           linear_state_predictor=(c["variant"] == "linear"))
    R64, H64 = rc["rootclip.robot64"], rc["rootclip.humans64"]
    R32, H32 = torch.tensor(R64.astype(np.float32)), torch.tensor(H64.astype(np.float32))
    rep, levels = _check_against_oracle(R32, H32, gio.oracle_params("trained", 2, c["variant"]), cfg, roots64=(R64, H64))
    assert "reward_clip" in levels[0] and not torch.equal(levels[0]["reward_clip"], levels[0]["reward"])
    assert np.array_equal(rep["best_action"], rc["rootclip.%s.action" % c["tag"]])


@pytest.mark.parametrize("D,w,clip,sparse", [(1, 1, False, False), (2, 2, True, False), (2, 5, True, False), (3, 2, True, False),
                                             (3, 3, True, True), (4, 2, True, False), (4, 5, True, False)])
def test_replay_reproduces_the_oracle_on_deeper_and_wider_searches(D, w, clip, sparse):
    """The three roots of planning.npz's scene s5 with the trained weights, up to depth 4 and width 5 (d = 2, 3, 4 in the
    back-up: c = 1/2, 2/3, 3/4)."""
    pl = gio.load("planning")
    cfg = orc.OracleConfig(planning_depth=D, planning_width=w, do_action_clip=clip, sparse_search=sparse)
    R = torch.tensor(pl["plan.scene.s5.robot"].astype(np.float32))
    Hh = torch.tensor(pl["plan.scene.s5.humans"].astype(np.float32))
    _check_against_oracle(R, Hh, gio.oracle_params("trained"), cfg)


SELECT_A = (1, 2, 63, 64, 65, 81, 128, 129, 192, 193, 255, 256)
NAN_FREE = ("distinct", "three_levels", "all_equal", "leader", "two_leaders", "inf_mixed", "all_neg_inf", "zeros", "denormals")


def select_widths(A):
    return sorted({w for w in (1, 2, 3, 16, 17, A - 1, A) if 1 <= w <= A})


@pytest.mark.parametrize("A", SELECT_A)
def test_replay_order_is_the_oracles_on_the_synthetic_rows(A):
    """The NaN-free families of the GPU selection test: the replay's kept lists equal orc.select_top's.  Dense selection on every
    family (both order exact ties lower index first); the sparse walk on the `distinct` family only -- the oracle's sparse walk
    is numpy's reversed argsort, which visits exact ties in a platform-defined order (the documented deviation)."""
    fam = sb.synthetic_rows(A)
    g = 0.9 ** 0.25
    n = 0
    for name in NAN_FREE:
        if name not in fam:
            continue
        v1 = sb.one_step_values(fam[name][0], fam[name][1], g)
        assert not np.isnan(v1).any(), name
        for W in select_widths(A):
            assert np.array_equal(sb.select(v1, W), orc.select_top(v1, W, None, False)), (name, W)
            n += 1
    v1 = sb.one_step_values(*fam["distinct"], g)
    assert all(len(set(row.tolist())) == A for row in v1)
    for groups in (np.arange(A) % 5, np.arange(A)[::-1].copy(), np.arange(A) // 7 - 3):
        for W in (1, 3, 16):
            if W <= len(set(groups.tolist())):                     # the oracle has no fallback fill
                assert np.array_equal(sb.select(v1, W, True, True, groups), orc.select_top(v1, W, groups, True)), W
                n += 1
    assert n > 0


def test_synthetic_rows_are_what_their_names_say():
    """Row counts per family (stated in synthetic_rows' docstring) and the property each family is there for, on the values the
    selection sees; among them: a cut inside a tie, winners in every lane slot, NaNs produced by the addition itself."""
    g = 0.9 ** 0.25
    for A in SELECT_A:
        fam = sb.synthetic_rows(A)
        v = {k: sb.one_step_values(r, c, g) for k, (r, c) in fam.items()}
        assert set(fam) <= set(sb.FAMILIES) and all(r.shape == c.shape == (r.shape[0], A) and r.shape[0] > 0 for r, c in fam.values())
        assert v["distinct"].shape[0] == 4 and v["three_levels"].shape[0] == 4 and v["all_equal"].shape[0] == 2
        assert (v["all_equal"] == v["all_equal"][:, :1]).all() and np.isneginf(v["all_neg_inf"]).all()
        want_leaders = sorted({i for i in sb.LEADER_INDICES + (A - 1,) if i < A})
        assert v["leader"].argmax(1).tolist() == want_leaders and ((v["leader"] == 2.0).sum(1) == 1).all()
        if A >= 2:
            assert ((v["two_leaders"] == 2.0).sum(1) == 2).all() and (v["two_leaders"].max(1) == 2.0).all()
            nn = np.isnan(v["some_nans"]).sum(1)
            assert ((nn > 0) & (nn < A)).all()
        if A > 64:
            lead = [np.nonzero(row == 2.0)[0] for row in v["two_leaders"]]
            assert all(b - a == 64 for a, b in lead)                                   # two slots of ONE lane
            assert {int(a) // 64 for a, _ in lead} == {k for k in range(3) if 64 * (k + 1) < A}
        assert np.isinf(v["inf_mixed"]).any(1).all() and not np.isnan(v["inf_mixed"]).any()
        assert np.isnan(v["only_nans"]).all() and len(np.unique(fam["only_nans"][0].view(np.uint32))) > 1
        assert np.isnan(v["nan_from_inf"]).any(1).all() and not np.isnan(fam["nan_from_inf"][0]).any()
        assert (v["zeros"][:2] == 0).all() and np.signbit(v["zeros"]).any() and (~np.signbit(v["zeros"])).any()
        d = v["denormals"]
        assert (np.abs(d) < np.finfo(np.float32).tiny).all() and (d != 0).any()
        if A >= 16:
            t = v["three_levels"]
            order = sb.descending_order(t)
            cut_in_tie = [W for W in select_widths(A) if W < A
                          and (np.take_along_axis(t, order[:, W - 1:W], 1) == np.take_along_axis(t, order[:, W:W + 1], 1)).any()]
            assert len(cut_in_tie) >= 3, cut_in_tie


def test_replay_scans_are_first_strict_maxima():
    """The two scans on hand-made rows: ties keep the first slot, a NaN is never taken over a number, a leading NaN stays in the
    back-up scan (nothing compares greater than it) and the root scan returns slot -1 / -inf when nothing is above -inf."""
    nan, inf = np.nan, np.inf
    ret = np.array([[1, 2, 2], [3, 3, 1], [nan, 5, 6], [1, nan, 0], [-inf, -inf, -inf]], np.float32)
    best, slot = sb._first_strict_maximum(ret)
    assert slot.tolist() == [1, 0, 0, 0, 0] and np.isnan(best[2]) and best[[0, 1, 3]].tolist() == [2, 3, 1]
    best, slot = sb._first_strict_maximum(ret, -np.inf)
    assert slot.tolist() == [1, 0, 2, 0, -1] and best[:4].tolist() == [2, 3, 6, 1] and np.isneginf(best[4])
    v = np.array([[0.0, -0.0, nan, 1.0, -inf, nan, 1.0, inf]], np.float32)
    assert sb.descending_order(v)[0].tolist() == [7, 3, 6, 0, 1, 4, 2, 5]
    groups = np.array([4, 4, 4, 9, 9, 9, 9, 4])
    assert sb.select(v, 3, True, True, groups)[0].tolist() == [7, 3, 3]             # two groups, width 3: the last one repeats
