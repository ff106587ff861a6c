"""The search's select, back-up and root steps (csrc/rgl_tail.h) against the host replay (tests/search_bookkeeping.py), BIT FOR BIT.

Every operation of the bookkeeping is an individually rounded float32 operation on arrays the search leaves in its workspace, so
given the device's own `reward` / `child_value` (/ `child_robot` / `humans_next`) arrays the replay must reproduce every other
array exactly: no tolerance, no forgiven ties.  The replay is pinned to the oracle by tests/test_search_bookkeeping_cpu.py; nothing
computed by the code under test is used as an expectation.

  * selection on synthetic arrays through TreeSearch.action_clip (mprl_select_kernel -> tail_select): every lane slot, ties,
    NaN / inf / zero ordering, widths up to A, the sparse walk and its fallback fill, blocks with fewer than four parents;
  * whole searches replayed level by level, with the trained weights (distinct values) and with the value head's last weight
    zeroed (V = the last bias for every state: exact ties at every level), over depths, widths, action tables and root readings;
  * the same searches under every form the bookkeeping is compiled into (fused kernel tail with / without the back-up chain,
    robot_head_kernel's tail, the deep kernel's trailing phase, the stand-alone kernels), one child process per environment --
    the switches are read once per process -- each checked against the replay and, with the tie weights, against each other
    wherever the forms hand the bookkeeping bit-equal inputs.

NaNs are compared as NaNs (one canonical pattern): the payload and sign of a NaN that an addition generates are the platform's.
profiles/search_bookkeeping_forms.txt holds the kernel calls of every case of every form, from kernel traces of child_main.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import relationalgraphlearning_amd as rga
from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd.config import policy_config
from tests import golden_io as gio
from tests import search_bookkeeping as sb
from tests.helpers import dense_scenes, make_mprl_policy
from tests.test_gpu_parity import report, seeded_scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def same_bits(got, want):
    return np.array_equal(sb.bits(got), sb.bits(want))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. selection on synthetic arrays (mprl_action_clip_f32 -> mprl_select_kernel -> tail_select)
# ---------------------------------------------------------------------------------------------------------------------------
SELECT_A = (1, 2, 63, 64, 65, 81, 128, 129, 192, 193, 255, 256)
SELECT_P = (1, 3, 4, 5, 1027)          # four parents per block: a lone wave, a partial block, a full one, one over, many blocks


def select_widths(A):
    return sorted({w for w in (1, 2, 3, 16, 17, A - 1, A) if 1 <= w <= A})


@pytest.fixture(scope="module")
def nets(dev):
    pol = make_mprl_policy("trained", device=dev)
    return pol.value_estimator, pol.state_predictor


def selector(nets, A, clip, sparse=False, groups=None):
    """A TreeSearch whose action table has A rows (action_clip reads only their number)."""
    table = np.stack([np.linspace(0.0, 1.0, A), np.zeros(A)], axis=1)
    return rga.TreeSearch(nets[0], nets[1], table, groups, planning_depth=1, planning_width=1, do_action_clip=clip,
                          sparse_search=sparse)


def group_ids(A):
    """Sparse walks: many members per group (arbitrary int32 ids), one member per group, fewer distinct ids than the width."""
    many = np.array([-2 ** 31, 7, 2 ** 31 - 1, 0, -1], np.int64)[np.arange(A) % 5].astype(np.int32)
    single = (np.random.RandomState(A).permutation(A) * 3 - A).astype(np.int32)
    few = (np.arange(A) % 2 * 40 - 20).astype(np.int32)
    return {"many": many, "single": single, "few": few}


def run_select(ts, reward, child_value, width, dev, sparse=False, groups=None, clip=True):
    v1, keep = ts.action_clip(torch.tensor(reward).to(dev), torch.tensor(child_value).to(dev), width)
    torch.cuda.synchronize()
    want_v1 = sb.one_step_values(reward, child_value, ts.gamma_bar)
    got_v1 = v1.cpu().numpy()
    assert same_bits(got_v1, want_v1), "value1"
    want = sb.select(want_v1, width, clip, sparse, groups)
    got = keep.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape
    if not np.array_equal(got, want):
        p = int(np.nonzero((got != want).any(1))[0][0])
        raise AssertionError("keep differs at parent %d of %d: device %s, replay %s, values %s"
                             % (p, got.shape[0], got[p].tolist(), want[p].tolist(), want_v1[p, want[p]].tolist()))
    return want_v1, want


@pytest.mark.parametrize("A", SELECT_A)
def test_selection_on_synthetic_rows(A, nets, dev):
    """Rows per family: see search_bookkeeping.synthetic_rows (4 distinct, 4 three-level, 2 all-equal, one strict leader at each of
    0, 63, 64, 127, 128, 191, 192, A-1 that exists, two tied leaders in two slots of one lane, 3 with infinities, 1 all -inf, 3 of
    signed zeros, 2 of denormals, 3 with some NaNs, 2 of NaNs only, 2 where +inf + g * -inf makes the NaNs); every count asserted
    non-zero below.  Every width of {1, 2, 3, 16, 17, A-1, A} <= A, clipping off, the sparse walk with W in {1, 3, 16} over three
    kinds of group ids, and P in {1, 3, 4, 5, 1027}."""
    reward, cv, counts = sb.synthetic_batch(A)
    for f in sb.FAMILIES:
        if A >= 2 or f not in ("two_leaders", "some_nans"):
            assert counts.get(f, 0) > 0, f
    n = reward.shape[0]
    batches = {"all": np.arange(n)}
    for P in SELECT_P:
        batches["P%d" % P] = (np.arange(P) * 5 + P) % n if P < 10 else np.arange(P) % n
    ts = selector(nets, A, True)
    launches = ties_cut = 0
    for tag, rows in batches.items():
        widths = select_widths(A)
        for W in widths:
            v1, keep = run_select(ts, reward[rows], cv[rows], W, dev)
            launches += 1
            if W < A:                                                     # rows whose cut at W falls inside a tie
                order = sb.descending_order(v1)
                ties_cut += int((np.take_along_axis(v1, order[:, W - 1:W], 1) == np.take_along_axis(v1, order[:, W:W + 1], 1)).sum())
    if A >= 2:
        assert ties_cut > 0
    ts_off = selector(nets, A, False)
    for tag in ("all", "P3", "P1027"):
        _, keep = run_select(ts_off, reward[batches[tag]], cv[batches[tag]], None, dev, clip=False)
        assert keep.shape[1] == A
        launches += 1
    for kind, groups in group_ids(A).items():
        ts_sp = selector(nets, A, True, True, groups)
        n_groups = len(set(groups.tolist()))
        for W in (1, 3, 16):
            if W > A:
                continue
            for tag in ("all", "P5") + (("P1027",) if kind == "many" else ()):
                _, keep = run_select(ts_sp, reward[batches[tag]], cv[batches[tag]], W, dev, True, groups)
                launches += 1
                if W > n_groups:                                          # the fallback fill: the last action kept, repeated
                    assert (keep[:, n_groups:] == keep[:, n_groups - 1:n_groups]).all()
    report("selection, A = %d: %d launches of mprl_select_kernel equal to the replay bit for bit (%d rows per batch of %d families; "
           "%d row-widths cut inside a tie)" % (A, launches, n, len(counts), ties_cut))


def test_selection_refusals(nets, dev):
    """A = 257, W > A and a sparse W = 17 are refused; P = 0 succeeds and writes nothing."""
    r = torch.zeros(3, 257, device=dev)
    with pytest.raises(nat.NativeLibraryError, match="RGL_ERR_BAD_SHAPE"):
        selector(nets, 257, True).action_clip(r, r, 2)
    r = torch.zeros(3, 81, device=dev)
    with pytest.raises(nat.NativeLibraryError, match="RGL_ERR_BAD_SHAPE"):
        selector(nets, 81, True).action_clip(r, r, 82)
    groups = np.arange(81, dtype=np.int32)
    sparse = selector(nets, 81, True, True, groups)
    with pytest.raises(nat.NativeLibraryError, match="RGL_ERR_BAD_MODE"):
        sparse.action_clip(r, r, 17)
    v1, keep = sparse.action_clip(r, r, 16)                              # the widest sparse selection is served
    assert keep.cpu().numpy().tolist() == [list(range(16))] * 3
    # P = 0 with live pointers: success, and not a byte written
    pl = sparse.planner(dev)
    pl.planning_width = 3
    v1 = torch.full((4, 81), 7.0, device=dev)
    keep = torch.full((4, 3), -5, dtype=torch.int32, device=dev)
    from relationalgraphlearning_amd.nets import _stream
    with torch.cuda.device(dev):
        import ctypes as C
        rc = nat.lib().mprl_action_clip_f32(C.byref(pl), r.data_ptr(), r.data_ptr(), 0, v1.data_ptr(), keep.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((v1 == 7.0).all()) and bool((keep == -5).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 2. whole searches replayed
# ---------------------------------------------------------------------------------------------------------------------------
def case(weights, scenes, seed, B, H, D, W, clip=True, sparse=False, table=(5, 16), roots="joint", contraction="f32", L=2,
         sim="embedded_gaussian", note=""):
    """weights: "trained" | "tie" (the trained policy with the value head's last weight zeroed); scenes: "seeded" | "dense";
    table: (speed samples, rotation samples) -> A = their product + 1; roots: "tensor" | "joint" | "joint64" (float64 JointStates
    handed over as roots64: level 0 then carries both reward readings)."""
    return dict(weights=weights, scenes=scenes, seed=seed, B=B, H=H, D=D, W=W, clip=clip, sparse=sparse, table=list(table),
                roots=roots, contraction=contraction, L=L, sim=sim, note=note)


def case_id(c):
    A = c["table"][0] * c["table"][1] + 1
    return "%s-%s-B%d-H%d-D%d-%s%s-A%d-%s%s%s%s" % (
        c["weights"], c["scenes"], c["B"], c["H"], c["D"], ("W%d" % c["W"]) if c["clip"] else "noclip", "-sparse" if c["sparse"] else "",
        A, c["roots"], "" if c["contraction"] == "f32" else "-" + c["contraction"], "" if c["L"] == 2 else "-L%d" % c["L"],
        "" if c["sim"] == "embedded_gaussian" else "-" + c["sim"])


def make_search(c, dev):
    cfg = policy_config("model_predictive_rl", gcn__num_layer=c["L"], gcn__similarity_function=c["sim"],
                        action_space__speed_samples=c["table"][0], action_space__rotation_samples=c["table"][1],
                        model_predictive_rl__planning_depth=c["D"], model_predictive_rl__planning_width=c["W"],
                        model_predictive_rl__do_action_clip=c["clip"], model_predictive_rl__sparse_search=c["sparse"])
    pol = rga.ModelPredictiveRL()
    pol.time_step = 0.25
    pol.configure(cfg)
    pol.load_state_dict(gio.checkpoint("trained", c["L"], "separate", c["sim"]))
    pol.set_time_step(0.25)
    pol.set_phase("test")
    pol.set_device(dev)
    if c["weights"] == "tie":
        with torch.no_grad():
            pol.value_estimator.value_network[-1].weight.zero_()
    pol.contraction_dtype = c["contraction"]
    pol.build_action_space(1.0)
    ts = pol.tree_search()
    assert ts.num_actions == c["table"][0] * c["table"][1] + 1
    return pol, ts


def make_roots(c, dev):
    if c["scenes"] == "dense":
        robot, humans = dense_scenes(np.random.RandomState(c["seed"]), c["B"], c["H"])
    else:
        robot, humans = seeded_scenes(c["seed"], c["B"], c["H"])
    if c["roots"] != "joint64":
        return robot.to(dev), humans.to(dev), None
    rng = np.random.RandomState(c["seed"] + 77)                     # float64 states that are not float32 numbers
    r64, h64 = robot.double(), humans.double()
    r64[:, [0, 1, 5, 6]] += torch.tensor(rng.uniform(-1e-8, 1e-8, (c["B"], 4)))
    h64[:, :, 0:2] += torch.tensor(rng.uniform(-1e-8, 1e-8, (c["B"], c["H"], 2)))
    r64, h64 = r64.to(dev).contiguous(), h64.to(dev).contiguous()
    return r64.float(), h64.float(), (r64, h64)


LEVEL_INPUTS = ("reward", "child_value", "child_robot", "humans_next", "reward_clip")


def search_and_replay(c, dev):
    """Run the search of case `c`, replay it on the host from the device's reward / child_value / child_robot / humans_next arrays and
    compare every other array bit for bit.  Returns (integer arrays of the search, statistics)."""
    pol, ts = make_search(c, dev)
    robot, humans, roots64 = make_roots(c, dev)
    out = ts.search(robot, humans, roots_are_joint_states=c["roots"] != "tensor", roots64=roots64)
    torch.cuda.synchronize()
    D, B = c["D"], c["B"]
    A = ts.num_actions
    Wk = ts.kept_per_node
    dev_lv = []
    for l in range(D):
        arr = ts.level_arrays(l)
        dev_lv.append({k: v.cpu().numpy().copy() for k, v in arr.items() if torch.is_tensor(v)})
        assert arr["n_parents"] == B * Wk ** l
    if c["roots"] == "tensor" or not c["clip"]:
        assert "reward_clip" not in dev_lv[0]
    else:
        assert "reward_clip" in dev_lv[0]
        if c["roots"] == "joint64" and c["scenes"] == "dense":       # the two readings of the same crowded roots do differ
            assert not np.array_equal(dev_lv[0]["reward_clip"], dev_lv[0]["reward"])
    rep = sb.replay([{k: lv.get(k) for k in LEVEL_INPUTS} for lv in dev_lv], ts.gamma_bar, D, c["W"], c["clip"], c["sparse"],
                    ts.groups_np)
    tag = case_id(c)
    for l in range(D):
        got, want = dev_lv[l], rep["levels"][l]
        assert same_bits(got["value1"], want["value1"]), (tag, l, "value1")
        if not np.array_equal(got["keep"], want["keep"]):
            p = int(np.nonzero((got["keep"] != want["keep"]).any(1))[0][0])
            raise AssertionError("%s: level %d keep of parent %d: device %s, replay %s (values %s)"
                                 % (tag, l, p, got["keep"][p].tolist(), want["keep"][p].tolist(),
                                    want["value1"][p, want["keep"][p]].tolist()))
        assert same_bits(got["backup"], want["backup"]), (tag, l, "backup", int((sb.bits(got["backup"]) != sb.bits(want["backup"])).sum()))
        assert np.array_equal(got["best_slot"], want["best_slot"]), (tag, l, "best_slot", int((got["best_slot"] != want["best_slot"]).sum()))
        if l + 1 < D:
            assert same_bits(dev_lv[l + 1]["robot"], want["next_robot"]), (tag, l, "next level's robot rows")
            assert same_bits(dev_lv[l + 1]["humans"], want["next_humans"]), (tag, l, "next level's humans")
    res = {k: out[k].cpu().numpy() for k in ("root_values", "root_kept", "best_action", "best_value")}
    assert same_bits(res["root_values"], rep["root_values"]), (tag, "root_values")
    assert np.array_equal(res["root_kept"], rep["root_kept"]), (tag, "root_kept")
    assert same_bits(res["best_value"], rep["best_value"]), (tag, "best_value")
    assert np.array_equal(res["best_action"], rep["best_action"]), (tag, "best_action", int((res["best_action"] != rep["best_action"]).sum()))
    assert (rep["best_action"] >= 0).all()
    for b in sorted({0, B // 2, B - 1}):                              # best_trajectory follows the best_slots
        traj = ts.best_trajectory(b)
        branch = sb.best_branch(rep, b, Wk)
        assert [t[1] for t in traj[:-1]] == [a for _, _, _, a in branch], (tag, b)
        assert [np.float32(t[2]) for t in traj[:-1]] == [dev_lv[l]["reward"][p, a] for l, p, _, a in branch], (tag, b)
        l, p, _, a = branch[-1]
        assert same_bits(traj[-1][0][0].cpu().numpy().reshape(9), dev_lv[l]["child_robot"][p, a]) and traj[-1][1] is None
    stats = {"cut_in_tie": [], "distinct": []}
    for l in range(D):
        v1 = rep["levels"][l]["value1"]
        stats["distinct"].append(float(np.mean([len(np.unique(row)) > 1 for row in v1])))
        if c["clip"] and c["W"] < A:
            order = sb.descending_order(v1)
            W = c["W"]
            stats["cut_in_tie"].append(float((np.take_along_axis(v1, order[:, W - 1:W], 1) ==
                                              np.take_along_axis(v1, order[:, W:W + 1], 1)).mean()))
    ints = {"best_action": res["best_action"], "root_kept": res["root_kept"]}
    for l in range(D):
        ints["L%d/keep" % l], ints["L%d/best_slot" % l] = dev_lv[l]["keep"], dev_lv[l]["best_slot"]
        h = hashlib.sha1()                                           # the level's inputs to the bookkeeping, as a digest
        for k in ("reward", "reward_clip", "child_value"):
            if k in dev_lv[l]:
                h.update(dev_lv[l][k].tobytes())
        ints["L%d/inputs" % l] = np.frombuffer(h.digest(), np.uint8)
    return ints, stats


# Default dispatch, every configuration; the smallest crowds (H = 3 or 5).  Trained weights on seeded scenes give distinct values,
# the tie weights on dense scenes exact ties at every level.
CONFIG_CASES = [
    case("trained", "seeded", 11, 33, 3, 1, 1, clip=False),
    case("trained", "seeded", 12, 3, 3, 2, 1, clip=False, roots="tensor"),                      # W = A = 81 at both levels
    case("trained", "seeded", 13, 7, 3, 2, 1, clip=False, table=(1, 8)),
    case("trained", "seeded", 14, 20, 3, 2, 1),
    case("trained", "seeded", 15, 48, 5, 2, 2, roots="joint64"),
    case("trained", "seeded", 16, 24, 3, 3, 2, roots="tensor"),
    case("trained", "seeded", 17, 10, 3, 4, 2),
    case("trained", "seeded", 18, 16, 5, 2, 3, roots="joint64"),
    case("trained", "seeded", 19, 12, 3, 2, 5),
    case("trained", "seeded", 20, 6, 3, 3, 5, roots="tensor"),
    case("trained", "seeded", 21, 16, 5, 2, 3, sparse=True),
    case("trained", "seeded", 22, 9, 3, 3, 3, sparse=True, roots="joint64"),
    case("trained", "seeded", 23, 14, 3, 3, 2, table=(1, 8)),
    case("trained", "seeded", 24, 10, 3, 2, 2, table=(6, 16)),
    case("trained", "seeded", 25, 6, 3, 2, 3, table=(12, 16), roots="tensor"),
    case("tie", "dense", 31, 48, 5, 1, 1, clip=False),                                          # 81 tied root values: tail_root's lanes
    case("tie", "dense", 32, 9, 3, 2, 1, clip=False, table=(1, 8), roots="tensor"),
    case("tie", "dense", 33, 5, 3, 2, 1, clip=False),
    case("tie", "dense", 34, 20, 3, 2, 1),
    case("tie", "dense", 35, 20, 3, 4, 2),
    case("tie", "dense", 36, 12, 5, 3, 5, roots="joint64"),
    case("tie", "dense", 37, 16, 5, 2, 3, sparse=True),
    case("tie", "dense", 38, 9, 3, 3, 3, sparse=True, roots="tensor"),
    case("tie", "dense", 39, 8, 3, 2, 2, table=(6, 16)),
    case("tie", "dense", 40, 6, 3, 3, 3, table=(12, 16)),
]


@pytest.mark.parametrize("c", CONFIG_CASES, ids=case_id)
def test_whole_search_is_the_replay(c, dev):
    search_and_replay(c, dev)


@pytest.mark.parametrize("H,D,W", [(5, 3, 2), (3, 2, 3)])
def test_tie_weights_cut_inside_ties_at_every_level(H, D, W, dev):
    """The condition the tie weights are there for, asserted on the device's own arrays: with the value head's last weight zeroed
    at least half of the nodes of every level have their cut at W inside an exact tie, and some nodes hold more than one distinct
    value (the rewards differ).  On the oracle (CPU) the cut fell inside a tie at >= 46 of these 48 roots and at every deeper node."""
    _, stats = search_and_replay(case("tie", "dense", 5, 48, H, D, W), dev)
    assert len(stats["cut_in_tie"]) == D and min(stats["cut_in_tie"]) >= 0.5, stats
    assert max(stats["distinct"]) > 0.0, stats
    report("tie weights, dense_scenes(RandomState(5), 48, %d), D = %d, W = %d: fraction of nodes cut inside a tie per level %s; with "
           "more than one distinct value %s" % (H, D, W, ["%.2f" % x for x in stats["cut_in_tie"]], ["%.2f" % x for x in stats["distinct"]]))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. every form the bookkeeping is compiled into: one child process per environment
# ---------------------------------------------------------------------------------------------------------------------------
BIG = 20011    # roots of the D = 1, A = 9, H = 2 search: more roots per workgroup than one pass of tail_root's loop, last workgroup short

# The same cases under every environment.  Which kernel serves a case depends on the environment (and on the default dispatch's size
# rules); profiles/search_bookkeeping_forms.txt records it from kernel traces.  With the default dispatch on 256 CUs:
#   fused kernel from 1200 child tiles per launch (A = 81: 200 parents); its tail takes the back-up chain from 128 roots (CUs / 2);
#   robot_head_kernel's tail (two-stage pair) takes it from 128 roots; D = 1 always chains.
FORM_CASES = [
    case("tie", "dense", 5, 48, 5, 3, 2, note="below both chain rules: selection in the launch, stand-alone back-up and root"),
    case("tie", "dense", 5, 48, 3, 2, 3, roots="joint64"),
    case("tie", "dense", 51, 120, 5, 3, 2, note="deepest level on the fused kernel (480 parents), 120 roots: no chain"),
    case("tie", "dense", 52, 301, 5, 2, 2, note="fused kernel with the chain; 602 parents in blocks of 4: the last workgroup has one root"),
    case("tie", "dense", 53, 200, 3, 2, 2, table=(1, 8), note="A = 9: 400 tiles, the two-stage pair; 200 roots: chain in the head's tail"),
    case("tie", "dense", 54, 131, 5, 3, 3, sparse=True, note="chain over two back-up steps, sparse"),
    case("tie", "dense", 55, BIG, 2, 1, 1, clip=False, table=(1, 8), roots="tensor", note="many roots per workgroup"),
    case("trained", "seeded", 56, BIG, 2, 1, 1, clip=False, table=(1, 8)),
    case("trained", "seeded", 57, 301, 5, 2, 2, roots="joint64"),
    case("trained", "seeded", 58, 130, 3, 4, 2, roots="tensor", note="chain over three back-up steps (d = 2, 3, 4)"),
    case("tie", "dense", 59, 600, 16, 2, 2, contraction="bf16x6", note="bf16x6, N = 17, 1200 parents at level 1: the level prologue form"),
    case("tie", "dense", 60, 100, 5, 3, 2, contraction="bf16x6", note="bf16x6 fused kernel, no chain"),
    case("trained", "seeded", 61, 600, 16, 2, 2, contraction="bf16x6"),
    case("tie", "dense", 62, 3, 49, 2, 2, L=3, note="deep kernel (N = 50, three layers)"),
    case("tie", "dense", 63, 5, 49, 1, 1, clip=False, L=3),
    case("trained", "seeded", 64, 140, 49, 2, 2, L=3, note="deep kernel, 140 roots: chain"),
    case("tie", "dense", 65, 16, 5, 2, 2, sim="cosine", note="scene kernel family (value rows + robot_head_kernel)"),
    case("trained", "seeded", 66, 150, 5, 2, 2, sim="cosine"),
]

FORMS = {
    "default": {},
    "fused_no_tail": {"RGL_FUSED_NO_TAIL": "1"},
    "fused_forced": {"RGL_CHILDREN_FUSED": "1"},
    "two_stage": {"RGL_CHILDREN_TWO_STAGE": "1"},
    "no_level_prologue": {"RGL_LEVEL_PROLOGUE": "0"},
    "deep_head_outside": {"RGL_DEEP_FUSE_HEAD": "0"},
    "generic": {"RGL_FORCE_GENERIC": "1"},
}


def _source_constant(path, pattern):
    import re
    with open(os.path.join(ROOT, "relationalgraphlearning_amd", "csrc", path)) as f:
        m = re.search(pattern, f.read())
    assert m, (path, pattern)
    return int(m.group(1))


def roots_per_workgroup(B, dev):
    """(fused kernel, robot_head_kernel) roots per workgroup of a D = 1 search of B roots, and the roots one pass of their tail_root
    loops holds, with the block sizes and slot counts read from the sources that set them: plan_items (rgl_fused.hip,
    `k = (P + n_cu - 1) / n_cu`) hands ceil(P / CUs) parents to a fused workgroup of kFusedWaves waves (rgl_fused.h); head_args_for
    (rgl_head_body.h, `k = (P + slots - 1) / slots`) ceil(P / slots) to a head workgroup of kHeadThreads threads, slots being what
    launch_head_rows passes for the shipped head (rgl_head.hip, `hv == 0 ? 512 : 256`); tail_root scores a root on kRootLanes
    lanes (rgl_tail.h).  The kernel record (profiles/search_bookkeeping_forms.txt) shows the launches these sizes produce."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    fused_threads = 64 * _source_constant("rgl_fused.h", r"constexpr int kFusedWaves = (\d+);")
    head_threads = _source_constant("rgl_head_body.h", r"constexpr int kHeadThreads = (\d+);")
    head_slots = _source_constant("rgl_head.hip", r"hv == 0 \? (\d+) : \d+, &ha, &chain")
    lanes = _source_constant("rgl_tail.h", r"constexpr int kRootLanes = (\d+);")
    return -(-B // cus), -(-B // head_slots), fused_threads // lanes, head_threads // lanes


def child_main(out, separators=False):
    """Entry point of the child processes: every FORM_CASES search under this process's environment, each against the replay; the
    integer arrays of the tie-weight cases (and a digest of each level's inputs) are saved for the comparison across forms.  `separators`: launch one recognisable
    kernel (torch's erfinv) before every case, so that a kernel trace of the process can be cut into cases."""
    dev = torch.device("cuda:0")
    sep = torch.full((64,), 0.5, device=dev)
    res = {}
    for i, c in enumerate(FORM_CASES):
        if separators:
            torch.erfinv(sep)
        ints, _ = search_and_replay(c, dev)
        if c["weights"] == "tie":
            for k, v in ints.items():
                res["%d/%s" % (i, k)] = v
    torch.cuda.synchronize()
    np.savez(out, **res)
    print("OK %d searches equal to the replay" % len(FORM_CASES))


_form_results = {}


def run_form(name, tmp_path_factory):
    """The child of form `name`, started ONCE per session: a failure is kept and raised again for every test that needs the form
    (a child that failed is not launched a second time)."""
    if name not in _form_results:
        out = str(tmp_path_factory.mktemp("forms") / (name + ".npz"))
        code = "import sys\nfrom tests.test_search_bookkeeping import child_main\nchild_main(sys.argv[1])\n"
        try:
            res = subprocess.run([sys.executable, "-c", code, out], cwd=ROOT, env=dict(os.environ, **FORMS[name]), capture_output=True,
                                 text=True, timeout=600)
            if res.returncode != 0 or "OK" not in res.stdout:
                raise AssertionError("form %s: child ended with %s\n%s" % (name, res.returncode, res.stdout[-2000:] + res.stderr[-4000:]))
            _form_results[name] = dict(np.load(out))
        except Exception as e:              # also a timeout: remembered, not retried
            _form_results[name] = e
    if isinstance(_form_results[name], Exception):
        raise AssertionError("the child process of form %s failed (started once): %s" % (name, _form_results[name]))
    return _form_results[name]


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_is_the_replay_and_the_forms_agree(form, dev, tmp_path_factory):
    """FORM_CASES in a child process under the form's environment: every search equals the replay (asserted in the child).  Across
    forms, with the tie weights, the same roots must give the default dispatch's keep / best_slot / best_action arrays: V is the
    last bias whatever kernel computes it, and the rewards come from the same float64 kernel on the same states.  Asserted in
    full -- every level's reward / child_value arrays bit-equal to the default's (by digest) and every integer array identical, in
    every case -- for every form but RGL_FORCE_GENERIC=1.  That switch also replaces the state predictor's kernel, so the humans
    it moves, and with them the rewards below the root level, differ in their last bits (network arithmetic, not bookkeeping):
    there level 0's inputs and kept actions are held identical in every case, the depth-1 cases in full, and the deeper cases in
    full wherever the inputs came out bit-equal."""
    fused_k, head_k, fused_pass, head_pass = roots_per_workgroup(BIG, dev)
    assert fused_k > fused_pass and head_k > head_pass and BIG % fused_k and BIG % head_k    # several passes; a short last workgroup
    got = run_form(form, tmp_path_factory)
    base = run_form("default", tmp_path_factory)
    assert sorted(got) == sorted(base) and len(got) > 0
    ties = [i for i, c in enumerate(FORM_CASES) if c["weights"] == "tie"]
    full = compared = 0
    for i in ties:
        D = FORM_CASES[i]["D"]
        assert np.array_equal(got["%d/L0/inputs" % i], base["%d/L0/inputs" % i]), (form, FORM_CASES[i], "level 0 inputs differ")
        same_inputs = all(np.array_equal(got["%d/L%d/inputs" % (i, l)], base["%d/L%d/inputs" % (i, l)]) for l in range(D))
        full += same_inputs
        keys = [k for k in sorted(base) if k.startswith("%d/" % i)] if same_inputs else ["%d/L0/keep" % i, "%d/root_kept" % i]
        for k in keys:
            assert got[k].dtype == base[k].dtype and np.array_equal(got[k], base[k]), (form, k, FORM_CASES[i])
            compared += 1
    n_depth1 = sum(FORM_CASES[i]["D"] == 1 for i in ties)
    if form == "generic":
        assert full >= n_depth1 > 0, (form, full, len(ties))           # depth 1 has no level below the roots
    else:
        assert full == len(ties), (form, full, len(ties))              # a form that moves a reward or a value by a bit fails here
    report("search bookkeeping, form %s (%s): %d searches equal to the replay; %d of %d tie-weight cases with inputs bit-equal to the "
           "default dispatch's at every level, %d arrays identical" % (form, " ".join("%s=%s" % kv for kv in FORMS[form].items()) or "no switch",
                                                                       len(FORM_CASES), full, len(ties), compared))


if __name__ == "__main__":
    child_main(sys.argv[1], separators="--separators" in sys.argv)
