"""Path G's prepare, rotate and select steps (csrc/rgl_rotate.h: rotate_row; csrc/rgl_onestep.h: gcn_prepare_kernel,
onestep_select_kernel) against the host replay (tests/path_g_steps.py), BIT FOR BIT wherever no libm is involved.  The select step
is the one SARL's search runs too: the decision tests run it behind both networks, and with SARL also hold the attention row it
gathers.

The device's atan2f / cosf / sinf are not the host's, so the tests read the device's own trig back through probe rows -- a row with
velocity (1, 0) returns c and -sn exactly, a unicycle row with theta = 0 returns -rot -- hand it to the replay, and demand bits for
everything else; the recovered trig itself is held to the 2e-6 of test_path_g_rotate against float64.  The replay is pinned to the
oracle by tests/test_path_g_steps_cpu.py, which also counts the teeth of every family used here; nothing computed by the code under
test is an expectation.  The same reward families run through path M's reward step (mprl_estimate_reward_f32).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import relationalgraphlearning_amd as rga
from oracle import rgl_oracle as orc
from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd.nets import _stream, batched_transposes
from relationalgraphlearning_amd.rollout import GcnSearch, SarlSearch, prepare_scenes
from tests import path_g_steps as pg
from tests.helpers import JS, make_gcn_policy, make_mprl_policy
from tests.test_gpu_parity import report
from tests.test_sarl_gpu import make_policy as make_sarl_policy

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DT, GAMMA = 0.25, 0.9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(pg.bits(got), pg.bits(want))


def same_but_zero_signs(got, want):
    """Bit patterns equal, the two zeros taken as one (rotated columns: 0 * c + 0 * sn carries the signs of c and sn)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(((pg.bits(got) == pg.bits(want)) | ((got == 0) & (want == 0))).all())


def assert_features(got13, want13, tag, lo=0):
    """Columns lo.. of the 13 features: trig-free ones bit for bit, rotated ones (and theta) bit for bit up to the sign of a zero."""
    assert got13.shape == want13.shape
    for k in range(lo, lo + got13.shape[-1]):
        g, w = got13[..., k - lo], want13[..., k - lo]
        ok = same_bits(g, w) if k in pg.TRIG_FREE else same_but_zero_signs(g, w)
        assert ok, (tag, "column %d" % k, int((pg.bits(g) != pg.bits(w)).sum()), float(np.abs(g.astype(F64) - w).max()))


def holonomic_table():
    return orc.cadrl_action_space(orc.OracleConfig(), 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# gcn_rotate_f32
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 255, 256, 257, 5000])
def test_rotate_is_the_replay_given_the_devices_trig(R, dev):
    """R test rows (dense scenes, robot at goal, axis-aligned goals, coordinates of order 1e4, denormal goal offsets; see
    path_g_steps.rotate_rows), each with its two probe rows, in one launch of 3R rows: all 13 columns of every row equal the
    replay's given the (rot, c, sn) the probes return, in both kinematics; that trig is within 2e-6 of float64's."""
    rows = pg.rotate_rows(R, seed=5 + R)
    three = pg.with_probes(rows)
    x = torch.tensor(three).to(dev)
    got = {kin: rga.rotate(x, kin).cpu().numpy() for kin in ("holonomic", "unicycle")}
    rot, c, sn = pg.trig_from_probes(got["holonomic"], got["unicycle"])
    for kin in got:
        want = pg.rotate(three, kin, tuple(np.repeat(t, 3) for t in (rot, c, sn)))
        assert_features(got[kin], want, (R, kin))
    dx, dy = pg.goal_offsets(rows)
    rot64 = np.arctan2(dy.astype(F64), dx.astype(F64))
    err = max(float(np.abs(rot - rot64).max()), float(np.abs(c - np.cos(rot64)).max()), float(np.abs(sn - np.sin(rot64)).max()))
    assert err <= 2e-6, err
    report("path G rotate, R = %d (+ 2R probe rows): 13 columns x 2 kinematics equal to the replay bit for bit given the device's "
           "trig; max |d(rot, c, sn)| vs float64 = %.2e" % (R, err))


# ---------------------------------------------------------------------------------------------------------------------------
# gcn_prepare_f32
# ---------------------------------------------------------------------------------------------------------------------------
def prepare_raw(robot, humans, table, kinematics, dev, r64=None, h64=None):
    """gcn_prepare_f32 with each of the two float64 pointers set or not on its own (rollout.prepare_scenes sets both or none)."""
    robot, humans = torch.tensor(robot).to(dev), torch.tensor(humans).to(dev)
    tab = torch.tensor(np.asarray(table, F64).reshape(-1, 2)).to(dev).contiguous()
    keep = [torch.tensor(x).to(dev).contiguous() if x is not None else None for x in (r64, h64)]
    B, H, A = robot.shape[0], humans.shape[1], tab.shape[0]
    pl = nat.GcnPlanner()
    pl.kinematics, pl.num_actions, pl.time_step, pl.actions = nat.KINEMATICS[kinematics], A, DT, tab.data_ptr()
    if keep[0] is not None:
        pl.root_robot_f64 = keep[0].data_ptr()
    if keep[1] is not None:
        pl.root_humans_f64 = keep[1].data_ptr()
    self6 = torch.empty(B * A, 6, dtype=torch.float32, device=dev)
    hum7 = torch.empty(B * A, H, 7, dtype=torch.float32, device=dev)
    reward = torch.empty(B * A, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().gcn_prepare_f32(C.byref(pl), robot.data_ptr(), humans.data_ptr(), B, H, self6.data_ptr(), hum7.data_ptr(),
                                            reward.data_ptr(), _stream()), "gcn_prepare_f32")
        torch.cuda.synchronize()
    return self6.cpu().numpy(), hum7.cpu().numpy(), reward.cpu().numpy()


def run_prepare(robot, humans, table, kinematics, dev, roots64=None):
    r64 = None if roots64 is None else tuple(torch.tensor(x).to(dev).contiguous() for x in roots64)
    out = prepare_scenes(torch.tensor(robot).to(dev), torch.tensor(humans).to(dev), table, kinematics, DT, r64)
    return tuple(t.cpu().numpy() for t in out)


PREPARE_H = (1, 2, 3, 5, 63, 64, 65, 85, 86, 127)         # workgroups of 256, 256, 255, 255, 252, 256, 195, 255, 172, 254 threads


def batch_for(A, H):
    """The smallest B >= 3 whose B * A * H threads do not fill whole workgroups of (256 // H) * H.  None exists when 256 // H
    divides A (81 actions and H = 65 or 85: three pairs per workgroup; 256 actions and H a power of two)."""
    threads = (256 // H) * H
    for B in range(3, 12):
        if (B * A * H) % threads:
            return B, True
    return 3, False


def prepare_tables():
    rng = np.random.RandomState(41)
    sp, an = rng.uniform(0.0, 1.0, 256), rng.uniform(0, 2 * np.pi, 256)
    return {"A81": holonomic_table(), "A1": np.array([[0.3125, -0.21]]), "A256": np.stack([sp * np.cos(an), sp * np.sin(an)], axis=1)}


@pytest.mark.parametrize("float64_roots", [False, True], ids=["f32_roots", "roots64"])
def test_prepare_holonomic_is_the_replay(float64_roots, dev):
    """self6, hum7 and reward of every (root, action, human) equal the replay's bit for bit, the probe human of every scene handing
    back c and sn of its (root, action) pair: H in PREPARE_H (every workgroup grouping), A = 81 / 1 / 256, dense scenes, a
    partly filled last workgroup wherever the sizes allow one."""
    rng = np.random.RandomState(4100 + int(float64_roots))
    n = {"collisions": 0, "discomfort": 0, "goals": 0, "pairs": 0, "launches": 0, "partial": 0}
    for H in PREPARE_H:
        for name, table in prepare_tables().items():
            A = table.shape[0]
            B, partial = batch_for(A, H)
            if A == 1:                                                    # more than a handful of pairs
                B, partial = 7 * B, (7 * B * H) % ((256 // H) * H) != 0
            assert partial == (A % (256 // H) != 0), (name, H)
            robot, humans, r64 = pg.probe_scenes(rng, B, H, float64_roots)
            self6, hum7, reward = run_prepare(robot, humans, table, "holonomic", dev, r64)
            trig = pg.trig_from_probe_human(hum7, B, A)
            _, want6, want7, want_r = pg.prepare(robot, humans, table, "holonomic", DT, r64, trig)
            tag = (H, name, B)
            assert_features(self6, want6[:, :6], tag + ("self6",))
            assert_features(hum7, want7, tag + ("hum7",), lo=6)
            assert same_bits(reward, want_r), tag + ("reward", int((pg.bits(reward) != pg.bits(want_r)).sum()))
            n["collisions"] += int((want_r == -0.25).sum()); n["goals"] += int((want_r == 1).sum())
            n["discomfort"] += int(((want_r < 0) & (want_r > -0.25)).sum())
            n["pairs"] += B * A; n["launches"] += 1; n["partial"] += int(partial)
    assert min(n["collisions"], n["discomfort"], n["goals"]) > 100, n
    report("path G prepare, holonomic, %s: %d launches (H in %s, A in {81, 1, 256}; %d with a partly filled last workgroup), %d pairs "
           "equal to the replay bit for bit (%d collisions, %d discomfort values, %d goals)"
           % ("float64 roots" if float64_roots else "float32 roots", n["launches"], list(PREPARE_H), n["partial"], n["pairs"],
              n["collisions"], n["discomfort"], n["goals"]))


def test_prepare_with_one_float64_pointer_is_none_set(dev):
    """Only one of root_robot_f64 / root_humans_f64: the float32 rows are read, exactly as with none."""
    robot, humans, r64 = pg.probe_scenes(np.random.RandomState(43), 9, 5, True)
    table = holonomic_table()
    none = prepare_raw(robot, humans, table, "holonomic", dev)
    both = prepare_raw(robot, humans, table, "holonomic", dev, r64[0], r64[1])
    assert not same_bits(none[2], both[2]) or not same_bits(none[1], both[1])           # the float64 roots do matter here
    for one in ((r64[0], None), (None, r64[1])):
        got = prepare_raw(robot, humans, table, "holonomic", dev, *one)
        assert all(same_bits(g, w) for g, w in zip(got, none))


def test_reward_thresholds_of_path_g(dev):
    """The exact-contact, goal-boundary and collision-beats-goal families through roots64: rewards bit for bit.  On the CPU a
    contracted evaluation turns 170 of the 4096 contacts into collisions (test_path_g_steps_cpu.py)."""
    table = holonomic_table()
    robot, humans, _, mine = pg.contact_family(table)
    got = run_prepare(robot.astype(F32), humans.astype(F32), table, "holonomic", dev, (robot, humans))[2]
    nr, nh = pg.propagate(None, None, table, "holonomic", DT, (robot, humans))
    want = pg.reward_of(*pg.clearances(nr, nh), nr[:, :, 4], DT)
    contact = want[np.arange(len(mine)), mine]
    assert (contact == (0.0 - 0.2) * 0.5 * DT).all()
    wrong = pg.bits(got.reshape(want.shape)) != pg.bits(want.astype(F32))
    assert not wrong.any(), ("exact contact", int(wrong.sum()), int((got.reshape(want.shape)[np.arange(len(mine)), mine] == -0.25).sum()))
    robot, humans, tab4, k, reach = pg.goal_boundary_family()
    got = run_prepare(robot.astype(F32), humans.astype(F32), tab4, "holonomic", dev, (robot, humans))[2].reshape(-1, 4)
    want = np.zeros((len(k), 4), F32)
    want[np.arange(len(k)), k] = reach
    assert same_bits(got, want), ("goal boundary", np.nonzero(got != want))
    robot, humans, tab4, want = pg.collision_beats_goal_family()
    got = run_prepare(robot.astype(F32), humans.astype(F32), tab4, "holonomic", dev, (robot, humans))[2].reshape(1, 4)
    assert same_bits(got, want.astype(F32)), got
    report("path G reward thresholds through roots64: 4096 exact contacts x 81 actions (clearance 0: -0.025, never -0.25), %d goal "
           "distances equal to the radius / one ulp inside, collision beats goal: bit for bit" % len(k))


def test_prepare_unicycle_is_the_replay_to_the_device_trig(dev):
    """Unicycle: propagate calls the float64 cos / sin, the device's differ from the host's by a few 1e-16, so (a) the rewards must
    be the replay's bit for bit wherever every decision margin of the replay exceeds 1e-9 -- everywhere, for this family (asserted
    here and on the CPU) -- and (b) the features, given the probe's c / sn, stay within the project's unicycle bound of 1e-6 (theta
    against the host's atan2f: its rot cannot be read back)."""
    table = orc.cadrl_action_space(orc.OracleConfig(kinematics="unicycle"), 1.0)
    A = table.shape[0]
    pairs = exact = total = 0
    worst = 0.0
    for B, H, seed in pg.UNICYCLE_CASES:
        robot, humans, _ = pg.probe_scenes(np.random.RandomState(seed), B, H)
        self6, hum7, reward = run_prepare(robot, humans, table, "unicycle", dev)
        host = lambda dy, dx: (np.arctan2(dy, dx), np.cos(np.arctan2(dy, dx)), np.sin(np.arctan2(dy, dx)))
        joint = pg.prepare(robot, humans, table, "unicycle", DT, None, host)[0]
        dx, dy = pg.goal_offsets(joint[:, :, 0])
        _, c, sn = pg.trig_from_probe_human(hum7, B, A)
        _, want6, want7, want_r = pg.prepare(robot, humans, table, "unicycle", DT, None, (np.arctan2(dy, dx).astype(F32), c, sn))
        nr, nh = pg.propagate(robot, humans, table, "unicycle", DT)
        d, gd = pg.clearances(nr, nh)
        safe = np.minimum.reduce(pg.margins(d, gd, nr[:, :, 4])).reshape(-1) > 1e-9
        assert safe.all()
        assert same_bits(reward[safe], want_r[safe]), (B, H, int((pg.bits(reward) != pg.bits(want_r)).sum()))
        for got, want in ((self6, want6), (hum7, want7)):
            worst = max(worst, float(np.abs(got.astype(F64) - want).max()))
            exact += int((pg.bits(got) == pg.bits(want)).sum() + ((got == 0) & (want == 0) & (pg.bits(got) != pg.bits(want))).sum())
            total += got.size
        pairs += B * A
    assert worst <= 1e-6, worst
    report("path G prepare, unicycle: %d pairs, rewards bit for bit (no pair within 1e-9 of a threshold); features within %.2e of the "
           "replay given the device's c / sn (%d of %d values bit-equal)" % (pairs, worst, exact, total))


# ---------------------------------------------------------------------------------------------------------------------------
# path M's reward step on its contact family
# ---------------------------------------------------------------------------------------------------------------------------
def test_reward_thresholds_of_path_m(dev):
    """mprl_estimate_reward_f32 with float64 joint-state roots on the segment-distance contact family: the oracle's rewards
    (estimate_reward_batched on the float64 arrays, root=True) bit for bit.  On the CPU a contracted evaluation turns 212 of the
    4096 contacts into collisions."""
    cfg = orc.OracleConfig()
    table = orc.mprl_action_space(cfg, 1.0)[0]
    pol = make_mprl_policy("trained", D=1, device=dev)
    pol.build_action_space(1.0)
    ts = pol.tree_search()
    assert np.array_equal(ts.actions_np, table)
    robot, humans, _, mine = pg.contact_family(table, segment=True)
    r64, h64 = torch.tensor(robot).to(dev).contiguous(), torch.tensor(humans).to(dev).contiguous()
    _, reward = ts.estimate_reward(r64.float(), h64.float(), parents_are_joint_states=True, roots64=(r64, h64))
    want = orc.estimate_reward_batched(robot, humans, table, cfg, root=True)
    got = reward.cpu().numpy()
    contact = want[np.arange(len(mine)), mine]
    assert (contact == (0.0 - 0.2) * 0.5 * DT).all()
    wrong = pg.bits(got) != pg.bits(want.astype(F32))
    assert not wrong.any(), (int(wrong.sum()), int((got[np.arange(len(mine)), mine] == -0.25).sum()))
    report("path M reward step, 4096 exact segment contacts x 81 actions through roots64: bit for bit (no contact read as a collision)")


# ---------------------------------------------------------------------------------------------------------------------------
# gcn_predict_f32's decision
# ---------------------------------------------------------------------------------------------------------------------------
NETWORKS = ("gcn", "sarl")


def constant_search(c, table, dev, kinematics="holonomic", network="gcn"):
    """A one-step search whose value network answers c for every scene: last layer's weight zero, bias c.  "sarl": the attention
    network on 13-wide rows (no maps), whose attention weights stay what the scenes make them."""
    if network == "sarl":
        pol = make_sarl_policy(dev, kinematics, 13, True, "plain")
        last = [m for m in pol.model.mlp3 if isinstance(m, torch.nn.Linear)][-1]
    else:
        pol = make_gcn_policy(device=dev)
        last = pol.model.value_net[-1]
    with torch.no_grad():
        last.weight.zero_()
        last.bias.fill_(c)
    return pol, (SarlSearch if network == "sarl" else GcnSearch)(pol.model, table, kinematics, DT, GAMMA)


def scene_attention(search, robot, humans, dev):
    """(B, A, H) attention weights of sarl_value_f32 on the B x A candidate scenes of prepare_scenes, evaluated on their own."""
    r, h = torch.tensor(robot).to(dev), torch.tensor(humans).to(dev)
    self6, hum7, _ = prepare_scenes(r, h, search.actions_np, search.kinematics, DT)
    S, H = hum7.shape[0], hum7.shape[1]
    rows = torch.cat([self6[:, None, :].expand(S, H, 6), hum7], dim=2).contiguous()
    value = torch.empty(S, dtype=torch.float32, device=dev)
    att = torch.empty(S, H, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        pl = search.planner(dev, H)
        ws = torch.empty(nat.lib().sarl_value_workspace_bytes_for(C.byref(pl), S, H), dtype=torch.uint8, device=dev)
        nat.check(nat.lib().sarl_value_f32(C.byref(pl), rows.data_ptr(), None, None, None, S, 1, H, ws.data_ptr(), ws.numel(),
                                           value.data_ptr(), att.data_ptr(), _stream()), "sarl_value_f32")
        torch.cuda.synchronize()
    return att.cpu().numpy().reshape(robot.shape[0], -1, H)


def run_search(search, robot, humans, dev):
    """(action_values, best_action, best_value) of one search.  SARL: last_attention must be, bit for bit, row best_action of the
    attention the value network returns for the candidate scenes on their own, and all zeros where no action was chosen."""
    vals, best = search.search(torch.tensor(robot).to(dev), torch.tensor(humans).to(dev))
    torch.cuda.synchronize()
    best = best.cpu().numpy()
    if isinstance(search, SarlSearch):
        att = scene_attention(search, robot, humans, dev)
        want = np.where(best[:, None] >= 0, att[np.arange(len(best)), np.maximum(best, 0)], F32(0))
        got = search.last_attention.cpu().numpy()
        assert same_bits(got, want), ("last_attention", int((pg.bits(got) != pg.bits(want)).sum()))
        assert (np.abs(want[best >= 0].astype(F64).sum(1) - 1.0) < 1e-5).all()                  # softmax rows, not a cleared buffer
    return vals.cpu().numpy(), best, search.last_best_value.cpu().numpy()


def replay_decision(robot, humans, table, c, disc=None):
    host = lambda dy, dx: (np.arctan2(dy, dx), np.cos(np.arctan2(dy, dx)), np.sin(np.arctan2(dy, dx)))      # the rewards take no trig
    rew = pg.prepare(robot, humans, table, "holonomic", DT, None, host)[3].reshape(robot.shape[0], -1)
    return pg.decide(rew, np.full(rew.shape, c, F32), GAMMA, DT, robot[:, 7], disc)


def assert_decision(got, want, tag):
    assert np.array_equal(got[1], want[1]), (tag, "best_action", got[1].tolist()[:40], want[1].tolist()[:40])
    assert got[1].dtype == np.int32
    nan_eq = lambda a, b: same_bits(np.where(np.isnan(a), F32(np.nan), a), np.where(np.isnan(b), F32(np.nan), b))
    assert nan_eq(got[0], want[0]), (tag, "action_values")
    assert same_bits(got[2], want[2]), (tag, "best_value")


@pytest.mark.parametrize("A,network", [pytest.param(A, "gcn", id=str(A)) for A in (1, 2, 15, 16, 17, 31, 32, 33, 81, 256)]
                         + [pytest.param(33, "sarl", id="33-sarl")])
def test_every_action_slot_can_win(A, network, dev):
    """A scenes in one launch, scene b's goal on the end point of action b of a dyadic table, robot radius 1/64: only action b
    reaches.  best_action is arange(A), best_value float32(1 + disc * c), every action value the replay's, bit for bit; with
    dt * v_pref = 0 (disc = 1) and = 1 (disc = gamma)."""
    table = pg.dyadic_table(A)
    c = 0.375
    _, search = constant_search(c, table, dev, network=network)
    for v_pref, disc in ((0.0, 1.0), (4.0, GAMMA)):
        robot, humans = pg.lane_scenes(table, list(range(A)), 5, v_pref)
        want = replay_decision(robot, humans, table, c)
        assert np.array_equal(want[1], np.arange(A)) and (want[2] == F32(1.0 + disc * F64(F32(c)))).all()
        assert ((want[0] == want[0].max(1, keepdims=True)).sum(1) == 1).all()
        assert_decision(run_search(search, robot, humans, dev), want, (A, v_pref))
    report("%s decision, A = %d: every action wins its scene (16 lanes x %d slots), values bit for bit at disc = 1 and gamma"
           % (network, A, -(-A // 16)))


@pytest.mark.parametrize("network", NETWORKS)
def test_ties_go_to_the_lower_index(network, dev):
    """Duplicate table rows k1 < k2, both reaching: k2 in a lower lane than k1 (17 / 32), in the same lane (3 / 19), neighbours
    (5 / 6), both in the last slots (64 / 80); a scene where nothing reaches answers action 0."""
    dup = [(17, 32), (3, 19), (5, 6), (64, 80)]
    table = pg.dyadic_table(81, dup)
    c = -0.125
    _, search = constant_search(c, table, dev, network=network)
    targets = [k1 for k1, _ in dup] + [k2 for _, k2 in dup] + [-1]
    robot, humans = pg.lane_scenes(table, targets, 5, 4.0)
    want = replay_decision(robot, humans, table, c)
    assert want[1].tolist() == [17, 3, 5, 64, 17, 3, 5, 64, 0]
    assert ((want[0] == want[0].max(1, keepdims=True)).sum(1)).tolist() == [2] * 8 + [81]
    assert_decision(run_search(search, robot, humans, dev), want, "ties")
    report("%s decision, exact ties across lanes, within a lane and between neighbours: the lower index wins; 81 equal values: action 0"
           % network)


@pytest.mark.parametrize("c,action,network", [pytest.param(c, action, network, id=("" if network == "gcn" else "sarl-") + name)
                                              for network in NETWORKS
                                              for name, c, action in (("nan", float("nan"), -1), ("inf", float("inf"), 0), ("-inf", float("-inf"), -1))])
def test_non_finite_values(c, action, network, dev):
    """V = NaN: no action beats -inf -> -1, best_value 0, NaN action values; GCN.predict (SARL inherits it) raises as upstream
    does, predict_batch returns -1.  V = +inf: action 0.  V = -inf: -1.  SARL: the attention row of a root without an action is zeros."""
    table = holonomic_table()
    pol, search = constant_search(c, table, dev, network=network)
    robot, humans, _ = pg.probe_scenes(np.random.RandomState(47), 17, 5)
    want = replay_decision(robot, humans, table, c)
    assert (want[1] == action).all() and (action >= 0 or (want[2] == 0).all())
    got = run_search(search, robot, humans, dev)
    assert_decision(got, want, c)
    if np.isnan(c):
        assert np.isnan(got[0]).all()
    pol.build_action_space(1.0)
    pa, pv = pol.predict_batch(torch.tensor(robot).to(dev), torch.tensor(humans).to(dev))
    assert (pa.cpu().numpy() == action).all() and same_bits(pv.cpu().numpy(), want[2])
    b = int(np.argmax(np.hypot(robot[:, 5] - robot[:, 0], robot[:, 6] - robot[:, 1])))       # a robot that is not at its goal yet
    if action < 0:
        with pytest.raises(ValueError, match="not well trained"):
            pol.predict(JS(robot[b], humans[b]))
    else:
        assert pol.predict(JS(robot[b], humans[b])) == pol.action_space[0]


@pytest.mark.parametrize("network", NETWORKS)
def test_predict_runs_in_exactly_its_workspace(network, dev):
    """gcn_predict_f32 / sarl_predict_f32 on a buffer of exactly their size query: the decision of the search object (which hands
    over a buffer of its own), bit for bit; one byte less: RGL_ERR_WORKSPACE (tests/test_host_cpu.py holds the sizes themselves)."""
    table = holonomic_table()
    _, search = constant_search(0.375, table, dev, network=network)
    robot, humans, _ = pg.probe_scenes(np.random.RandomState(49), 17, 5)
    want = run_search(search, robot, humans, dev)
    r, h = torch.tensor(robot).to(dev), torch.tensor(humans).to(dev)
    B, H, A = 17, 5, table.shape[0]
    lib = nat.lib()
    vals, best, best_value = search._outputs(B, dev)
    att = torch.empty(B, H, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if network == "sarl":
            pl = search.planner(dev, H)
            need = lib.sarl_predict_workspace_bytes(C.byref(pl), B, H)
            call = lambda ws, n: lib.sarl_predict_f32(C.byref(pl), r.data_ptr(), h.data_ptr(), B, H, ws.data_ptr(), n, vals.data_ptr(),
                                                      best.data_ptr(), best_value.data_ptr(), att.data_ptr(), _stream())
        else:
            pl = search._fill_search(nat.GcnPlanner(), dev, B, H, None)
            with batched_transposes():
                pl.graph, pl.value_head = search.model.descriptor(), search.model.head_descriptor()
            need = lib.gcn_predict_workspace_bytes(B, H, A)
            call = lambda ws, n: lib.gcn_predict_f32(C.byref(pl), r.data_ptr(), h.data_ptr(), B, H, ws.data_ptr(), n, vals.data_ptr(),
                                                     best.data_ptr(), best_value.data_ptr(), _stream())
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        assert call(ws, need - 1) == -4
        nat.check(call(ws, need), "predict")
        torch.cuda.synchronize()
    assert_decision((vals.cpu().numpy(), best.cpu().numpy(), best_value.cpu().numpy()), want, network)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 1000])
def test_decisions_over_batch_sizes(B, dev):
    """Dense scenes, 81 actions, V = c: rewards tie all over the table, so the first maximum is asked of every root; 16 roots per
    workgroup.  dt * v_pref = 1: bit for bit.  The general exponent (v_pref = 1): the device's pow may return the host's
    gamma^0.25 or one of its float64 neighbours -- one of the three must explain every value of the launch."""
    table = holonomic_table()
    c = 0.375
    _, search = constant_search(c, table, dev)
    robot, humans, _ = pg.probe_scenes(np.random.RandomState(4800 + B), B, 5)
    robot[:, 7] = 4.0
    want = replay_decision(robot, humans, table, c)
    assert_decision(run_search(search, robot, humans, dev), want, B)
    tied = int(((want[0] == want[0].max(1, keepdims=True)).sum(1) > 1).sum())
    robot[:, 7] = 1.0
    got = run_search(search, robot, humans, dev)
    host = pg.discount(GAMMA, DT, robot[:, 7])
    explained = []
    for disc in (host, np.nextafter(host, 0.0), np.nextafter(host, 2.0)):
        w = replay_decision(robot, humans, table, c, disc)
        explained.append(same_bits(got[0], w[0]) and np.array_equal(got[1], w[1]) and same_bits(got[2], w[2]))
    assert any(explained), explained
    report("path G decision, B = %d dense scenes: bit for bit at dt * v_pref = 1 (%d roots with a tied maximum); general exponent "
           "explained by the host's pow or a float64 neighbour: %s" % (B, tied, explained))
