"""Host replay of the tree search's bookkeeping (csrc/rgl_tail.h): one-step values, top-w clipping, the V_planning back-up
and the root's first maximum, in numpy float32 -- every operation an individually rounded float32 operation, as on the device.

This module is the DEFINITION of that bookkeeping for the tests.  It is written from the reference's
arithmetic (crowd_nav/policy/model_predictive_rl.py:228-231, :242-269, :271-302) and pinned to the oracle and to the reference's
fixtures by tests/test_search_bookkeeping_cpu.py; nothing in it comes from the kernels.  Given the `reward` / `child_value` /
`child_robot` / `humans_next` arrays a search left in its workspace it reproduces every other array bit for bit.

The order of a row of one-step values: numbers by descending value, NaNs after every number, the lower index first among equal
values (-0.0 == +0.0 is a tie) and among NaNs.  numpy only; no torch operation.
"""
import numpy as np

F32 = np.float32


def one_step_values(sel, child_value, gamma_bar):
    """value1 = sel + g * child_value, both operations rounded to float32 (g = float32(gamma_bar))."""
    g = F32(gamma_bar)
    with np.errstate(all="ignore"):
        return (np.asarray(sel, F32) + g * np.asarray(child_value, F32)).astype(F32)


def descending_order(values):
    """(P,A) float32 -> (P,A) indices: numbers by descending value, then the NaNs; lower index first among equals."""
    v = np.asarray(values, F32)
    nan = np.isnan(v)
    key = np.where(nan, 0.0, -v.astype(np.float64)) + 0.0           # + 0.0: the two zeros are one key
    idx = np.broadcast_to(np.arange(v.shape[1]), v.shape)
    return np.lexsort((idx, key, nan), axis=1)                        # last key first: NaN flag, value, index


def select(values, width, clip=True, sparse=False, groups=None):
    """`keep` (P,W) int32 of a level.  Clipping off: every action in index order.  Clipping on: the first `width` of the order;
    sparse: the first action of each group id not yet taken along that order, and when the groups run out before `width` the
    rest of the row repeats the last action kept."""
    v = np.asarray(values, F32)
    P, A = v.shape
    if not clip:
        return np.tile(np.arange(A, dtype=np.int32), (P, 1))
    order = descending_order(v)
    if not sparse:
        return order[:, :width].astype(np.int32)
    groups = np.asarray(groups)
    keep = np.zeros((P, width), np.int32)
    for p in range(P):
        seen, row = set(), []
        for a in order[p]:
            gid = int(groups[a])
            if gid in seen:
                continue
            seen.add(gid)
            row.append(int(a))
            if len(row) == width:
                break
        while len(row) < width:
            row.append(row[-1])
        keep[p] = row
    return keep


def _first_strict_maximum(ret, start_value=None):
    """Scan the columns left to right as the device does.  `start_value` None: the first column is taken whatever it holds and a
    later one replaces it only when strictly greater (back-up step); otherwise a column is taken only when strictly greater than
    the running maximum, which starts at `start_value` (root step: -inf, slot -1 when nothing is above it)."""
    P, W = ret.shape
    if start_value is None:
        best, slot, first = ret[:, 0].copy(), np.zeros(P, np.int32), 1
    else:
        best, slot, first = np.full(P, start_value, F32), np.full(P, -1, np.int32), 0
    with np.errstate(invalid="ignore"):
        for k in range(first, W):
            m = ret[:, k] > best
            best = np.where(m, ret[:, k], best).astype(F32)
            slot = np.where(m, k, slot).astype(np.int32)
    return best, slot


def _take(arr, keep):
    return np.take_along_axis(arr, keep.astype(np.int64), axis=1)


def replay(levels, gamma_bar, D, W, clip, sparse=False, groups=None):
    """`levels`: per tree level a dict with float32 `reward`, `child_value` (P_l, A), `child_robot` (P_l, A, 9), `humans_next`
    (P_l, H, 5) and, at level 0, optionally `reward_clip`.  W: the width as configured (used when `clip`).
    Returns {"levels": [per level: value1, keep, backup, best_slot, and below the deepest level next_robot / next_humans],
             "root_values", "root_kept", "best_value", "best_slot", "best_action"}."""
    assert len(levels) == D
    g = F32(gamma_bar)
    A = np.asarray(levels[0]["reward"]).shape[1]
    Wk = W if clip else A
    out = []
    for l, lv in enumerate(levels):
        rew, cv = np.asarray(lv["reward"], F32), np.asarray(lv["child_value"], F32)
        sel = np.asarray(lv["reward_clip"], F32) if l == 0 and lv.get("reward_clip") is not None else rew
        v1 = one_step_values(sel, cv, gamma_bar)
        keep = select(v1, Wk, clip, sparse, groups)
        o = {"value1": v1, "keep": keep, "reward": rew, "child_value": cv}
        if l + 1 < D:
            cr = np.asarray(lv["child_robot"], F32)
            o["next_robot"] = np.take_along_axis(cr, keep.astype(np.int64)[:, :, None], axis=1).reshape(-1, 9)
            o["next_humans"] = np.asarray(lv["humans_next"], F32)
        out.append(o)
    out[D - 1]["backup"] = _take(out[D - 1]["child_value"], out[D - 1]["keep"])            # V_planning(child, 1) = V(child)
    with np.errstate(all="ignore"):
        for l in range(D - 1, 0, -1):
            d = D - l + 1
            c = F32((d - 1) / d)
            L, U = out[l], out[l - 1]
            v = _take(U["child_value"], U["keep"]).reshape(-1, 1)                      # row p = q * W + slot
            inner = (g * L["backup"]).astype(F32) + _take(L["reward"], L["keep"])
            ret = ((v / F32(d)).astype(F32) + (c * inner).astype(F32)).astype(F32)
            best, slot = _first_strict_maximum(ret)
            U["backup"] = best.reshape(-1, Wk)
            L["best_slot"] = slot
        L0 = out[0]
        root_values = (_take(L0["reward"], L0["keep"]) + (g * L0["backup"]).astype(F32)).astype(F32)
    best_value, best_slot = _first_strict_maximum(root_values, -np.inf)
    L0["best_slot"] = best_slot
    best_action = np.where(best_slot >= 0, _take(L0["keep"], np.maximum(best_slot, 0)[:, None])[:, 0], -1).astype(np.int32)
    return {"levels": out, "root_values": root_values, "root_kept": L0["keep"], "best_value": best_value,
            "best_slot": best_slot, "best_action": best_action}


def best_branch(rep, b, W_kept):
    """[(level, parent index, slot, action)] along the best branch of root b, following the replay's best_slots."""
    path, p = [], b
    for l, lv in enumerate(rep["levels"]):
        slot = int(lv["best_slot"][p])
        path.append((l, p, slot, int(lv["keep"][p, slot])))
        p = p * W_kept + slot
    return path


def bits(x):
    """float32 array -> its bit patterns, every NaN as ONE pattern: numbers (signed zeros, denormals, infinities) compare by bits, a
    NaN equals any NaN -- the sign and payload of a NaN that an addition generates or passes on are the platform's, not the
    bookkeeping's."""
    a = np.ascontiguousarray(np.asarray(x, F32))
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


# ---------------------------------------------------------------------------------------------------------------------------
# synthetic rows for the selection tests (shared by the CPU test of the replay and the GPU test of tail_select)
# ---------------------------------------------------------------------------------------------------------------------------
LEADER_INDICES = (0, 63, 64, 127, 128, 191, 192)        # each lane slot (a = lane + 64 k) and, with A - 1, the last valid lane

FAMILIES = ("distinct", "three_levels", "all_equal", "leader", "two_leaders", "inf_mixed", "all_neg_inf", "zeros", "denormals",
            "some_nans", "only_nans", "nan_from_inf")


def synthetic_rows(A, seed=0):
    """{family: (reward (n,A), child_value (n,A))} float32.  Rows are built so that reward + g * child_value has the property the
    family names for ANY g in (0, 1]: where the property is about the sum, child_value is 0 (the sum is then the reward exactly;
    `zeros`: a zero of the reward's sign); the `distinct`, `denormals` and `nan_from_inf` families use both operands.  The number of rows of each family is stated here and asserted
    non-zero by the tests:
      distinct 4, three_levels 4, all_equal 2, leader one per index of LEADER_INDICES + (A-1) that exists, two_leaders one per
      lane l in (0, 1, 63) with l + 64 < A, plus (l + 64, l + 128) and (l + 128, l + 192) pairs where they exist (A <= 64: one row
      with leaders 0 and A-1 instead, when A >= 2), inf_mixed 3, all_neg_inf 1, zeros 3, denormals 2, some_nans 3 (A >= 2),
      only_nans 2, nan_from_inf 2."""
    rng = np.random.RandomState(1000 * A + seed)
    z = lambda n=1: np.zeros((n, A), F32)
    fam = {}
    fam["distinct"] = (rng.permutation(4 * A).reshape(4, A).astype(F32) / F32(8) - F32(3), (rng.uniform(-1, 1, (4, A)) / 32).astype(F32))      # |g cv| < half the spacing: distinct sums
    fam["three_levels"] = (rng.choice(np.array([-0.25, 0.5, 1.75], F32), (4, A)), z(4))
    fam["all_equal"] = (np.stack([np.full(A, 0.3, F32), np.full(A, -7.0, F32)]), z(2))
    idx = sorted({i for i in LEADER_INDICES + (A - 1,) if i < A})
    r = rng.uniform(-1, 1, (len(idx), A)).astype(F32)
    for n, i in enumerate(idx):
        r[n, i] = F32(2.0)
    fam["leader"] = (r, z(len(idx)))
    pairs = [(l + 64 * k, l + 64 * (k + 1)) for l in (0, 1, 63) for k in range(3) if l + 64 * (k + 1) < A]
    if not pairs and A >= 2:
        pairs = [(0, A - 1)]
    if pairs:
        r = rng.uniform(-1, 1, (len(pairs), A)).astype(F32)
        for n, (i, j) in enumerate(pairs):
            r[n, i] = r[n, j] = F32(2.0)
        fam["two_leaders"] = (r, z(len(pairs)))
    r = rng.uniform(-1, 1, (3, A)).astype(F32)
    r[0, rng.rand(A) < 0.3] = np.inf
    r[1, rng.rand(A) < 0.3] = -np.inf
    m = rng.rand(A)
    r[2, m < 0.25] = np.inf
    r[2, m > 0.7] = -np.inf
    r[0, 0], r[1, A - 1], r[2, A // 2], r[2, 0] = np.inf, -np.inf, np.inf, -np.inf     # (A = 1: row 2 is -inf)
    fam["inf_mixed"] = (r, z(3))
    fam["all_neg_inf"] = (np.full((1, A), -np.inf, F32), z(1))
    r = np.where(rng.rand(3, A) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    r[2, rng.rand(A) < 0.3] = F32(-1.0)
    r[0, 0], r[0, A - 1] = F32(-0.0), F32(0.0)
    r[1, 0], r[1, A - 1] = F32(0.0), F32(-0.0)
    fam["zeros"] = (r, np.where(r == 0, r, F32(0.0)).astype(F32))   # -0.0 + g * -0.0 = -0.0: the sum keeps the zero's sign
    tiny = np.float32(1.401298464324817e-45)                       # the smallest denormal
    r = (rng.randint(-4, 5, (2, A)).astype(F32) * tiny).astype(F32)
    c = z(2)
    c[1] = (rng.randint(-4, 5, A).astype(F32) * tiny).astype(F32)     # g * denormal: rounded to a denormal
    fam["denormals"] = (r, c)
    if A >= 2:
        r = rng.choice(np.array([-0.25, 0.5, 1.75], F32), (3, A))
        for n, frac in enumerate((0.1, 0.5, 0.9)):
            m = rng.rand(A) < frac
            m[rng.randint(A)] = True
            m[(np.nonzero(m)[0][0] + 1) % A] = False                # at least one NaN and one number
            r[n, m] = np.nan
        fam["some_nans"] = (r, z(3))
    r = np.full((2, A), np.nan, F32)
    r[1].view(np.uint32)[::2] = 0xFFC00001                           # other payloads and signs: still "a NaN"
    fam["only_nans"] = (r, z(2))
    r, c = rng.uniform(-1, 1, (2, A)).astype(F32), rng.uniform(-1, 1, (2, A)).astype(F32)
    m = rng.rand(2, A) < 0.3
    m[0, A - 1] = m[1, 0] = True
    r[m], c[m] = np.inf, -np.inf                                     # +inf + g * -inf = NaN for any g > 0
    fam["nan_from_inf"] = (r, c)
    return fam


def synthetic_batch(A, seed=0):
    """All families stacked: (reward (n,A), child_value (n,A), {family: row count})."""
    fam = synthetic_rows(A, seed)
    counts = {k: v[0].shape[0] for k, v in fam.items()}
    return (np.concatenate([v[0] for v in fam.values()]).astype(F32), np.concatenate([v[1] for v in fam.values()]).astype(F32),
            counts)
