"""The wide SARL / OM-SARL training cases without a device: batches assembled scene by scene (tests/sarl_train.py) against their
fixture, the table that bounds them, and the two mistakes these shapes exist to expose, planted in float64."""
import os

import numpy as np
import pytest
import torch

from tests import sarl_cpu as cpu
from tests import sarl_train as st

ENTRIES = st.wide_entries()
_cache = {}


def entry_id(entry):
    return st.entry_tag(*entry)


def reference(case, kind="mse"):
    """float64 gradients of an entry: computed once and shared."""
    if (case, kind) not in _cache:
        _cache[case, kind] = st.wide_gradients(case, kind)
    return _cache[case, kind]


def test_fixture_holds_every_case_and_stays_small():
    fx = st.wide_fixture()
    assert [str(t) for t in fx["cases"]] == [st.entry_tag(c, k) for c, k in ENTRIES]
    assert os.path.getsize(st.WIDE_GOLDEN) < 1 << 20
    assert all(v.dtype.kind in "fiU" for v in fx.values())                   # arrays and tag strings, nothing else
    flagship = [(2, 64), (2, 65), (3, 127), (17, 22), (100, 5), (100, 19), (2624, 5)]
    span = [(128, 2), (129, 2)]                                               # 256 and 258 rows: one span of the contraction, and two
    assert st.WIDE_SHAPES == [(2, 64, 61, True), (2, 65, 61, True), (2, 64, 13, False)] + [s + (61, True) for s in flagship[2:] + span]
    assert st.TAIL_SHAPES == [(3, 127, 61, True), (2624, 5, 61, True)] and set(st.TAIL_SHAPES) <= set(st.WIDE_SHAPES)
    assert not set(st.WIDE_SHAPES) & set(st.SHAPES)
    assert len(ENTRIES) == 2 * (len(st.WIDE_SHAPES) + len(st.TAIL_SHAPES))
    # the sizes the shapes are there for: the 64-thread stride's two sides, the human limit with a ragged row tile, more tiles of
    # a 150-column product than one grid pass of 2048 blocks of four waves takes -- with the last row tile a full one
    assert 3 * 127 == 23 * 16 + 13 and 127 == cpu_max_humans()
    rows = 2624 * 5
    assert rows % 16 == 0 and (rows // 16) * 10 > 4 * 2048 >= ((rows - 16) // 16) * 10
    assert fx["tr.C.losses"].shape == (2,) and all("tr.C.model.%s" % k in fx for k in st.PARAMS)


def cpu_max_humans():
    from relationalgraphlearning_amd import _native as nat
    return nat.SARL_MAX_HUMANS


@pytest.mark.parametrize("shape", st.WIDE_SHAPES, ids=st.shape_tag)
def test_kept_candidates(shape):
    """The stored indices are S increasing candidates of which at most 95 % were rejected; where the candidates are few enough to
    rebuild them all, every one passed over misses the margin for a weight set: the kept ones are the FIRST that hold."""
    S, H, D, gs = shape
    kept = st.wide_fixture()["kept.%s" % st.shape_tag(shape)]
    assert kept.shape == (S,) and kept[0] >= 0 and (np.diff(kept) > 0).all()
    tried = int(kept[-1]) + 1
    assert 1.0 - S / float(tried) <= st.MAX_REJECTED
    assert tuple(st.wide_rows(shape).shape) == (S, H, D)
    if tried <= 40:
        sds = [cpu.weight_set(w, D, gs) for w in ("plain", "sharp")]
        for k in sorted(set(range(tried)) - set(int(i) for i in kept)):
            scene = st.case_rows(1, H, D, st.wide_base(shape) + k)
            assert min(st.relu_margin(scene, sd, gs) for sd in sds) < st.RELU_MARGIN, k


@pytest.mark.parametrize("entry", ENTRIES, ids=entry_id)
def test_assembled_margin(entry):
    case, kind = entry
    S, H, D, gs, w = case
    margin = st.relu_margin(st.wide_rows(case), cpu.weight_set(w, D, gs), gs)
    assert margin >= st.RELU_MARGIN
    assert abs(margin - float(st.wide_fixture()["margins"][ENTRIES.index(entry)])) <= 1e-9


@pytest.mark.parametrize("entry", ENTRIES, ids=entry_id)
def test_restatement_reproduces_the_fixtures_figures(entry):
    """float64 autograd through sarl_cpu.value_network against what upstream's float32 network gave on the assembled batch."""
    case, kind = entry
    fx, tag = st.wide_fixture(), st.entry_tag(case, kind)
    ref_max = st.max_abs(reference(case, kind))
    assert np.allclose(ref_max, fx["grad.%s.max64" % tag], rtol=1e-9, atol=1e-30)
    for k, m64, m32, d in zip(st.PARAMS, ref_max, fx["grad.%s.max" % tag], fx["grad.%s.dist" % tag]):
        if k == "attention.4.bias":
            continue                                    # mathematically zero: upstream holds rounding noise
        assert m64 > 0 and abs(m64 - m32) <= d + 1e-30 and d <= 2e-5 * m64, (k, m64, m32, d)


def test_tail_weighted_gradient_is_the_last_two_scenes():
    gv = st.tail_grad_value(7)
    assert gv.shape == (7, 1) and gv.dtype == torch.float32
    assert gv[:5].abs().max() == 0 and float(gv[5]) == 1.0 and float(gv[6]) == -0.5


def test_pinned_table_equals_the_fixtures():
    """The wide table is, per tensor, the larger of the single-seed cases' pinned figure and the wide fixture's largest upstream
    figure; it never undercuts the table it extends, and that table is as it was."""
    skip = st.PARAMS.index("attention.4.bias")
    for w in ("plain", "sharp"):
        measured, pinned, old = st.wide_relative_figures(w), st.WIDE_GRADIENT_DEVIATION[w], st.REFERENCE_GRADIENT_DEVIATION[w]
        assert pinned[skip] is None and len(pinned) == len(st.PARAMS)
        for i, (m, p, o) in enumerate(zip(measured, pinned, old)):
            assert i == skip or (abs(m - p) <= 0.006 * p and p >= o), (w, st.PARAMS[i], m, p, o)
        assert 1e-7 < min(p for p in pinned if p) and max(p for p in pinned if p) < 8e-6
    assert st.gradient_bounds((2, 64, 61, True, "sharp"), np.ones(len(st.PARAMS)))[0] == st.MARGIN_FACTOR * 7.8e-07
    assert st.gradient_bounds((2, 21, 61, True, "sharp"), np.ones(len(st.PARAMS)))[0] == st.MARGIN_FACTOR * 5.81e-07


# ---- the bounds' teeth at these shapes ---------------------------------------------------------------------------------------------
def _violations(case, kind="mse", **switches):
    ref = reference(case, kind)
    wrong = st.wide_gradients(case, kind, **switches)
    dist, bound = st.distances(wrong, ref), st.gradient_bounds(case, st.max_abs(ref))
    return {k for k, d, b in zip(st.PARAMS, dist, bound) if d > b}


MLP1 = {"mlp1.0.weight", "mlp1.0.bias", "mlp1.2.weight", "mlp1.2.bias"}
ATTENTION = {"attention.%d.%s" % (i, p) for i in (0, 2, 4) for p in ("weight", "bias") if (i, p) != (4, "bias")}
MLP3 = {"mlp3.%d.%s" % (i, p) for i in (0, 2, 4, 6) for p in ("weight", "bias")}


@pytest.mark.parametrize("case", [c for c in st.wide_cases() if c[4] == "sharp"], ids=st.case_tag)
def test_the_switches_are_the_restatement_when_off(case):
    got, ref = st.wide_gradients(case, "mse", detach_weights_from=None, drop_last_scene=False), reference(case)
    assert all(torch.equal(got[k], ref[k]) for k in st.PARAMS)


@pytest.mark.parametrize("case", [(2, 65, 61, True, "sharp"), (3, 127, 61, True, "sharp")], ids=st.case_tag)
def test_a_softmax_backward_that_stops_at_64_humans_is_caught(case):
    bad = _violations(case, detach_weights_from=64)
    assert MLP1 | ATTENTION <= bad, sorted((MLP1 | ATTENTION) - bad)


@pytest.mark.parametrize("case", [(2, 64, 61, True, "sharp"), (2, 64, 13, False, "sharp")], ids=st.case_tag)
def test_the_same_switch_changes_nothing_at_64_humans(case):
    """No human is past the 64th: the switch is the fault, not noise."""
    assert _violations(case, detach_weights_from=64) == set()
    wrong, ref = st.wide_gradients(case, "mse", detach_weights_from=64), reference(case)
    assert all(torch.equal(wrong[k], ref[k]) for k in st.PARAMS)


def test_a_dropped_last_scene_is_caught_under_the_mse():
    bad = _violations((2624, 5, 61, True, "sharp"), drop_last_scene=True)
    assert MLP3 <= bad, sorted(MLP3 - bad)


@pytest.mark.parametrize("case", [(2624, 5, 61, True, "sharp"), (3, 127, 61, True, "sharp")], ids=st.case_tag)
def test_a_dropped_last_scene_is_caught_in_every_tensor_under_the_tail_weights(case):
    bad = _violations(case, "tail", drop_last_scene=True)
    want = set(st.PARAMS) - {"attention.4.bias"}               # mathematically zero with or without the scene
    assert want <= bad, sorted(want - bad)


def test_float64_trainer_loop_lands_on_upstreams_parameters_with_a_short_last_batch():
    fx = st.wide_fixture()
    data = st.wide_trainer_data()
    assert data[0].shape == (50, st.TRAINER_H, st.TRAINER_D) and 50 % st.TRAINER_BATCH == 2
    assert not torch.equal(data[0][:48], st.trainer_data()[0])
    sd, losses = st.trainer_loop("C", torch.float64, st.WIDE_TRAINER_CASE, data)
    want = fx["tr.C.losses"]
    assert st.parameter_distance(sd, "C", fx) <= st.PARAMETER_BOUND / 4
    assert len(losses) == len(want) and all(abs(a - b) <= st.LOSS_BOUND * max(1.0, abs(b)) for a, b in zip(losses, want))
