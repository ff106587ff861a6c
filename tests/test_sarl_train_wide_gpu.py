"""SARL / OM-SARL gradients on the device at the batch and crowd sizes training launches: the wide cases of tests/sarl_train.py
(batches assembled scene by scene) through sarl_value_backward_f32 against float64 autograd -- more than 64 humans, crowds past the
forward's LDS form, more tiles than one grid pass, contractions over 500 to 13120 rows -- gradients other than the MSE's, the row
limit, and the trainer with a short last batch."""
import ctypes as C

import pytest
import torch

from tests import sarl_train as st
from tests.test_sarl_train_gpu import abi_train, check_gradients, dev, make_model, module_gradients, reference, run_trainer  # noqa: F401

pytestmark = pytest.mark.gpu

_tail_references = {}


def tail_reference(case):
    """float64 gradients of sum(tail_grad_value * value): computed once and shared."""
    if case not in _tail_references:
        _tail_references[case] = st.wide_gradients(case, "tail")
    return _tail_references[case]


@pytest.mark.parametrize("case", st.wide_cases(), ids=st.case_tag)
def test_gradients_against_float64(dev, case):
    """Through the C ABI (gradient buffers pre-filled with NaN: the call overwrites) and, up to the trainer's published batches,
    through loss.backward() on the module, bit for bit the same."""
    S, H, D, gs, w = case
    rows, targets, _ = reference(case)
    model = make_model(dev, D, gs, w)
    _, _, grads, _ = abi_train(model, rows.to(dev), targets.to(dev))
    check_gradients(case, grads, "C ABI")
    if S * H <= st.MODULE_ROWS:
        by_module = module_gradients(model, rows.to(dev), targets.to(dev))
        assert all(torch.equal(grads[k], by_module[k]) for k in st.PARAMS)


def test_every_case_up_to_the_published_batches_runs_through_the_module():
    assert [c[:2] for c in st.wide_cases() if c[0] * c[1] > st.MODULE_ROWS] == [(2624, 5)] * 2


@pytest.mark.parametrize("case", [(3, 127, 61, True, "sharp"), (2, 65, 61, True, "sharp"), (17, 22, 61, True, "plain")], ids=st.case_tag)
def test_gradients_with_poisoned_workspaces(dev, monkeypatch, case):
    """RGL_DEBUG_POISON_WORKSPACES=1: no workspace byte is read before this call has written it."""
    monkeypatch.setenv("RGL_DEBUG_POISON_WORKSPACES", "1")
    S, H, D, gs, w = case
    rows, targets, _ = reference(case)
    model = make_model(dev, D, gs, w)
    check_gradients(case, abi_train(model, rows.to(dev), targets.to(dev))[2], "C ABI, poisoned")
    check_gradients(case, module_gradients(model, rows.to(dev), targets.to(dev)), "autograd, poisoned")


@pytest.mark.parametrize("case", [(2624, 5, 61, True, "sharp"), (3, 127, 61, True, "plain")], ids=st.case_tag)
def test_backward_is_deterministic(dev, case):
    """Waves of one launch take different trip counts through the tiles at 13120 rows; the bits do not depend on it."""
    S, H, D, gs, w = case
    rows, targets, _ = reference(case)
    model = make_model(dev, D, gs, w)
    _, _, first, ws = abi_train(model, rows.to(dev), targets.to(dev))
    _, _, reused, _ = abi_train(model, rows.to(dev), targets.to(dev), ws=ws)
    assert all(torch.equal(first[k], reused[k]) for k in st.PARAMS)


@pytest.mark.parametrize("case", [shape + (w,) for shape in st.TAIL_SHAPES for w in ("plain", "sharp")], ids=st.case_tag)
def test_tail_weighted_gradients_against_float64(dev, case):
    """grad_value is zero but for the last two scenes: what the last rows of the last tile contribute is the whole gradient."""
    S, H, D, gs, w = case
    rows = reference(case)[0]
    model = make_model(dev, D, gs, w)
    _, _, grads, _ = abi_train(model, rows.to(dev), None, grad_value=st.tail_grad_value(S).to(dev))
    check_gradients(case, grads, "C ABI, tail-weighted", tail_reference(case))


def test_a_sum_loss_through_autograd_and_accumulation(dev):
    """loss = model(rows).sum() hands the backward an expanded gradient of stride 0; the gradients are the C ABI's for ones, bit for
    bit, and a second backward() without zero_grad() leaves exactly twice the first."""
    case = (17, 22, 61, True, "sharp")
    S, H, D, gs, w = case
    rows = reference(case)[0].to(dev)
    model = make_model(dev, D, gs, w)
    _, _, want, _ = abi_train(model, rows, None, grad_value=torch.ones(S, 1, device=dev))
    assert all(torch.isfinite(want[k]).all() and want[k].abs().max() > 0 for k in st.PARAMS if k != "attention.4.bias")
    model.enable_training()
    model.zero_grad()
    with torch.enable_grad():
        model(rows).sum().backward()
    first = {k: p.grad.detach().clone() for k, p in zip(st.PARAMS, model.training_parameters())}
    assert all(torch.equal(first[k], want[k]) for k in st.PARAMS)
    with torch.enable_grad():
        model(rows).sum().backward()
    for k, p in zip(st.PARAMS, model.training_parameters()):
        assert torch.equal(p.grad, 2 * first[k]), k


def test_the_row_limit_is_refused(dev):
    """n_scenes * H may be 2^20 and no more; the refusal comes before anything of that size exists."""
    from relationalgraphlearning_amd import _native as nat
    lib = nat.lib()
    model = make_model(dev, 61, True, "plain")
    with torch.no_grad():
        pl = model.fill_planner(nat.SarlPlanner())
    assert 8256 * 127 < 1 << 20 < 8257 * 127 and 61681 * 17 == (1 << 20) + 1
    assert lib.sarl_train_workspace_bytes(C.byref(pl), 8257, 127) == 0
    assert lib.sarl_train_workspace_bytes(C.byref(pl), 61681, 17) == 0
    assert lib.sarl_train_workspace_bytes(C.byref(pl), 8256, 127) > 0 and lib.sarl_train_workspace_bytes(C.byref(pl), 16384, 64) > 0
    need = lib.sarl_train_workspace_bytes(C.byref(pl), 4, 5)
    rows, ws = torch.zeros(4, 5, 61, device=dev), torch.empty(need, dtype=torch.uint8, device=dev)
    value, gv = torch.empty(4, 1, device=dev), torch.zeros(4, 1, device=dev)
    out = [torch.full_like(p, 7.0) for p in model.training_parameters()]
    grads = nat.SarlGrads()
    for l in range(nat.SARL_LAYERS):
        grads.weight[l], grads.bias[l] = out[2 * l].data_ptr(), out[2 * l + 1].data_ptr()
    for S, H in ((8257, 127), (61681, 17)):
        assert lib.sarl_value_backward_f32(C.byref(pl), rows.data_ptr(), gv.data_ptr(), S, H, ws.data_ptr(), need, C.byref(grads), None) == -1
        assert lib.sarl_value_train_f32(C.byref(pl), rows.data_ptr(), S, H, ws.data_ptr(), need, value.data_ptr(), None, None) == -1
    torch.cuda.synchronize()
    assert all(bool((g == 7.0).all()) for g in out)            # a refused call writes nothing


# ---- the trainer with a short last batch -------------------------------------------------------------------------------------------
def test_trainer_with_a_short_last_batch(dev):
    """Case C: 50 transitions in batches of 16, so optimize_epoch(1) and optimize_batch(3, 0) each meet a batch of 2 -- a second shape
    for either kind of captured step -- against upstream's VNRLTrainer fixture, and captured against eager bit for bit."""
    fx, spec, data = st.wide_fixture(), st.WIDE_TRAINER_CASE, st.wide_trainer_data()
    t, model, losses, captures = run_trainer(dev, "C", spec=spec, data=data)
    want = fx["tr.C.losses"]
    distance = st.parameter_distance(model.state_dict(), "C", fx)
    print("trainer case C: losses %s, upstream %s; parameters %.2e from upstream" % (losses, want.tolist(), distance))
    sizes = [min(st.TRAINER_BATCH, st.WIDE_TRAINER_N - lo) for lo in range(0, st.WIDE_TRAINER_N, st.TRAINER_BATCH)]
    assert sizes == [16, 16, 16, 2]
    il = {("il", n) for n in sizes}                              # optimize_epoch(1) meets every batch
    rl = {("rl", n) for n in sizes[:spec["batches"] + 1]}        # optimize_batch(3, 0) consumes four
    assert t._capturable and captures == [len(il), len(il | rl)] == [2, 4]
    assert len(losses) == len(want)
    for got, w in zip(losses, want):
        assert abs(got - w) <= st.LOSS_BOUND * max(1.0, abs(w)), (got, w)
    assert distance <= st.PARAMETER_BOUND
    _, eager, _, eager_captures = run_trainer(dev, "C", eager=True, spec=spec, data=data)
    assert eager_captures == [0, 0]
    for (k, a), b in zip(model.state_dict().items(), eager.state_dict().values()):
        assert torch.equal(a, b), k
