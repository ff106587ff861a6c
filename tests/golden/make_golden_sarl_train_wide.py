"""Fixture generator for the wide SARL / OM-SARL training cases (build container only: imports the upstream reference through
make_golden_sarl_train.py, whose upstream_network, upstream_gradients and upstream_trainer_run it uses as they are).

Writes tests/golden/sarl_train_wide.npz: per shape of tests/sarl_train.WIDE_SHAPES the candidate indices whose scenes make up the
batch (tests/sarl_train.assemble: each scene keeps the ReLU margin on its own, for both weight sets); per entry of
tests/sarl_train.wide_entries() the assembled batch's margin, what UPSTREAM's sarl.ValueNetwork gives on the CPU in float32 -- max
|g| of every parameter tensor and its distance from the float64 restatement -- and the float64 max |g|; and upstream's VNRLTrainer on
the 50 transitions of trainer case C.  Arrays and short tag strings only.  sarl_train.npz is not touched.

    python tests/golden/make_golden_sarl_train_wide.py
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_sarl_train import upstream_network, upstream_gradients, upstream_trainer_run  # noqa: E402

from tests import sarl_cpu as cpu  # noqa: E402
from tests import sarl_train as st  # noqa: E402


def upstream_weighted_gradients(rows, grad_value, sd, input_dim, with_global_state):
    net = upstream_network(input_dim, with_global_state, sd)
    (grad_value * net(rows)).sum().backward()
    named = dict(net.named_parameters())
    return {k: named[k].grad.detach().clone() for k in st.PARAMS}


def main():
    out, tags, margins = {}, [], []
    for shape in st.WIDE_SHAPES:
        t0 = time.time()
        kept, rows = st.assemble(shape)
        tried = int(kept[-1]) + 1
        rejected = 1.0 - len(kept) / float(tried)
        if rejected > st.MAX_REJECTED:
            raise RuntimeError("%s rejects %.3f of its candidates" % (st.shape_tag(shape), rejected))
        out["kept.%s" % st.shape_tag(shape)] = kept
        st._wide_rows[tuple(shape)] = rows
        print("%-22s kept %d of %d candidates (%.1f %% rejected), %.1f s" % (st.shape_tag(shape), len(kept), tried, 100 * rejected,
                                                                              time.time() - t0))
    st._wide_fixture.update(out)                                # wide_rows() and wide_gradients() read the kept indices from it
    for case, kind in st.wide_entries():
        S, H, D, gs, w = case
        rows, sd = st.wide_rows(case), cpu.weight_set(w, D, gs)
        margin = st.relu_margin(rows, sd, gs)
        if not margin >= st.RELU_MARGIN:
            raise RuntimeError("%s: the assembled batch's margin is %g" % (st.entry_tag(case, kind), margin))
        ref = st.wide_gradients(case, kind)
        if kind == "tail":
            up = upstream_weighted_gradients(rows, st.tail_grad_value(S), sd, D, gs)
        else:
            up = upstream_gradients(rows, st.wide_targets(case), sd, D, gs)
        tag = st.entry_tag(case, kind)
        out["grad.%s.max" % tag] = st.max_abs(up)
        out["grad.%s.dist" % tag] = st.distances(up, ref)
        out["grad.%s.max64" % tag] = st.max_abs(ref)
        tags.append(tag)
        margins.append(margin)
        rel = np.where(out["grad.%s.max64" % tag] > 0, out["grad.%s.dist" % tag] / np.maximum(out["grad.%s.max64" % tag], 1e-300), 0)
        print("%-30s margin %.2e  upstream rel. distance %.1e .. %.1e (%s)" % (tag, margin, rel[rel > 0].min(), rel.max(),
                                                                             st.PARAMS[int(rel.argmax())]))
    out["cases"], out["margins"] = np.asarray(tags), np.asarray(margins, np.float64)

    # trainer case C: tests/sarl_train.wide_trainer_data()'s 50 seeded transitions (made from seeds, not stored)
    data = st.wide_trainer_data()
    sd, losses = upstream_trainer_run("C", data, st.WIDE_TRAINER_CASE)
    sd64, losses64 = st.trainer_loop("C", torch.float64, st.WIDE_TRAINER_CASE, data)
    gap = max(float((sd[k].double() - sd64[k]).abs().max()) for k in st.PARAMS)
    print("trainer case C: losses %s (float64 %s), float64 loop ends %.2e from upstream" % (losses, losses64, gap))
    if not gap <= st.PARAMETER_BOUND / 4:
        raise RuntimeError("trainer case C: float32 and float64 end %.2e apart, more than a quarter of the bound" % gap)
    for k in st.PARAMS:
        out["tr.C.model.%s" % k] = sd[k].numpy().astype(np.float32)
    out["tr.C.losses"] = np.asarray(losses, np.float64)
    path = os.path.join(HERE, "sarl_train_wide.npz")
    np.savez_compressed(path, **out)
    print("wrote sarl_train_wide.npz, %d bytes" % os.path.getsize(path))
    st._wide_fixture.clear()
    for w in ("plain", "sharp"):                 # what tests/sarl_train.WIDE_GRADIENT_DEVIATION pins
        print('    "%s": [%s],' % (w, ", ".join("None" if k == "attention.4.bias" else "%.3g" % x
                                                for k, x in zip(st.PARAMS, st.wide_relative_figures(w)))))


if __name__ == "__main__":
    main()
