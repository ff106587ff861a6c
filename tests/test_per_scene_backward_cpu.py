"""CPU half of the per-scene backward tests (-m "not gpu"): the conditions on the case table of tests/per_scene_backward.py, held against
the library's own planners (rgl_plan_scene_backward, rgl_plan_graph_tiles: host only) and against the float64 reference.  Each fails when
the run that meets it is taken out of the table, or when the table's run no longer reaches what it is there for."""
import ctypes

import numpy as np
import pytest

from relationalgraphlearning_amd import _native as nat
from tests import graph_forms as gf
from tests import per_scene_backward as psb
from tests import row_forms as rf
from tests.test_gpu_parity import REG_GRAD

THREADS = 1024                      # kThreads of csrc/rgl_backward.hip, as the export reports it
CC = [r for r in psb.RUNS if psb.short(r) == "cc"]
N = lambda r: r.H + 1


def reg_grad(run):
    return max(REG_GRAD, 8 * psb.reference(run)["yard_grad"])


def test_no_run_is_covered_by_the_tile_pipeline():
    """A run that becomes covered belongs in tests/graph_forms.py."""
    assert len(psb.RUN) == len(psb.RUNS) and 50 <= len(psb.RUNS) <= 70, len(psb.RUNS)
    assert psb.VALID in psb.RUN and psb.WALK in psb.RUN and psb.WALK_TAIL in psb.RUN
    for r in psb.RUNS + psb.REFUSALS:
        for backward in (False, True):
            p = gf.plan(r, backward)
            assert p["covered"] == 0 and p["inst"] is None, (r.id, backward, p)
    # every configuration graph_forms lists as refused has a run here
    have = {(psb.short(r), r.lw, r.X, r.L, N(r)) for r in psb.RUNS}
    assert any(s == "cc" for s, *_ in have)
    assert any(s == "co" and lw for s, lw, *_ in have) and any(s == "cs" and lw for s, lw, *_ in have)
    assert any(lw and X == 64 and s in ("eg", "ga", "sq") for s, lw, X, _, _ in have)
    assert any(lw and n > 32 and s in ("eg", "ga", "sq") for s, lw, _, _, n in have)
    assert any(L >= 4 for _, _, _, L, _ in have) and any(n >= 65 for *_, n in have)


def test_every_run_fits_and_the_limit_runs_are_the_last_that_fit():
    for r in psb.RUNS:
        p = psb.plan(r)
        assert p["fits"] == 1 and 0 < p["lds_bytes"] <= 160 * 1024 and p["threads"] == THREADS, (r.id, p)
        assert p["grid"] == min(r.S, 4096) and p["scenes_per_wg"] == -(-r.S // p["grid"]), (r.id, p)
        assert p["n_params"] == sum(rf.n_params(r)) + (psb.descriptors(r)[0].w_a_mlp.dims[1] * (2 * r.X + 2) + 1 if psb.short(r) == "cc" else 0), (r.id, p)
    assert len(psb.LIMITS) == len(psb.REFUSALS) == 3
    for fit, over in zip(psb.LIMITS, psb.REFUSALS):
        assert over.H == fit.H + 1 and over._replace(id=fit.id, H=fit.H, seed=fit.seed) == fit
        p, q = psb.plan(fit), psb.plan(over)
        assert p["fits"] == 1 and q["fits"] == 0 and p["lds_bytes"] <= 160 * 1024 < q["lds_bytes"], (fit.id, p, q)
        assert psb.limit_H(fit.id) == fit.H
    shipped = [r for r in psb.LIMITS if len(r.wr) == 2]
    narrow = [r for r in psb.LIMITS if len(r.wr) == 1]
    assert len(shipped) == 2 and len(narrow) == 1 and {psb.family(r) for r in shipped} == {"cc", "cslw"}
    assert all(33 <= N(r) <= 64 for r in shipped) and all(65 <= N(r) <= 80 for r in narrow), [(r.id, N(r)) for r in psb.LIMITS]


def test_loop_pass_boundaries():
    """Every `idx += kThreads` loop in one pass and in more than one, per family that has the loop."""
    def both(runs, count, what):
        counts = sorted({count(r) for r in runs})
        assert counts and counts[0] <= THREADS < counts[-1], (what, counts)
    cc, cclw = [r for r in CC if not r.lw], [r for r in CC if r.lw]
    cos = [r for r in psb.RUNS if psb.family(r) in ("colw", "cslw")]
    lw = [r for r in psb.RUNS if psb.family(r) == "lw"]
    for runs, name in ((cc, "cc"), (cclw, "cclw"), (cos, "cosine")):
        both(runs, lambda r: N(r) * N(r), name + ": N N")
        both(runs, lambda r: N(r) * r.X, name + ": N x_dim")
    for runs, name in ((cc, "cc"), (cclw, "cclw")):
        both(runs, lambda r: N(r) * 2 * r.X, name + ": N hid")
        assert any(N(r) * 2 * r.X == THREADS + 2 * r.X for r in CC), "the first N at which N hid passes 1024"
    both(lw, lambda r: N(r) * N(r), "layerwise softmax / squared: N N")
    both(lw, lambda r: N(r) * r.X, "layerwise softmax / squared: N x_dim")
    # the first N of the second pass itself: N N at 33, N x_dim at 33 (x_dim 32) and 17 (x_dim 64)
    assert any(N(r) == 33 and r.X == 32 for r in cc) and any(N(r) == 33 for r in lw) and any(N(r) == 34 for r in cos)
    assert any(N(r) == 17 and r.X == 64 for r in cos)
    assert any(r.X == 64 for r in cc) and any(r.X == 64 for r in cos) and any(r.X == 64 for r in lw)
    assert {N(r) for r in cc} >= {2, 6, 20, 33} and {N(r) for r in cos} >= {2, 6, 20, 34} and {N(r) for r in lw} >= {6, 33, 40}


def test_routes_layers_skip_depth_nodes_and_batches():
    fams = {}
    for r in psb.RUNS:
        fams.setdefault(psb.family(r), []).append(r)
    assert set(fams) == {"cc", "cclw", "colw", "cslw", "lw", "plain"}
    for fam, runs in fams.items():
        assert {r.module for r in runs} == {"value", "motion", "rgl"}, (fam, sorted({r.module for r in runs}))
        assert {r.skip for r in runs} == {True, False}, fam
    for fam in ("cc", "colw", "cslw"):
        assert {1, 2, 3} <= {r.L for r in fams[fam]}, fam
    assert {2, 3, 4} <= {r.L for r in fams["cclw"]}
    assert {psb.short(r) for r in fams["lw"]} == {"eg", "ga", "sq"}
    # depth: 4 and RGL_MAX_GCN_LAYERS, plain and layerwise, a softmax, a cosine and a concatenation graph each; no layer at all
    kind = lambda r: "cc" if psb.short(r) == "cc" else ("cosine" if psb.short(r) in ("co", "cs") else "softmax")
    for L in (4, nat.MAX_GCN_LAYERS):
        for lw in (False, True):
            assert {kind(r) for r in psb.RUNS if r.L == L and r.lw == lw} == {"softmax", "cosine", "cc"}, (L, lw)
    assert nat.MAX_GCN_LAYERS == 8
    assert {r.module for r in psb.RUNS if r.L == 0} == {"value", "motion", "rgl"}
    # many nodes
    wide = [r for r in psb.RUNS if N(r) >= 65 and r not in psb.LIMITS]
    assert {N(r) for r in wide} == {65, 80} and all(r.L == 1 and len(r.wr) == len(r.wh) == len(r.head or [1]) == 1 for r in wide)
    # batch: one scene, the reference's 100, a second block of reduce_slabs_kernel with a tail and with a 16-unrolled step and a tail
    S = {r.S for r in psb.RUNS}
    assert {1, 100, 257, 273, 4101} <= S, sorted(S)
    assert (257 - 256) < 16 <= (273 - 256) and (273 - 256) % 16
    walk, tail = psb.RUN[psb.WALK], psb.RUN[psb.WALK_TAIL]
    p = psb.plan(walk)
    assert p["grid"] == 4096 and p["scenes_per_wg"] == 2 and walk.S - p["grid"] == 5 == tail.S and N(walk) == 3, p
    assert walk.dark == p["grid"] == tail.first and walk.first == 0 == tail.dark
    assert tail._replace(id=walk.id, S=walk.S, first=0, dark=walk.dark) == walk
    assert psb.family(walk) == "cclw" and walk.L >= 2, "a walked scene accumulates the pair MLP's gradients over its layers"
    # the pair: the same scenes and the same upstream gradient where it is not dark
    (r1, h1), (r2, h2) = rf.scenes(walk), rf.scenes(tail)
    assert np.array_equal(r1[walk.dark:].numpy(), r2.numpy()) and np.array_equal(h1[walk.dark:].numpy(), h2.numpy())
    u1, u2 = rf.upstream(walk), rf.upstream(tail)
    assert np.array_equal(u1[walk.dark:].numpy(), u2.numpy()) and not u1[:walk.dark].any() and u2.abs().min() > 0


def test_seeds_and_references():
    """Every reference is finite (a zero cosine norm would give NaN) and its seed keeps every ReLU away from zero."""
    for r in psb.RUNS:
        for detach in ((False, True) if r.module == "motion" else (False,)):
            ref = psb.reference(r, detach)
            assert ref["masks_agree"] and ref["n_masks"] > 0 and ref["margin"] >= 8, (r.id, ref["margin"])
            assert np.isfinite(ref["out"]).all() and all(np.isfinite(g).all() for g in ref["grads"].values()), r.id
            assert np.isfinite(ref["yard_fwd"]) and np.isfinite(ref["yard_grad"]), r.id
        names = sorted(psb.reference(r)["grads"])
        block = psb.block_parameters(r)
        assert (set(block) <= set(names)) == (r.L > 0 or not block), (r.id, names)        # no layer: torch gives the block no gradient
        assert sum(k.startswith("graph.Ws.") for k in names) == r.L, (r.id, names)


def test_concatenation_adjacencies_are_alive_with_closed_entries_and_empty_rows():
    fractions = {}
    for r in CC:
        A = psb.adjacency(r.id)
        assert len(A) == (max(r.L, 1) if r.lw else 1) and all(a.shape == (r.S, N(r), N(r)) for a in A), r.id
        fractions[r.id] = [float((a > 0).mean()) for a in A]
        assert min(fractions[r.id]) >= 0.1, (r.id, fractions[r.id], "the pair MLP's output is closed nearly everywhere: a dead graph")
    # an all-open run never uses the A > 0 mask
    partly = [k for k, f in fractions.items() if 0.2 <= f[0] <= 0.9]
    assert len(partly) >= 3 and any(N(psb.RUN[k]) >= 20 for k in partly), fractions
    # a node whose whole row is closed: T_i = 0 and pre-activations that are exactly 0 (row_forms.reference: zeros_decided)
    empty = [r.id for r in CC if any((a == 0).all(axis=2).any() for a in psb.adjacency(r.id))]
    assert empty, "no concatenation run has an all-zero adjacency row"
    assert any(psb.RUN[k].L >= 1 for k in empty)


def test_every_layer_adds_to_the_block_gradients_of_a_layerwise_run():
    """Without any one layer's pass through the block, each of the block's parameter gradients moves by 10 regression bounds: a kernel
    that writes where it should add (or adds where it should write) is far outside the bound of the run that meets it."""
    runs = [r for r in psb.RUNS if r.lw and r.L >= 1 and psb.block_parameters(r)]
    assert {psb.short(r) for r in runs} == {"eg", "cc"} and len(runs) >= 8
    assert any(psb.short(r) == "cc" and r.L >= 2 for r in runs) and any(r.L == 8 for r in runs)
    for r in runs:
        ref = psb.reference(r)
        for layer in range(r.L):
            moved = psb.without_layer(r, layer)
            for k in psb.block_parameters(r):
                move = rf.grad_error(moved[k], ref["grads"][k])
                assert move >= 10 * reg_grad(r), (r.id, layer, k, move, reg_grad(r))


def test_the_column_term_of_the_cosine_norm_matters():
    runs = [r for r in psb.RUNS if r.lw and psb.short(r) in ("co", "cs") and r.L >= 1]
    assert len(runs) >= 8
    for r in runs:
        ref, moved = psb.reference(r), psb.without_column_term(r)
        move = max(rf.grad_error(moved[k], ref["grads"][k]) for k in ref["grads"])
        assert move >= 10 * reg_grad(r), (r.id, move, reg_grad(r))


def test_the_relu_mask_beyond_one_pass_matters():
    """A 33-node concatenation run has closed entries beyond the first 1024 of its adjacency whose gradient would be far off if the mask
    stopped there, on each route that reaches them (value through two layers, rgl)."""
    runs = [r for r in CC if N(r) * N(r) > THREADS]
    assert {r.module for r in runs if not r.lw} >= {"value", "rgl"} and any(r.lw for r in runs)
    seen = 0
    for r in runs:
        closed = [int((a.reshape(r.S, -1)[:, THREADS:] <= 0).sum()) for a in psb.adjacency(r.id)]
        if psb.RUN[r.id] in psb.LIMITS:
            continue
        assert closed[0] > 0, (r.id, closed)
        ref, moved = psb.reference(r), psb.without_mask_beyond(r, THREADS)
        move = max(rf.grad_error(moved[k], ref["grads"][k]) for k in ref["grads"])
        assert move >= 10 * reg_grad(r), (r.id, move, reg_grad(r))
        seen += 1
    assert seen >= 3


def test_plan_export_checks_its_arguments():
    lib, ref = nat.lib(), ctypes.byref
    run = psb.RUN[psb.VALID]
    g, vh, _ = psb.descriptors(run)
    p = nat.RglSceneBackwardPlan()
    assert ctypes.sizeof(nat.RglSceneBackwardPlan) == 6 * 4 + 8
    assert lib.rgl_plan_scene_backward(None, ref(vh), None, 3, 5, ref(p)) == -3 and lib.rgl_plan_scene_backward(ref(g), ref(vh), None, 3, 5, None) == -3
    for S, H in ((0, 5), (3, 0), (3, nat.MAX_NODES)):
        assert lib.rgl_plan_scene_backward(ref(g), ref(vh), None, S, H, ref(p)) == -1, (S, H)
    assert lib.rgl_plan_scene_backward(ref(g), ref(vh), None, 3, 5, ref(p)) == 0
    assert (p.fits, p.threads, p.grid, p.scenes_per_wg) == (1, THREADS, 3, 1) and p.lds_bytes > 0
    assert p.n_params == lib.rgl_graph_param_count(ref(g), ref(vh), None)
    assert lib.rgl_plan_scene_backward(ref(g), ref(vh), None, 10000, 5, ref(p)) == 0 and (p.grid, p.scenes_per_wg) == (4096, 3)
    assert lib.rgl_plan_scene_backward(ref(g), ref(vh), None, 8192, 5, ref(p)) == 0 and (p.grid, p.scenes_per_wg) == (4096, 2)
    # a scene that does not fit is an answer, not an error
    assert lib.rgl_plan_scene_backward(ref(g), ref(vh), None, 3, nat.MAX_NODES - 1, ref(p)) == 0 and p.fits == 0 and p.lds_bytes > 160 * 1024
    # the descriptors are validated as the launch validates them
    g.similarity = 99
    assert lib.rgl_plan_scene_backward(ref(g), ref(vh), None, 3, 5, ref(p)) == -2
    g.similarity, g.num_layer = nat.SIMILARITY["concatenation"], nat.MAX_GCN_LAYERS + 1
    assert lib.rgl_plan_scene_backward(ref(g), ref(vh), None, 3, 5, ref(p)) == -1
    g.num_layer = 1
    g.w_a_mlp.weight[0] = None
    assert lib.rgl_plan_scene_backward(ref(g), ref(vh), None, 3, 5, ref(p)) == -3
