"""The tile-packed head pass of the fused children kernel taken early (RGL_FUSED_HEAD_EARLY) against the pass behind a barrier.

A parent's partial last tile -- the lone `stop` child of the 5 x 16 + 1 table -- hands its rows to a pass that scores them tile-packed
over the workgroup's parents.  That pass used to start behind a workgroup barrier at the end of the kernel, one wave per packed tile
while the others waited; now the waves that run out of work items first take the packed tiles, as soon as a counter in LDS says the
rows are there, while the other waves still work (rgl_fused_kernel.hip).  Which wave scores a tile, and when, changes; the chain it
runs does not, so the check is `np.array_equal` on every value, not a tolerance: the same library with the switch off, in a process
of its own (the switch is read once per process), is the reference.

Shapes: tables with a lone partial child (A = 17, 81, 97), a wider partial tile (9, 25: rem = 9) and none (96); crowds on both sides
of every register bucket (N = 8 / 9, 16 / 17, 20 / 21), the softmax and a plain-weight similarity, skip on and off; 1, 2, 3, 10 and 17
parents per workgroup -- one packed tile, two (17 rows; 18 and 27 with rem = 9) and six (90 rows); workgroups with fewer items than
waves (idle waves take the tiles at once and wait for the rows) and with several passes of items; every dealing setting that leaves
the partial tile to the packed pass, and one that does not.  f32 and bf16x6.  Then one depth-2 search whose two levels take the
prologue form, where the tail of the kernel reads the values behind its own barrier.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import test_bf16x6_kernels as bk
from tests import test_level_prologue as lp
from tests.test_gpu_parity import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOP_TABLE = {17: (1, 16)}                      # one speed x 16 rotations + stop: one full tile and the `stop` child
SETTINGS = [(None, None), (1, 0), (2, 0), (99, 0), (1, 1)]      # (RGL_FUSED_G, RGL_FUSED_INLINE_PARTIAL); None: the cost model's cut


def cases(C):
    """(A, P, H, similarity, skip, flavour)"""
    eg = "embedded_gaussian"
    return [(17, 17 * C, 19, eg, True, "trained"), (17, 1, 1, eg, False, "trained"), (17, 9 * C + 5, 7, eg, True, "rand"),
            (81, C + 1, 15, eg, True, "trained"), (81, 2 * C + 3, 19, eg, True, "trained"), (81, 7, 20, eg, False, "trained"),
            (81, 9 * C + 5, 16, eg, True, "trained"), (97, 7, 8, eg, True, "trained"), (97, 2 * C + 3, 19, "squared", True, "trained"),
            (9, C + 1, 15, eg, False, "trained"), (9, 7, 7, eg, True, "trained"), (9, 9 * C + 5, 15, "squared", True, "trained"),
            (25, 2 * C + 3, 20, eg, True, "rand"), (25, 7, 1, eg, False, "trained"), (96, C + 1, 16, eg, True, "trained")]


def child_main(spec, out):
    """Entry point of the child processes (run_child): the children kernel's values in both modes, or one search."""
    with open(spec) as f:
        s = json.load(f)
    dev = torch.device("cuda:0")
    bk.TABLES.update(STOP_TABLE)
    res = {}
    for i, c in enumerate(s["cases"]):
        got = lp.search_outputs(c, dev) if s["kind"] == "search" else bk.children_outputs(c, dev)
        for k, v in got.items():
            res["%d/%s" % (i, k)] = v
    np.savez(out, **res)
    print("OK")


def run_child(kind, case_list, env_add, tmp_path, tag):
    spec, out = str(tmp_path / ("%s.json" % tag)), str(tmp_path / ("%s.npz" % tag))
    with open(spec, "w") as f:
        json.dump({"kind": kind, "cases": case_list}, f)
    code = "import sys\nfrom tests.test_stop_child import child_main\nchild_main(sys.argv[1], sys.argv[2])\n"
    res = subprocess.run([sys.executable, "-c", code, spec, out], cwd=ROOT, env=dict(os.environ, **env_add), capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and "OK" in res.stdout, (env_add, res.stdout[-2000:] + res.stderr[-3000:])
    return dict(np.load(out))


def identical(on, off, what):
    assert sorted(on) == sorted(off), what
    for k in sorted(on):
        assert on[k].dtype == off[k].dtype and on[k].shape == off[k].shape, (what, k)
        assert np.array_equal(on[k], off[k]) and on[k].tobytes() == off[k].tobytes(), (
            what, k, float(np.abs(on[k].astype(np.float64) - off[k]).max()))


def test_early_head_pass_is_the_pass_behind_the_barrier_bit_for_bit(tmp_path):
    """RGL_FUSED_HEAD_EARLY 1 against 0 under every dealing setting, every value of every shape in both modes."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    C = torch.cuda.get_device_properties(0).multi_processor_count
    cs = [dict(A=A, P=P, H=H, sim=sim, skip=skip, flavour=fl) for A, P, H, sim, skip, fl in cases(C)]
    packed_tiles, idle_waves, n = set(), False, 0
    for G, inline in SETTINGS:
        env_add = {"RGL_CHILDREN_FUSED": "1"}
        if G is not None:
            env_add.update(RGL_FUSED_G=str(G), RGL_FUSED_INLINE_PARTIAL=str(inline))
        plans = [bk.forced_plan(c["P"], c["A"], G, inline, C) if G is not None else None for c in cs]
        idx = [i for i, p in enumerate(plans) if p is None or bk.plan_allowed(p)]
        tag = "G%s_inline%s" % (G, inline)
        on = run_child("children", [cs[i] for i in idx], dict(env_add, RGL_FUSED_HEAD_EARLY="1"), tmp_path, tag + "_on")
        off = run_child("children", [cs[i] for i in idx], dict(env_add, RGL_FUSED_HEAD_EARLY="0"), tmp_path, tag + "_off")
        identical(on, off, tag)
        n += len(on)
        for j, i in enumerate(idx):
            c, p = cs[i], plans[i]
            assert on["%d/f32" % j].shape == (c["P"], c["A"])
            if p is not None and p["rem"] and not p["inline"]:
                packed_tiles.add((p["k"] * p["rem"] + 15) // 16)
                idle_waves |= p["k"] * p["ipp"] < 8
    assert {1, 2, 6} <= packed_tiles and idle_waves, (packed_tiles, idle_waves)
    report("early head pass: %d value arrays over %d shapes x %d dealing settings bit-identical to the pass behind the barrier "
           "(packed tiles per workgroup: %s)" % (n, len(cs), len(SETTINGS), sorted(packed_tiles)))


def test_early_head_pass_leaves_a_depth_two_search_unchanged(tmp_path):
    """One depth-2 search of four roots per CU -- both levels fold their prologue into the children launch (four and eight
    parents per workgroup: one packed tile each) --, the switch on against off: every output and per-level array byte for byte."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    C = torch.cuda.get_device_properties(0).multi_processor_count
    case = [(19, 4 * C, 2, 2, 11)]
    on = run_child("search", case, {"RGL_FUSED_HEAD_EARLY": "1"}, tmp_path, "search_on")
    off = run_child("search", case, {"RGL_FUSED_HEAD_EARLY": "0"}, tmp_path, "search_off")
    assert {"0/best_action", "0/best_value", "0/root_values"} <= set(on)
    identical(on, off, "depth-2 search of %d roots" % (4 * C))
    report("early head pass: %d arrays of a depth-2 search of %d roots byte-identical to the pass behind the barrier" % (len(on), 4 * C))
