"""SARL / OM-SARL for 21..127 humans without a GPU: the limit in the header and in the package, the workspace sizes the host side of
the library reports, and the float32 restatement's distance from float64 on the scenes the GPU tests run -- the measurement the GPU
bound is built from (tests/sarl_dense.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from relationalgraphlearning_amd import _native as nat
from tests import sarl_cpu as cpu
from tests import sarl_dense as dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARK_BYTES = 29 * 64 * 4          # a human's parking slot: 28 registers of a wave and its attention score


def planner(input_dim=61, with_global_state=True, widths_ok=True):
    """A SarlPlanner of the shipped widths for the host-side size functions: they read shapes and that the pointers are set,
    nothing behind them."""
    keep = ctypes.create_string_buffer(16)
    addr = ctypes.addressof(keep)

    def mlp(dims, last_relu):
        m = nat.RglMlp()
        m.n_layers, m.last_relu = len(dims) - 1, int(last_relu)
        for l, d in enumerate(dims):
            m.dims[l] = d
        for l in range(len(dims) - 1):
            m.weight[l], m.bias[l] = addr, addr
        return m

    pl = nat.SarlPlanner()
    pl.mlp1 = mlp([input_dim, 150, 100 if widths_ok else 96], True)
    pl.mlp2 = mlp([100, 100, 50], False)
    pl.attention = mlp([200 if with_global_state else 100, 100, 100, 1], False)
    pl.mlp3 = mlp([56, 150, 100, 100, 1], False)
    pl.with_global_state = int(with_global_state)
    om = cpu.om_of(input_dim)
    pl.om_channel_size, pl.cell_num, pl.cell_size = (om[2], om[0], om[1]) if om else (0, 4, 1.0)
    pl.contraction_dtype = nat.CONTRACTION_DTYPES["f32"]
    pl.num_actions = 81
    pl._keep = keep
    return pl


def test_header_and_package_agree_on_127():
    hdr = open(os.path.join(ROOT, "include", "rgl_hip.h")).read()
    assert int(re.search(r"#define RGL_SARL_MAX_HUMANS (\d+)", hdr).group(1)) == nat.SARL_MAX_HUMANS == 127
    assert int(re.search(r"#define RGL_MAX_NODES (\d+)", hdr).group(1)) == nat.SARL_MAX_HUMANS + 1
    assert nat.ABI_VERSION == 8


def test_the_new_entry_point_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "rgl_hip.h")).read()
    name = "sarl_value_workspace_bytes_for"
    assert name in nat.SIGNATURES and name in re.findall(r"^\s*(?:int|size_t)\s+(\w+)\s*\(", hdr, flags=re.M)
    assert hasattr(ctypes.CDLL(nat.LIB_PATH), name)


@pytest.mark.parametrize("input_dim,with_global_state", [(13, True), (61, True), (61, False)])
def test_value_workspace_sizes(monkeypatch, input_dim, with_global_state):
    monkeypatch.delenv("RGL_SARL_PARK", raising=False)
    monkeypatch.delenv("RGL_SARL_GRID_CAP", raising=False)
    lib = nat.lib()
    pl = planner(input_dim, with_global_state)
    ref = ctypes.byref(pl)
    packed = lib.sarl_value_workspace_bytes(ref)
    assert packed > 0
    S = 162                                                    # 11 tiles: the launch starts 11 workgroups
    for H in ([1] if input_dim == 13 else []) + [2, 20]:
        assert lib.sarl_value_workspace_bytes_for(ref, S, H) == packed
    sizes = [lib.sarl_value_workspace_bytes_for(ref, S, H) for H in (21, 50, 127)]
    assert packed < sizes[0] <= sizes[1] <= sizes[2]
    for H, size in zip((21, 50, 127), sizes):
        assert packed + 11 * H * PARK_BYTES <= size < packed + 11 * H * PARK_BYTES + 256
    # a persistent, capped grid: the region stops growing with the scenes, and follows the test switch for the grid
    big = lib.sarl_value_workspace_bytes_for(ref, 2048 * 81, 50)
    assert big == lib.sarl_value_workspace_bytes_for(ref, 4096 * 81, 50) and big <= packed + 512 * 50 * PARK_BYTES + 256
    monkeypatch.setenv("RGL_SARL_GRID_CAP", "2")
    assert lib.sarl_value_workspace_bytes_for(ref, S, 50) - packed in range(2 * 50 * PARK_BYTES, 2 * 50 * PARK_BYTES + 256)
    monkeypatch.delenv("RGL_SARL_GRID_CAP")
    # outside the supported shapes
    assert lib.sarl_value_workspace_bytes_for(ref, S, 128) == 0 and lib.sarl_value_workspace_bytes_for(ref, S, 0) == 0
    assert lib.sarl_value_workspace_bytes_for(ref, 0, 21) == 0 and lib.sarl_value_workspace_bytes_for(None, S, 21) == 0
    if input_dim != 13:
        assert lib.sarl_value_workspace_bytes_for(ref, S, 1) == 0          # maps of a single human
    odd = planner(input_dim, with_global_state, widths_ok=False)
    assert lib.sarl_value_workspace_bytes_for(ctypes.byref(odd), S, 21) == 0 == lib.sarl_value_workspace_bytes(ctypes.byref(odd))
    # the switch: the global form, and its size, at small H too; any other value is the automatic choice
    monkeypatch.setenv("RGL_SARL_PARK", "global")
    assert lib.sarl_value_workspace_bytes_for(ref, S, 5) - packed in range(11 * 5 * PARK_BYTES, 11 * 5 * PARK_BYTES + 256)
    assert lib.sarl_value_workspace_bytes(ref) == packed
    assert lib.sarl_value_workspace_bytes_for(ref, S, 21) == sizes[0]
    monkeypatch.setenv("RGL_SARL_PARK", "lds")
    assert lib.sarl_value_workspace_bytes_for(ref, S, 5) == packed and lib.sarl_value_workspace_bytes_for(ref, S, 21) == sizes[0]


def test_predict_workspace_covers_dense_crowds(monkeypatch):
    monkeypatch.delenv("RGL_SARL_PARK", raising=False)
    monkeypatch.delenv("RGL_SARL_GRID_CAP", raising=False)
    lib = nat.lib()
    pl = planner()
    ref = ctypes.byref(pl)
    at = {H: lib.sarl_predict_workspace_bytes(ref, 2, H) for H in (20, 21, 127)}
    assert at[20] > 0 and at[21] > 0 and at[127] > 0
    assert lib.sarl_predict_workspace_bytes(ref, 2, 128) == 0
    # the step from 20 to 21 humans holds the parking region of the 11 workgroups two roots start; it grows with H from there
    assert at[21] - at[20] >= 11 * 21 * PARK_BYTES and at[127] - at[21] >= 11 * 106 * PARK_BYTES


@pytest.mark.parametrize("weights", ["plain", "sharp"])
@pytest.mark.parametrize("H", dense.DENSE_H)
def test_float32_restatement_on_the_gpu_scenes(H, weights):
    """Upstream's float32 arithmetic against float64 on the scenes the GPU test runs (input_dim 13 and 61, both global-state
    settings): its distance on the action values stays below the small crowds' value bound -- it does not grow with H -- and at most
    one root in ten has its two best actions closer than twice the bound a case is held to (the GPU test leaves those decisions
    out); where they are further apart, float32 decides as float64 does."""
    close = total = 0
    for input_dim in (13, 61):
        for with_global_state in (True, False):
            roots = dense.case(H, input_dim, with_global_state, weights)
            value_bound, attention_bound = dense.bounds(weights, roots)
            dv, da = max(r["dev_value"] for r in roots), max(r["dev_attention"] for r in roots)
            print("H %d D %d global %d %s: float32 - float64 action values %.2e (bound %.2e), attention %.2e (bound %.2e)"
                  % (H, input_dim, with_global_state, weights, dv, value_bound, da, attention_bound))
            assert np.isfinite(dv) and np.isfinite(da) and dv < cpu.value_bound(weights)
            for r in roots:
                total += 1
                if cpu.gap(r["action_values"]) > 2 * value_bound:
                    assert r["best32"] == r["best"]
                else:
                    close += 1
    assert 10 * close <= total
