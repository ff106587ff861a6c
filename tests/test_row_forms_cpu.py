"""CPU half of the row-kernel form tests (-m "not gpu"): the case table of tests/row_forms.py reaches every launch form of the MLP
row kernels, as the library's own planner (rgl_plan_mlp_rows: host only) answers -- with RGL_HEAD_ROWS_DIRECT unset and =0, each
in a child process because the switch is read once."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from relationalgraphlearning_amd import _native as nat
from tests import row_forms as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_plans = {}


def plans_under(direct):
    """{run id: {job: plan}} of a process with RGL_HEAD_ROWS_DIRECT unset (`direct`) or =0."""
    if direct not in _plans:
        env = {k: v for k, v in os.environ.items() if k != "RGL_HEAD_ROWS_DIRECT"}
        if not direct:
            env["RGL_HEAD_ROWS_DIRECT"] = "0"
        res = subprocess.run([sys.executable, "-c", "from tests import row_forms as rf\nrf.dump_plans()\n"], cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        _plans[direct] = json.loads(res.stdout.strip().splitlines()[-1])
    return _plans[direct]


def forms_reached(runs):
    """{form: [(run id, job, setting)]} over both settings, for the jobs the table names."""
    reached = {}
    for direct in (True, False):
        got = plans_under(direct)
        for r in runs:
            for job in r.jobs:
                reached.setdefault(got[r.id][job]["form"], []).append((r.id, job, "direct" if direct else "staged"))
    return reached


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "staged"])
def test_every_run_takes_the_form_the_table_states(direct):
    got = plans_under(direct)
    assert sorted(got) == sorted(r.id for r in rf.RUNS) and len(got) == len(rf.RUNS)
    for r in rf.RUNS:
        assert set(r.jobs) <= set(got[r.id]), r.id
        for job, want in r.jobs.items():
            p = got[r.id][job]
            assert p["direct"] == int(direct), (r.id, job, p)
            assert p["form"] == want[0 if direct else 1], (r.id, job, p, want)
            assert p["n_tiles"] == -(-rf.job_mlps(r)[job][2] // 16) and p["n_waves"] == min(p["n_tiles"], 2048), (r.id, job, p)
            assert p["lds_bytes"] <= 160 * 1024 - 1024 or p["form"] == "waves0", (r.id, job, p)
        # a run is "not mine" exactly where the table says so: no job the table does not name is without waves
        assert any(p["form"] == "waves0" for p in got[r.id].values()) == any(e[0 if direct else 1] == "waves0" for e in r.jobs.values()), r.id
        if rf.small(r):
            assert all(rf.job_mlps(r)[job][2] % 16 for job in r.jobs), (r.id, "a small run's rows are no multiple of the tile")


def test_the_table_reaches_every_form():
    """Each launch form has a run: a form that loses its last run fails here."""
    reached = forms_reached(rf.RUNS)
    assert set(rf.FORMS) <= set(reached), sorted(set(rf.FORMS) - set(reached))
    assert "kind11" not in reached and set(reached) <= set(rf.FORMS), sorted(reached)
    # every form in which a wave walks tiles has a run with more tiles than waves: the second tile adds to the first one's slab
    for direct in (True, False):
        got = plans_under(direct)
        walked = {got[r.id][job]["form"] for r in rf.RUNS for job in r.jobs if got[r.id][job]["n_tiles"] > 2048 >= got[r.id][job]["n_waves"]}
        assert set(rf.TWO_TILES) <= walked, sorted(set(rf.TWO_TILES) - walked)
    # the mixed launch: under RGL_HEAD_ROWS_DIRECT=0 a shared-tile job and a multi-wave job, both of mlp_rows_kernel (kind 0)
    mixed = plans_under(False)["E3-17100"]
    assert (mixed["w_r"]["kind"], mixed["w_r"]["coop"]) == (0, 1) and (mixed["w_h"]["kind"], mixed["w_h"]["coop"]) == (0, 0)
    assert mixed["w_h"]["waves_per_wg"] == 4
    # head_rows_kernel on either side of the 64 KB above which a launch has to raise the kernel's dynamic-LDS limit
    direct = plans_under(True)
    assert direct["V3-21"]["value"]["lds_bytes"] == 65280 and direct["V4-17"]["value"]["lds_bytes"] == 120576


def test_the_direct_form_fits_at_the_limits_of_the_abi():
    """the direct form returns before any LDS-fit check.  It fits whatever the ABI admits -- a static_assert in
    plan_rows_job says so; here the widest, deepest MLP is planned in both settings (staged: nothing holds 6 x 256 x 256 weights)."""
    dims = [nat.MAX_WIDTH] * (nat.MAX_MLP_LAYERS + 1)
    p = rf.plan(dims, 16)
    if p["direct"]:
        assert p["form"] == "kind1_gt64k" and p["lds_bytes"] == 148224 <= 160 * 1024 - 1024
    else:
        assert p["form"] == "waves0"
    assert rf.plan(dims, 1025 * 16)["form"] == "waves0"


def test_short_workspace_run_leaves_the_first_max_waves():
    """The run that is there for `n_waves < n_tiles`: at max_waves = 2048 its slabs do not fit the caller's workspace, at some smaller
    power of two they do, and there w_h has fewer waves than tiles."""
    run = rf.RUN[rf.SHORT_WORKSPACE]
    used, have = rf.backward_workspace(run, 2048)
    assert used > have, (used, have)
    fits = [mw for mw in (1 << k for k in range(11, -1, -1)) if rf.backward_workspace(run, mw)[0] <= have]
    assert fits and fits[0] < 2048
    p = rf.plans(run, fits[0])["w_h"]
    assert p["n_waves"] == fits[0] < p["n_tiles"] == 16, (fits[0], p)


def test_plan_export_checks_its_arguments():
    lib = nat.lib()
    m, p = nat.RglMlp(), nat.RglRowsPlan()
    m.n_layers, m.dims[0], m.dims[1] = 1, 32, 1
    assert lib.rgl_plan_mlp_rows(None, 16, 2048, ctypes.byref(p)) == -3 and lib.rgl_plan_mlp_rows(ctypes.byref(m), 16, 2048, None) == -3
    assert lib.rgl_plan_mlp_rows(ctypes.byref(m), 0, 2048, ctypes.byref(p)) == -1
    assert lib.rgl_plan_mlp_rows(ctypes.byref(m), 16, 0, ctypes.byref(p)) == -1
    m.dims[1] = nat.MAX_WIDTH + 1
    assert lib.rgl_plan_mlp_rows(ctypes.byref(m), 16, 2048, ctypes.byref(p)) == -1
    m.dims[1], m.n_layers = 1, nat.MAX_MLP_LAYERS + 1
    assert lib.rgl_plan_mlp_rows(ctypes.byref(m), 16, 2048, ctypes.byref(p)) == -1
    m.n_layers = 1                                      # the weight pointers are not read: they are NULL here
    assert lib.rgl_plan_mlp_rows(ctypes.byref(m), 37, 2, ctypes.byref(p)) == 0
    assert (p.n_tiles, p.n_waves, p.n_wgs, p.waves_per_wg) == (3, 2, 2, 1) and p.kind in (0, 1) and p.lds_bytes > 0
    assert ctypes.sizeof(nat.RglRowsPlan) == 8 * 4 + 8
