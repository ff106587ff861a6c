"""CPU-side tests (-m "not gpu"): the C ABI library loads and exports every declared symbol, host
logic (action tables, sharding, configs, checkpoints) is right, and the product refuses to run
without the device path."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import relationalgraphlearning_amd as rga
from relationalgraphlearning_amd import _native as nat
from tests import golden_io as gio
from tests.helpers import make_mprl_policy, make_gcn_policy, JS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol():
    hdr = open(os.path.join(ROOT, "include", "rgl_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(nat.SIGNATURES), declared ^ set(nat.SIGNATURES)
    assert os.path.exists(nat.LIB_PATH), "run __graft_entry__.build() first"
    handle = ctypes.CDLL(nat.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    lib = nat.lib()
    assert lib.rgl_abi_version() == nat.ABI_VERSION
    assert lib.rgl_build_target() == b"gfx950"


def test_struct_layout_matches_header_sizes():
    # sizes implied by include/rgl_hip.h on LP64 (ints 4 B, pointers 8 B, natural alignment)
    mlp = 4 + 4 + 4 * 7 + 4 + 8 * 6 + 8 * 6          # 4 B padding after dims[7] for pointer alignment
    assert ctypes.sizeof(nat.RglMlp) == mlp
    graph = 2 * mlp + 6 * 4 + 8 + mlp + 8 * 8
    assert ctypes.sizeof(nat.RglGraph) == graph
    assert ctypes.sizeof(nat.MprlLevelView) == 12 * 8               # ABI 6: + reward_clip_off
    assert ctypes.sizeof(nat.MprlPlanner) == 2 * graph + 2 * mlp + 8 * 4 + 2 * 8 + 2 * 8 + 2 * 8 + 8 + 8 + 8  # ABI 8: + action_speed_bound; ABI 2: + float64 root pointers; ABI 3: + children_image; ABI 4: + predictor_image
    assert ctypes.sizeof(nat.GcnPlanner) == graph + mlp + 2 * 4 + 2 * 8 + 8 + 2 * 8 + 2 * 4        # ABI 8: + contraction_dtype, reserved
    assert ctypes.sizeof(nat.RglTransposeJob) == 2 * 8 + 2 * 4 and ctypes.sizeof(nat.RglGatherJob) == 2 * 8 + 2 * 4      # ABI 7
    assert ctypes.sizeof(nat.RglValueChildrenPlan) == 6 * 4
    assert ctypes.sizeof(nat.RglTwoStageChildrenPlan) == 14 * 4 + 2 * 8
    assert ctypes.sizeof(nat.RglSceneBackwardPlan) == 6 * 4 + 8


def test_contraction_modes_and_level_view_match_the_header():
    """ABI 6 (7 adds entry points only): the contraction-mode constants of include/rgl_hip.h are the ones the Python side sends; the level view exposes the
    root's tensor-born reward array (reward_clip_off) at level 0 of a clipped search only."""
    hdr = open(os.path.join(ROOT, "include", "rgl_hip.h")).read()
    consts = {name: int(val) for name, val in re.findall(r"#define (RGL_CONTRACT_\w+)\s+(\d+)", hdr)}
    assert consts == {"RGL_CONTRACT_F32": 0, "RGL_CONTRACT_F16": 1, "RGL_CONTRACT_BF16X6": 3}      # 2 (F16X3) left with ABI 8
    assert nat.CONTRACTION_DTYPES == {"f32": 0, "f16": 1, "bf16x6": 3}
    assert int(re.search(r"#define RGL_ABI_VERSION (\d+)", hdr).group(1)) == nat.ABI_VERSION == 8
    lib = nat.lib()
    pl = nat.MprlPlanner()
    pl.planning_depth, pl.planning_width, pl.num_actions, pl.do_action_clip = 2, 2, 81, 1
    view = nat.MprlLevelView()
    assert lib.mprl_tree_level_view(ctypes.byref(pl), 64, 19, 0, ctypes.byref(view)) == 0 and view.reward_clip_off > 0
    assert view.reward_clip_off % 256 == 0 and view.reward_clip_off != view.reward_off
    assert lib.mprl_tree_level_view(ctypes.byref(pl), 64, 19, 1, ctypes.byref(view)) == 0 and view.reward_clip_off == -1
    pl.do_action_clip = 0
    assert lib.mprl_tree_level_view(ctypes.byref(pl), 64, 19, 0, ctypes.byref(view)) == 0 and view.reward_clip_off == -1


def test_host_side_argument_checks_without_gpu():
    lib = nat.lib()
    # NULL pointers and bad shapes are rejected on the host before any launch
    assert lib.rgl_transpose_f32(None, None, 4, 4, None) == -3
    assert lib.rgl_transpose_many_f32(None, 2, None) == -3 and lib.rgl_transpose_many_f32(None, 0, None) == 0
    assert ctypes.sizeof(nat.RglTransposeJob) == 24
    assert lib.gcn_rotate_f32(None, None, 4, 0, None) == -3
    assert lib.mprl_tree_workspace_bytes(None, 4, 5) == 0
    assert lib.gcn_predict_workspace_bytes(4, 5, 81) > 0
    pl = nat.MprlPlanner()
    pl.planning_depth, pl.planning_width, pl.num_actions, pl.do_action_clip = 2, 2, 81, 1
    n2 = lib.mprl_tree_workspace_bytes(ctypes.byref(pl), 2048, 19)
    pl.planning_depth = 3
    n3 = lib.mprl_tree_workspace_bytes(ctypes.byref(pl), 2048, 19)
    assert 0 < n2 < n3 < (1 << 31)
    view = nat.MprlLevelView()
    assert lib.mprl_tree_level_view(ctypes.byref(pl), 2048, 19, 2, ctypes.byref(view)) == 0
    assert view.n_parents == 2048 * 4
    assert lib.mprl_tree_level_view(ctypes.byref(pl), 2048, 19, 3, ctypes.byref(view)) == -1
    # ABI 3: the caller-owned weight image -- no image for an architecture without the image-based kernel (empty descriptors)
    assert lib.mprl_children_image_bytes(None) == 0
    assert lib.mprl_children_image_bytes(ctypes.byref(pl)) == 0
    assert lib.mprl_pack_children_image_f32(None, None, 0, None) == -3
    assert lib.mprl_pack_children_image_f32(ctypes.byref(pl), ctypes.c_void_p(16), 0, None) != 0


def test_path_g_steps_refuse_bad_shapes_without_gpu():
    """gcn_prepare_f32 / gcn_predict_f32 check their arguments on the host before any launch: B < 1, H = 0, H = 128 (129 nodes),
    A = 0, A = 257, an unknown kinematics, a NULL action table and NULL arrays are refused; no pointer is read."""
    lib = nat.lib()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below returns before its launch
    BAD_SHAPE, BAD_MODE, NULL = -1, -2, -3

    def planner(A=81, kinematics=0, table=p):
        pl = nat.GcnPlanner()
        pl.num_actions, pl.kinematics, pl.time_step, pl.gamma = A, kinematics, 0.25, 0.9
        pl.actions = table
        return ctypes.byref(pl)

    def prepare(pl, B=4, H=5, robot=p):
        return lib.gcn_prepare_f32(pl, robot, p, B, H, p, p, p, None)

    def predict(pl, B=4, H=5, ws=p):
        return lib.gcn_predict_f32(pl, p, p, B, H, ws, 1 << 30, p, p, p, None)

    for call in (prepare, predict):
        assert call(planner(), B=0) == BAD_SHAPE and call(planner(), B=-3) == BAD_SHAPE
        assert call(planner(), H=0) == BAD_SHAPE and call(planner(), H=128) == BAD_SHAPE
        assert call(planner(A=0)) == BAD_SHAPE and call(planner(A=257)) == BAD_SHAPE
        assert call(planner(kinematics=2)) == BAD_MODE and call(planner(kinematics=-1)) == BAD_MODE
        assert call(planner(table=None)) in (BAD_SHAPE, NULL)
        assert call(None) == NULL
    assert prepare(planner(), robot=None) == NULL and predict(planner(), ws=None) == NULL


def test_product_refuses_cpu_tensors():
    pol = make_mprl_policy("trained", 1)
    pol.set_device(torch.device("cpu"))
    pl = gio.load("planning")
    js = JS(pl["plan.scene.s5.robot"][0], pl["plan.scene.s5.humans"][0])
    with pytest.raises(nat.NativeLibraryError):
        pol.predict(js)
    with torch.no_grad(), pytest.raises(nat.NativeLibraryError):
        pol.value_estimator((torch.zeros(1, 1, 9), torch.zeros(1, 2, 5)))
    g = make_gcn_policy()
    g.set_device(torch.device("cpu"))
    with pytest.raises(nat.NativeLibraryError):
        g.predict(js)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "relationalgraphlearning_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f
                assert "/root/reference" not in text, f


def test_action_tables_and_groups():
    ar = gio.load("actions_rewards")
    pol = make_mprl_policy("trained")
    pol.build_action_space(1.0)
    assert len(pol.action_space) == 81 and pol.action_space[0] == rga.ActionXY(0, 0)
    from relationalgraphlearning_amd.actions import as_array
    assert np.array_equal(as_array(pol.action_space), ar["act.mprl"])
    assert pol.action_group_index == ar["act.mprl_groups"].tolist()
    g = make_gcn_policy()
    g.build_action_space(1.0)
    assert np.array_equal(as_array(g.action_space), ar["act.gcn"])


def test_parameter_names_and_shapes_match_reference_checkpoints():
    pol = make_mprl_policy("rand", L=3)
    sd = pol.get_state_dict()
    m = gio.master("rand")
    for k, v in sd["graph_model1"].items():
        assert tuple(v.shape) == m["graph_model1." + k].shape, k
    assert [tuple(v.shape) for v in sd["value_network"].values()] == \
        [(32, 32), (32,), (100, 32), (100,), (100, 100), (100,), (1, 100), (1,)]
    assert [tuple(v.shape) for v in sd["motion_predictor"].values()] == [(64, 32), (64,), (5, 64), (5,)]
    shared = make_mprl_policy("rand", variant="shared")
    assert set(shared.get_state_dict()) == {"graph_model", "value_network", "motion_predictor"}
    assert shared.state_predictor.graph_model is shared.value_estimator.graph_model
    lin = make_mprl_policy("rand", variant="linear")
    assert set(lin.get_state_dict()) == {"graph_model", "value_network"} and not lin.state_predictor.trainable
    g = make_gcn_policy()
    assert set(g.get_state_dict()) == set(gio.path_g_sd())
    assert pol.get_model() is pol.value_estimator
    assert abs(pol.get_normalized_gamma() - 0.9 ** 0.25) < 1e-15


def test_logical_eval_counts():
    assert make_mprl_policy("rand", 1).tree_search().logical_value_evals_per_root() == 81
    assert make_mprl_policy("rand", 2, 2, True).tree_search().logical_value_evals_per_root() == 249
    assert make_mprl_policy("rand", 3, 2, True).tree_search().logical_value_evals_per_root() == 581
    assert make_mprl_policy("rand", 2, 1, False).tree_search().logical_value_evals_per_root() == 81 * 82


def test_registration_uses_reference_keys():
    factory = {}
    rga.register(factory)
    assert factory["model_predictive_rl"] is rga.ModelPredictiveRL and factory["gcn"] is rga.GCN
    p = factory["model_predictive_rl"]()
    for attr in ("trainable", "phase", "model", "device", "last_state", "time_step", "env", "name",
                 "multiagent_training", "kinematics", "planning_depth", "traj", "state_predictor"):
        assert hasattr(p, attr), attr
    for meth in ("configure", "set_phase", "set_device", "set_env", "set_time_step", "set_epsilon", "get_model",
                 "save_model", "load_model", "get_state_dict", "load_state_dict", "predict", "transform",
                 "get_normalized_gamma", "get_traj"):
        assert callable(getattr(p, meth)), meth
    q = factory["gcn"]()
    assert hasattr(q, "action_values") and callable(q.get_matrix_A)


def test_shard_bounds_cover_everything_once():
    for n in (0, 1, 7, 8, 2048, 4097):
        for world in (1, 2, 3, 8):
            spans = [rga.shard_bounds(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def test_modules_deepcopy_and_pickle_with_populated_descriptor_cache():
    """Trainer.update_target_model deep-copies the model after forwards have run (crowd_nav/utils/trainer.py:41,187;
    train.py:161,206): the descriptor caches hold ctypes structs with raw pointers, which must not travel with a copy."""
    import copy
    import io
    pol = make_mprl_policy("trained", D=1)
    ve, sp = pol.value_estimator, pol.state_predictor
    for cache in (ve._cache, ve.graph_model._cache, sp._cache, sp.graph_model._cache):
        cache.key, cache.value, cache.keep = ("stale",), nat.RglGraph(), [torch.zeros(3)]   # what a forward leaves behind
    ve2, sp2 = copy.deepcopy(ve), copy.deepcopy(sp)
    for cache in (ve2._cache, ve2.graph_model._cache, sp2._cache, sp2.graph_model._cache):
        assert cache.key is None and cache.value is None and cache.keep is None
    assert ve._cache.key == ("stale",)                                  # the original keeps its cache
    for (k, a), (_, b) in zip(ve.state_dict().items(), ve2.state_dict().items()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr(), k
    buf = io.BytesIO()
    torch.save(ve, buf)
    buf.seek(0)
    ve3 = torch.load(buf, weights_only=False)
    assert ve3._cache.key is None and set(ve3.state_dict()) == set(ve.state_dict())
    g = make_gcn_policy().model
    g._cache.key, g._cache.value = ("stale",), nat.RglGraph()
    g._head_cache.key, g._head_cache.value = ("stale",), nat.RglMlp()
    g2 = copy.deepcopy(g)
    assert g2._cache.key is None and g2._head_cache.key is None


def test_empty_crowd_takes_the_reference_greedy_action():
    """Fixture vnrl_trainer.npz (greedy.*): the reference MultiHumanRL.predict on JointStates without humans (multi_human_rl.py:27-31 ->
    CADRL.select_greedy_action).  No network is involved, so this runs without a GPU."""
    from tests import golden_io as gio
    from tests.helpers import make_gcn_policy, JS
    fx = gio.load("vnrl_trainer")
    pol = make_gcn_policy()
    pol.device = "cpu"                                   # only marks the policy as configured: nothing is evaluated on it
    for row, want in zip(fx["greedy.robot"], fx["greedy.action"]):
        a = pol.predict(JS(row, []))
        assert a == pol.action_space[int(want)]


def test_flat_params_follow_the_module_like_parameters_does():
    """nets._flat_params (the descriptor caches' view of a module's parameters: a cached sub-module list, parameters read from the
    sub-modules' dicts on every call) against nn.Module.parameters(): same objects in the same order for every module of both
    policies, after a deep copy (the copy must list ITS parameters), after a parameter object was replaced, and after pickling."""
    import copy
    import io
    from relationalgraphlearning_amd import nets
    pol = make_mprl_policy("trained", 1)
    gcn = make_gcn_policy()
    for mod in (pol.value_estimator, pol.state_predictor, pol.value_estimator.graph_model, gcn.model):
        assert [id(p) for p in nets._flat_params(mod)] == [id(p) for p in mod.parameters()]
        assert [id(p) for p in nets._flat_params(mod)] == [id(p) for p in mod.parameters()]          # from the cached list
        twin = copy.deepcopy(mod)
        assert [id(p) for p in nets._flat_params(twin)] == [id(p) for p in twin.parameters()]
        assert not set(id(p) for p in nets._flat_params(twin)) & set(id(p) for p in mod.parameters())
        buf = io.BytesIO()
        torch.save(mod, buf)
        buf.seek(0)
        back = torch.load(buf, weights_only=False)
        assert [id(p) for p in nets._flat_params(back)] == [id(p) for p in back.parameters()]
    ve = pol.value_estimator
    ve.value_network[0].weight = torch.nn.Parameter(torch.zeros_like(ve.value_network[0].weight))      # a replaced Parameter object
    assert [id(p) for p in nets._flat_params(ve)] == [id(p) for p in ve.parameters()]
    # a replaced SUB-MODULE (the kept sub-module list used to hide it for ever) and an added one
    old = [id(p) for p in nets._flat_params(ve)]
    ve.value_network[2] = torch.nn.Linear(ve.value_network[2].in_features, ve.value_network[2].out_features)
    assert [id(p) for p in nets._flat_params(ve)] == [id(p) for p in ve.parameters()] != old
    ve.value_network.add_module("extra", torch.nn.Linear(1, 1))
    assert [id(p) for p in nets._flat_params(ve)] == [id(p) for p in ve.parameters()]
    nets.invalidate_packed_weights(ve)
    assert "_rgl_submodules" not in ve.__dict__


def test_a_failed_pack_leaves_no_transposes_queued():
    """pack_mlp queues one transpose job per Linear weight; a descriptor that fails part-way (here: the module's
    parameters are CPU tensors) must take its jobs back out instead of leaving them for the next unrelated flush."""
    from relationalgraphlearning_amd import nets
    pol = make_mprl_policy("trained", 1)
    assert not nets._PENDING_TRANSPOSES
    with pytest.raises(nat.NativeLibraryError):
        pol.value_estimator.graph_model.descriptor()
    assert not nets._PENDING_TRANSPOSES
    with pytest.raises(nat.NativeLibraryError):
        with nets.batched_transposes():
            pol.value_estimator.graph_model.descriptor()
    assert not nets._PENDING_TRANSPOSES and nets._BATCH_DEPTH[0] == 0


def test_tree_search_image_caches_are_keyed_on_the_contraction_mode():
    """the children / predictor weight images are laid out per contraction mode; the cache key must carry it."""
    import inspect
    from relationalgraphlearning_amd import rollout
    for fn in (rollout.TreeSearch._children_image, rollout.TreeSearch._predictor_image):
        src = inspect.getsource(fn)
        assert "self.contraction_dtype" in src.split("ent = ")[0], fn.__name__


def test_planner_speed_bound_and_path_g_contraction_modes():
    """ABI 8 host side: MprlPlanner.action_speed_bound is the top speed of the search's own action table (holonomic: |(vx, vy)|,
    unicycle: |v|) -- the reward step prunes far humans with it, so it must never be below a table entry; path G's search accepts the
    two contraction modes GcnPlanner knows and refuses anything else before any device work."""
    import numpy as np
    from relationalgraphlearning_amd import actions as act
    from relationalgraphlearning_amd.rollout import GcnSearch, TreeSearch
    table = act.speed_major_table(1.0, 5, 16, "holonomic", np.pi / 3)[0]
    arr = act.as_array(table)
    ts = TreeSearch(None, None, arr, None, "holonomic")
    assert ts._speed_bound() == float(np.hypot(arr[:, 0], arr[:, 1]).max()) and ts._speed_bound() >= 1.0 - 1e-12
    uni = act.speed_major_table(1.0, 5, 16, "unicycle", np.pi / 3)[0]
    ua = act.as_array(uni)
    assert TreeSearch(None, None, ua, None, "unicycle")._speed_bound() == float(np.abs(ua[:, 0]).max())
    for mode in ("f32", "bf16x6"):
        assert GcnSearch(None, arr, contraction_dtype=mode).contraction_dtype == mode
    with pytest.raises(ValueError):
        GcnSearch(None, arr, contraction_dtype="f16")


# ---------------------------------------------------------------------------------------------------------------------------
# workspace sizes: recorded from the build before the one-step searches shared their carve (csrc/rgl_onestep.h).  Every size
# function is its entry point's carve over a null base, so a buffer dropped, added or reordered by a rewrite shows here.
# ---------------------------------------------------------------------------------------------------------------------------
SIZE_CASES = [(1, 1), (1, 2), (17, 5), (2048, 19), (3, 21), (2, 127)]        # (B, H); A = 81
GCN_PREDICT_BYTES = {
    (1, 1): 112384,
    (1, 2): 125184,
    (17, 5): 1713152,
    (2048, 19): 560766976,
    (3, 21): 963072,
    (2, 127): 3343104,
}
SARL_BYTES = {      # (input_dim, with_global_state, RGL_SARL_PARK, B, H): (predict, value, value_for B * 81 scenes, train B scenes)
    (13, False, None, 1, 1): (459008, 452864, 452864, 465152),
    (13, False, None, 1, 2): (461568, 452864, 452864, 471808),
    (13, False, None, 17, 5): (718336, 452864, 452864, 987904),
    (13, False, None, 2048, 19): (106621440, 452864, 452864, 225634560),
    (13, False, None, 3, 21): (3119104, 452864, 2947328, 975360),
    (13, False, None, 2, 127): (11488768, 452864, 10824192, 2830848),
    (13, False, 'global', 1, 1): (503552, 452864, 497408, 472576),
    (13, False, 'global', 1, 2): (550656, 452864, 541952, 486656),
    (13, False, 'global', 17, 5): (3947776, 452864, 3682304, 1062144),
    (13, False, 'global', 2048, 19): (178842112, 452864, 72673536, 243689728),
    (13, False, 'global', 3, 21): (3119104, 452864, 2947328, 975360),
    (13, False, 'global', 2, 127): (11488768, 452864, 10824192, 2830848),
    (13, True, None, 1, 1): (509184, 503040, 503040, 516352),
    (13, True, None, 1, 2): (511744, 503040, 503040, 523520),
    (13, True, None, 17, 5): (768512, 503040, 503040, 1106176),
    (13, True, None, 2048, 19): (106671616, 503040, 503040, 256814336),
    (13, True, None, 3, 21): (3169280, 503040, 2997504, 1075712),
    (13, True, None, 2, 127): (11538944, 503040, 10874368, 3084288),
    (13, True, 'global', 1, 1): (553728, 503040, 547584, 523776),
    (13, True, 'global', 1, 2): (600832, 503040, 592128, 538368),
    (13, True, 'global', 17, 5): (3997952, 503040, 3732480, 1180416),
    (13, True, 'global', 2048, 19): (178892288, 503040, 72723712, 274869504),
    (13, True, 'global', 3, 21): (3169280, 503040, 2997504, 1075712),
    (13, True, 'global', 2, 127): (11538944, 503040, 10874368, 3084288),
    (61, False, None, 1, 2): (492544, 483584, 483584, 502528),
    (61, False, None, 17, 5): (765184, 483584, 483584, 1018624),
    (61, False, None, 2048, 19): (114123264, 483584, 483584, 225665280),
    (61, False, None, 3, 21): (3161856, 483584, 2978048, 1006080),
    (61, False, None, 2, 127): (11568128, 483584, 10854912, 2861568),
    (61, False, 'global', 1, 2): (581632, 483584, 572672, 517376),
    (61, False, 'global', 17, 5): (3994624, 483584, 3713024, 1092864),
    (61, False, 'global', 2048, 19): (186343936, 483584, 72704256, 243720448),
    (61, False, 'global', 3, 21): (3161856, 483584, 2978048, 1006080),
    (61, False, 'global', 2, 127): (11568128, 483584, 10854912, 2861568),
    (61, True, None, 1, 2): (542720, 533760, 533760, 554240),
    (61, True, None, 17, 5): (815360, 533760, 533760, 1136896),
    (61, True, None, 2048, 19): (114173440, 533760, 533760, 256845056),
    (61, True, None, 3, 21): (3212032, 533760, 3028224, 1106432),
    (61, True, None, 2, 127): (11618304, 533760, 10905088, 3115008),
    (61, True, 'global', 1, 2): (631808, 533760, 622848, 569088),
    (61, True, 'global', 17, 5): (4044800, 533760, 3763200, 1211136),
    (61, True, 'global', 2048, 19): (186394112, 533760, 72754432, 274900224),
    (61, True, 'global', 3, 21): (3212032, 533760, 3028224, 1106432),
    (61, True, 'global', 2, 127): (11618304, 533760, 10905088, 3115008),
}
REPLAY_BYTES = {
    (1, 1): 768,
    (6, 300): 9984,
    (17, 5): 1024,
    (40, 2048): 344320,
    (200, 257): 208384,
}
# (re-recorded when the children workspace became one carve, csrc/rgl_common.h carve_children: the weight image slot is reserved once,
# not twice, so the searches whose widest level has few parents need less; profiles/workspace_carve.txt has the old and new values)
TREE_BYTES = {      # (planning_depth, B, H): bytes; width 2, 81 actions, clipped, empty descriptors
    (1, 1, 1): 158208,
    (1, 1, 2): 158464,
    (1, 17, 5): 735232,
    (1, 2048, 19): 78247936,
    (1, 3, 21): 237312,
    (1, 2, 127): 109568,
    (2, 1, 1): 198912,
    (2, 1, 2): 199168,
    (2, 17, 5): 1414144,
    (2, 2048, 19): 164640768,
    (2, 3, 21): 366080,
    (2, 2, 127): 231936,
    (3, 1, 1): 279040,
    (3, 1, 2): 279552,
    (3, 17, 5): 2770176,
    (3, 2048, 19): 337426432,
    (3, 3, 21): 622592,
    (3, 2, 127): 475136,
}
# The children workspace and the module forwards' workspace with the shipped descriptors (dimensions and modes only: the size queries
# read no pointer), so that every user of the children workspace's region has a size: recorded from the build that made each of
# them one carve, every entry within the layout's bound of the build before it (at most 768 bytes of padding more; the children
# workspace of few parents less by about the weight image, which was reserved twice)
CHILDREN_BYTES = {(1, 1): 152064, (1, 2): 152320, (17, 5): 660480, (2048, 19): 68802560, (3, 21): 222208, (2, 127): 94720}   # (P, H)
FORWARD_VALUE_BYTES = {(1, 1): 31232, (1, 2): 31488, (17, 5): 539648, (2048, 19): 68681728, (3, 21): 101376,
                       (2, 127): 94720}                      # (B, H): B * 81 scenes, the 81 of a crowd sharing its rows
FORWARD_MOTION_BYTES = {(1, 1): 256, (1, 2): 512, (17, 5): 13056, (2048, 19): 5242880, (3, 21): 8448, (2, 127): 32768}   # B scenes
# mprl_tree_level_view of a depth-3, width-2 search of 3 roots with 21 humans: the offsets of the build before plan_levels walked a Carver
LEVEL_VIEWS = [
    dict(n_parents=3, robot_off=-1, humans_off=-1, humans_next_off=0, child_robot_off=1280, reward_off=10240, reward_clip_off=11264,
         child_value_off=12288, value1_off=13312, keep_off=14336, backup_off=14592, best_slot_off=14848),
    dict(n_parents=6, robot_off=15104, humans_off=0, humans_next_off=15360, child_robot_off=17920, reward_off=35584, reward_clip_off=-1,
         child_value_off=37632, value1_off=39680, keep_off=41728, backup_off=41984, best_slot_off=42240),
    dict(n_parents=12, robot_off=42496, humans_off=15360, humans_next_off=43008, child_robot_off=48128, reward_off=83200,
         reward_clip_off=-1, child_value_off=87296, value1_off=91392, keep_off=95488, backup_off=95744, best_slot_off=96000),
]


def _dims_mlp(dims, last_relu):
    m = nat.RglMlp()
    m.n_layers, m.last_relu = len(dims) - 1, int(last_relu)
    for i, d in enumerate(dims):
        m.dims[i] = d
    return m


def _shipped_graph():
    g = nat.RglGraph()
    g.w_r, g.w_h = _dims_mlp((9, 64, 32), True), _dims_mlp((5, 64, 32), True)
    g.x_dim, g.num_layer, g.similarity, g.skip_connection = 32, 2, nat.SIMILARITY["embedded_gaussian"], 1
    return g


def _shipped_planner():
    pl = nat.MprlPlanner()
    pl.value_graph, pl.value_head = _shipped_graph(), _dims_mlp((32, 32, 100, 100, 1), False)
    pl.predictor_graph, pl.motion_head = _shipped_graph(), _dims_mlp((32, 64, 5), False)
    pl.num_actions = 81
    return pl


def test_workspace_sizes_are_the_recorded_ones(monkeypatch):
    from tests.test_sarl_dense_cpu import planner as sarl_planner
    monkeypatch.delenv("RGL_SARL_GRID_CAP", raising=False)
    monkeypatch.delenv("RGL_SARL_PARK", raising=False)
    lib = nat.lib()
    assert {k: lib.gcn_predict_workspace_bytes(k[0], k[1], 81) for k in SIZE_CASES} == GCN_PREDICT_BYTES
    seen = set()
    for (D, gs, park, B, H), want in SARL_BYTES.items():
        if park:
            monkeypatch.setenv("RGL_SARL_PARK", park)
        else:
            monkeypatch.delenv("RGL_SARL_PARK", raising=False)
        pl = sarl_planner(D, gs)
        ref = ctypes.byref(pl)
        got = (lib.sarl_predict_workspace_bytes(ref, B, H), lib.sarl_value_workspace_bytes(ref),
               lib.sarl_value_workspace_bytes_for(ref, B * 81, H), lib.sarl_train_workspace_bytes(ref, B, H))
        assert got == want, (D, gs, park, B, H, got, want)
        seen.add((D, gs, park, (B, H)))
    monkeypatch.delenv("RGL_SARL_PARK", raising=False)
    assert seen == {(D, gs, park, c) for D in (13, 61) for gs in (False, True) for park in (None, "global") for c in SIZE_CASES
                    if D == 13 or c[1] >= 2}                                # maps of a single human: no such search
    assert {k: lib.rgl_replay_push_workspace_bytes(*k) for k in REPLAY_BYTES} == REPLAY_BYTES
    for (depth, B, H), want in TREE_BYTES.items():
        pl = nat.MprlPlanner()
        pl.planning_depth, pl.planning_width, pl.num_actions, pl.do_action_clip = depth, 2, 81, 1
        assert lib.mprl_tree_workspace_bytes(ctypes.byref(pl), B, H) == want, (depth, B, H)
    assert {(B, H) for _, B, H in TREE_BYTES} == set(SIZE_CASES)
    sp, g = ctypes.byref(_shipped_planner()), ctypes.byref(_shipped_graph())
    vh, mh = ctypes.byref(_dims_mlp((32, 32, 100, 100, 1), False)), ctypes.byref(_dims_mlp((32, 64, 5), False))
    assert {k: lib.mprl_value_children_workspace_bytes(sp, *k) for k in SIZE_CASES} == CHILDREN_BYTES
    assert {(B, H): lib.rgl_graph_forward_workspace_bytes(g, vh, None, B * 81, 81, H) for B, H in SIZE_CASES} == FORWARD_VALUE_BYTES
    assert {(B, H): lib.rgl_graph_forward_workspace_bytes(g, None, mh, B, 1, H) for B, H in SIZE_CASES} == FORWARD_MOTION_BYTES


def test_children_workspace_grows_with_the_parents():
    """A search gives ONE children workspace, sized for its widest level, to the calls of all its levels: a call of fewer parents must
    never ask for more.  Empty descriptors and the shipped ones, on both sides of the image slot's end (H + 1 = 32 | 33)."""
    lib = nat.lib()
    empty = nat.MprlPlanner()
    empty.num_actions = 81
    Ps = (1, 2, 3, 17, 199, 200, 256, 2048)
    for pl in (empty, _shipped_planner()):
        for H in (1, 5, 19, 24, 31, 32, 49):
            sizes = [lib.mprl_value_children_workspace_bytes(ctypes.byref(pl), P, H) for P in Ps]
            assert sizes[0] > 0 and sizes == sorted(sizes), (H, sizes)


def test_tree_level_view_offsets_are_the_recorded_ones():
    lib = nat.lib()
    pl = nat.MprlPlanner()
    pl.planning_depth, pl.planning_width, pl.num_actions, pl.do_action_clip = 3, 2, 81, 1
    for level, want in enumerate(LEVEL_VIEWS):
        v = nat.MprlLevelView()
        assert lib.mprl_tree_level_view(ctypes.byref(pl), 3, 21, level, ctypes.byref(v)) == 0
        assert {name: getattr(v, name) for name, _ in nat.MprlLevelView._fields_} == want, level


def test_predict_entry_points_refuse_one_byte_less():
    """gcn_predict_f32 and sarl_predict_f32 with a workspace of their size query less one byte: RGL_ERR_WORKSPACE, the last check
    before the first launch, so every other argument is in order (pointers set and never read).  With the full size the check is
    passed -- the call goes on to its launches, which this test only lets happen where there is no device to run them
    (tests/test_path_g_steps.py and tests/test_sarl_dense_gpu.py make the same two calls on real buffers)."""
    from tests.test_sarl_dense_cpu import planner as sarl_planner
    lib = nat.lib()
    p = ctypes.c_void_p(4096)
    keep = ctypes.create_string_buffer(16)
    addr = ctypes.addressof(keep)
    WORKSPACE = -4

    def mlp(dims):
        m = nat.RglMlp()
        m.n_layers = len(dims) - 1
        for l, d in enumerate(dims):
            m.dims[l] = d
        for l in range(len(dims) - 1):
            m.weight[l], m.bias[l] = addr, addr
        return m

    g = nat.GcnPlanner()
    g.num_actions, g.kinematics, g.time_step, g.gamma, g.actions = 81, 0, 0.25, 0.9, p
    g.graph.x_dim, g.graph.num_layer, g.graph.similarity = 32, 0, nat.SIMILARITY["gaussian"]
    g.graph.w_r, g.graph.w_h, g.value_head = mlp([6, 64, 32]), mlp([7, 64, 32]), mlp([32, 150, 100, 100, 1])
    s = sarl_planner(61, True)
    s.kinematics, s.time_step, s.gamma, s.actions = 0, 0.25, 0.9, p
    no_device = not torch.cuda.is_available()
    for B, H in SIZE_CASES[1:]:
        calls = ((lib.gcn_predict_workspace_bytes(B, H, 81),
                  lambda n: lib.gcn_predict_f32(ctypes.byref(g), p, p, B, H, p, n, p, p, p, None)),
                 (lib.sarl_predict_workspace_bytes(ctypes.byref(s), B, H),
                  lambda n: lib.sarl_predict_f32(ctypes.byref(s), p, p, B, H, p, n, p, p, p, p, None)))
        for need, call in calls:
            assert need > 0 and call(need - 1) == WORKSPACE and call(0) == WORKSPACE
            if no_device:
                assert call(need) not in (WORKSPACE, 0, -1, -2, -3)          # past every check: the first launch finds no device
