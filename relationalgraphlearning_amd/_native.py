"""ctypes binding of librgl_hip.so (the C ABI declared in include/rgl_hip.h).

There is deliberately NO fallback: if the shared library is missing or a call fails, the product
raises.  The CPU oracle under `oracle/` is test infrastructure and is never imported from here.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RGL_HIP_LIBRARY") or os.path.join(_HERE, "lib", "librgl_hip.so")   # override: debug builds only

MAX_MLP_LAYERS = 6
MAX_GCN_LAYERS = 8
MAX_NODES = 128
MAX_XDIM = 64
MAX_WIDTH = 256
MAX_ACTIONS = 256
ABI_VERSION = 8
MSE_WORKSPACE_BYTES = 2048

SIMILARITY = {"embedded_gaussian": 0, "gaussian": 1, "cosine": 2, "cosine_softmax": 3, "concatenation": 4,
              "squared": 5, "equal_attention": 6, "diagonal": 7}
KINEMATICS = {"holonomic": 0, "unicycle": 1}
CONTRACTION_DTYPES = {"f32": 0, "f16": 1, "bf16x6": 3}      # 2 was "f16x3" (ABI 4..7)

ERRORS = {-1: "RGL_ERR_BAD_SHAPE", -2: "RGL_ERR_BAD_MODE", -3: "RGL_ERR_NULL", -4: "RGL_ERR_WORKSPACE",
          -5: "RGL_ERR_LDS"}

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int)
c_double_p = C.POINTER(C.c_double)


class RglMlp(C.Structure):
    _fields_ = [("n_layers", C.c_int), ("last_relu", C.c_int), ("dims", C.c_int * (MAX_MLP_LAYERS + 1)),
                ("weight", C.c_void_p * MAX_MLP_LAYERS), ("bias", C.c_void_p * MAX_MLP_LAYERS)]


class RglTransposeJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int)]


class RglGatherJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_floats", C.c_int), ("src_rows", C.c_int)]


class RglRowsPlan(C.Structure):
    _fields_ = [("kind", C.c_int), ("coop", C.c_int), ("waves_per_wg", C.c_int), ("n_waves", C.c_int), ("n_tiles", C.c_int),
                ("n_wgs", C.c_int), ("direct", C.c_int), ("reserved", C.c_int), ("lds_bytes", C.c_size_t)]


class RglGraphTilesPlan(C.Structure):
    _fields_ = [("covered", C.c_int), ("node_tiles", C.c_int), ("feature_tiles", C.c_int), ("layers", C.c_int), ("family", C.c_int),
                ("norm", C.c_int), ("grid", C.c_int), ("resident", C.c_int), ("lds_bytes", C.c_size_t)]


class RglSceneBackwardPlan(C.Structure):
    _fields_ = [("fits", C.c_int), ("n_params", C.c_int), ("threads", C.c_int), ("grid", C.c_int), ("scenes_per_wg", C.c_int),
                ("reserved", C.c_int), ("lds_bytes", C.c_size_t)]


class RglPrologueEmbeddingPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("prologue", "parents_per_wg", "workgroups", "chunk_parents", "chunk_crowds", "human_tiles",
                                       "robot_tiles", "row_floats", "chunks_per_wg", "reserved")]


class RglGraph(C.Structure):
    _fields_ = [("w_r", RglMlp), ("w_h", RglMlp), ("x_dim", C.c_int), ("num_layer", C.c_int),
                ("similarity", C.c_int), ("layerwise_graph", C.c_int), ("skip_connection", C.c_int),
                ("reserved", C.c_int), ("w_a", C.c_void_p), ("w_a_mlp", RglMlp),
                ("Ws", C.c_void_p * MAX_GCN_LAYERS)]


class GcnPlanner(C.Structure):
    _fields_ = [("graph", RglGraph), ("value_head", RglMlp), ("kinematics", C.c_int), ("num_actions", C.c_int),
                ("time_step", C.c_double), ("gamma", C.c_double), ("actions", C.c_void_p),
                ("root_robot_f64", C.c_void_p), ("root_humans_f64", C.c_void_p), ("contraction_dtype", C.c_int), ("reserved", C.c_int)]


SARL_MAX_HUMANS = 127


class SarlPlanner(C.Structure):
    _fields_ = [("mlp1", RglMlp), ("mlp2", RglMlp), ("attention", RglMlp), ("mlp3", RglMlp), ("with_global_state", C.c_int),
                ("om_channel_size", C.c_int), ("cell_num", C.c_int), ("kinematics", C.c_int), ("cell_size", C.c_double),
                ("num_actions", C.c_int), ("contraction_dtype", C.c_int), ("time_step", C.c_double), ("gamma", C.c_double),
                ("actions", C.c_void_p), ("root_robot_f64", C.c_void_p), ("root_humans_f64", C.c_void_p)]


class LstmPlanner(C.Structure):
    _fields_ = [("mlp1", RglMlp), ("mlp", RglMlp), ("weight_ih", C.c_void_p), ("weight_hh", C.c_void_p), ("bias_ih", C.c_void_p),
                ("bias_hh", C.c_void_p), ("with_interaction_module", C.c_int), ("lstm_hidden_dim", C.c_int),
                ("om_channel_size", C.c_int), ("cell_num", C.c_int), ("cell_size", C.c_double), ("kinematics", C.c_int),
                ("num_actions", C.c_int), ("contraction_dtype", C.c_int), ("reserved", C.c_int), ("time_step", C.c_double),
                ("gamma", C.c_double), ("actions", C.c_void_p)]


SARL_LAYERS = 11


class SarlGrads(C.Structure):
    _fields_ = [("weight", C.c_void_p * SARL_LAYERS), ("bias", C.c_void_p * SARL_LAYERS)]


class MprlPlanner(C.Structure):
    _fields_ = [("value_graph", RglGraph), ("value_head", RglMlp), ("predictor_graph", RglGraph),
                ("motion_head", RglMlp), ("linear_state_predictor", C.c_int), ("kinematics", C.c_int),
                ("num_actions", C.c_int), ("planning_depth", C.c_int), ("planning_width", C.c_int),
                ("do_action_clip", C.c_int), ("sparse_search", C.c_int), ("contraction_dtype", C.c_int),
                ("time_step", C.c_double), ("gamma_bar", C.c_double), ("actions", C.c_void_p),
                ("action_groups", C.c_void_p), ("root_robot_f64", C.c_void_p), ("root_humans_f64", C.c_void_p),
                ("children_image", C.c_void_p), ("predictor_image", C.c_void_p), ("action_speed_bound", C.c_double)]


class RglDeepChildrenPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("covered", "node_tiles", "child_tiles", "table_stride", "layers", "norm", "f16", "skip", "t4", "fuse_head",
                 "parents_per_wg", "grid", "workgroups_per_cu", "reserved")] + [("lds_bytes", C.c_size_t)]


class RglTwoStageChildrenPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("pair", "hr", "node_tiles", "child_tiles", "sld", "norm", "skip", "image", "grid", "parents_per_wg",
                 "head_variant", "head_grid", "head_tiles", "head_tiles_per_wave")] + \
               [("lds_bytes", C.c_size_t), ("head_lds_bytes", C.c_size_t)]


class RglValueChildrenPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("family", "refusal", "fused_mode", "own_image", "f16", "pair_image")]


class RglSceneForwardPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("covered", "node_tiles", "family", "waves", "split", "embed_inside", "bx", "slots", "grid", "grid_cap", "last_steps",
                 "children_riding", "embed_launch", "reserved")] + [("lds_bytes", C.c_size_t)]


class CrowdSimConfig(C.Structure):
    _fields_ = [("time_step", C.c_double), ("time_limit", C.c_double), ("success_reward", C.c_double),
                ("collision_penalty", C.c_double), ("discomfort_dist", C.c_double),
                ("discomfort_penalty_factor", C.c_double), ("kinematics", C.c_int), ("human_policy", C.c_int)]


class CrowdOrcaParams(C.Structure):
    _fields_ = [("time_step", C.c_double), ("neighbor_dist", C.c_double), ("time_horizon", C.c_double),
                ("safety_space", C.c_double), ("max_neighbors", C.c_int), ("max_speed_rule", C.c_int), ("reserved", C.c_int)]


CROWD_ORCA_MAX_NEIGHBORS = 32
ORCA_MAX_SPEED_RULES = {"one": 0, "v_pref": 1}


class CrowdSceneConfig(C.Structure):
    _fields_ = [("circle_radius", C.c_double), ("square_width", C.c_double), ("discomfort_dist", C.c_double),
                ("robot_radius", C.c_double), ("robot_v_pref", C.c_double), ("human_radius", C.c_double),
                ("human_v_pref", C.c_double), ("scenario", C.c_int), ("randomize_attributes", C.c_int),
                ("max_attempts", C.c_int), ("reserved", C.c_int)]


CROWD_SCENARIOS = {"circle_crossing": 0, "square_crossing": 1}


class MprlLevelView(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in
                ("n_parents", "robot_off", "humans_off", "humans_next_off", "child_robot_off", "reward_off",
                 "child_value_off", "value1_off", "keep_off", "backup_off", "best_slot_off", "reward_clip_off")]


REPLAY_MAX_RUNS = 2
REPLAY_MAX_FIELDS = 6
REPLAY_LAYOUTS = {"mprl": 0, "gcn": 1}


class RglReplayRun(C.Structure):
    _fields_ = [("first", C.c_longlong), ("slot", C.c_longlong), ("count", C.c_longlong)]


class RglReplayPushJob(C.Structure):
    _fields_ = [("robot", C.c_void_p), ("humans", C.c_void_p), ("rewards", C.c_void_p), ("info", C.c_void_p),
                ("T", C.c_int), ("B", C.c_int), ("H", C.c_int), ("layout", C.c_int), ("kinematics", C.c_int),
                ("imitation_learning", C.c_int), ("step_discount", C.c_double), ("capacity", C.c_longlong),
                ("fields", C.c_void_p * REPLAY_MAX_FIELDS), ("n_runs", C.c_int), ("reserved", C.c_int),
                ("runs", RglReplayRun * REPLAY_MAX_RUNS), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class RglReplaySarlRows(C.Structure):
    _fields_ = [("cell_num", C.c_int), ("cell_size", C.c_double), ("channels", C.c_int)]      # channels 0: no maps, D = 13


EXPLORE_STATE_WORDS = 625


class CrowdExploreJob(C.Structure):
    _fields_ = [("greedy", C.c_void_p), ("done", C.c_void_p), ("table", C.c_void_p), ("state", C.c_void_p),
                ("chosen", C.c_void_p), ("action", C.c_void_p), ("explored", C.c_void_p), ("epsilon", C.c_double),
                ("B", C.c_int), ("n_actions", C.c_int), ("stream", C.c_void_p)]


class CrowdNonstopJob(C.Structure):
    _fields_ = [("sim", CrowdSimConfig), ("scene", CrowdSceneConfig), ("robot", C.c_void_p), ("humans", C.c_void_p),
                ("human_goals", C.c_void_p), ("human_vpref", C.c_void_p), ("robot_action", C.c_void_p),
                ("human_actions", C.c_void_p), ("time", C.c_void_p), ("done", C.c_void_p), ("state", C.c_void_p),
                ("status", C.c_void_p), ("attempts", C.c_void_p), ("reward", C.c_void_p), ("info", C.c_void_p),
                ("dmin", C.c_void_p), ("B", C.c_int), ("H", C.c_int), ("policy_draws", C.c_int), ("reserved", C.c_int),
                ("stream", C.c_void_p)]


# name -> (restype, argtypes); every symbol include/rgl_hip.h declares
SIGNATURES = {
    "rgl_graph_forward_workspace_bytes": (C.c_size_t, [C.POINTER(RglGraph), C.POINTER(RglMlp), C.POINTER(RglMlp), C.c_int,
                                                       C.c_int, C.c_int]),
    "rgl_graph_forward_f32": (C.c_int, [C.POINTER(RglGraph), C.POINTER(RglMlp), C.POINTER(RglMlp), C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rgl_graph_param_count": (C.c_int, [C.POINTER(RglGraph), C.POINTER(RglMlp), C.POINTER(RglMlp)]),
    "rgl_graph_backward_workspace_bytes": (C.c_size_t, [C.POINTER(RglGraph), C.POINTER(RglMlp), C.POINTER(RglMlp), C.c_int]),
    "rgl_graph_backward_f32": (C.c_int, [C.POINTER(RglGraph), C.POINTER(RglMlp), C.POINTER(RglMlp), C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    "rgl_plan_mlp_rows": (C.c_int, [C.POINTER(RglMlp), C.c_int, C.c_int, C.POINTER(RglRowsPlan)]),
    "rgl_plan_graph_tiles": (C.c_int, [C.POINTER(RglGraph), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RglGraphTilesPlan)]),
    "rgl_plan_scene_backward": (C.c_int, [C.POINTER(RglGraph), C.POINTER(RglMlp), C.POINTER(RglMlp), C.c_int, C.c_int,
                                          C.POINTER(RglSceneBackwardPlan)]),
    "rgl_plan_prologue_embedding": (C.c_int, [C.POINTER(MprlPlanner), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RglPrologueEmbeddingPlan)]),
    "rgl_plan_deep_children": (C.c_int, [C.POINTER(MprlPlanner), C.c_int, C.c_int, C.c_int, C.POINTER(RglDeepChildrenPlan)]),
    "rgl_plan_two_stage_children": (C.c_int, [C.POINTER(MprlPlanner), C.c_int, C.c_int, C.c_int, C.POINTER(RglTwoStageChildrenPlan)]),
    "rgl_plan_value_children": (C.c_int, [C.POINTER(MprlPlanner), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RglValueChildrenPlan)]),
    "rgl_plan_scene_forward": (C.c_int, [C.POINTER(RglGraph), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(RglSceneForwardPlan)]),
    "rgl_transpose_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "rgl_transpose_many_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "rgl_gather_rows_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "rgl_mse_step_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "gcn_rotate_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gcn_prepare_f32": (C.c_int, [C.POINTER(GcnPlanner), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "gcn_predict_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "gcn_predict_f32": (C.c_int, [C.POINTER(GcnPlanner), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                  C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mprl_expand_f32": (C.c_int, [C.POINTER(MprlPlanner), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                  C.c_void_p]),
    "mprl_value_children_workspace_bytes": (C.c_size_t, [C.POINTER(MprlPlanner), C.c_int, C.c_int]),
    "mprl_children_image_bytes": (C.c_size_t, [C.POINTER(MprlPlanner)]),
    "mprl_pack_children_image_f32": (C.c_int, [C.POINTER(MprlPlanner), C.c_void_p, C.c_size_t, C.c_void_p]),
    "mprl_predictor_image_bytes": (C.c_size_t, [C.POINTER(MprlPlanner)]),
    "mprl_pack_predictor_image_f32": (C.c_int, [C.POINTER(MprlPlanner), C.c_void_p, C.c_size_t, C.c_void_p]),
    "mprl_value_children_f32": (C.c_int, [C.POINTER(MprlPlanner), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    "mprl_tree_workspace_bytes": (C.c_size_t, [C.POINTER(MprlPlanner), C.c_int, C.c_int]),
    "mprl_tree_search_f32": (C.c_int, [C.POINTER(MprlPlanner), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "mprl_tree_search_traced_f32": (C.c_int, [C.POINTER(MprlPlanner), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, c_float_p, c_float_p, c_float_p]),
    "mprl_estimate_reward_f32": (C.c_int, [C.POINTER(MprlPlanner), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "mprl_action_clip_f32": (C.c_int, [C.POINTER(MprlPlanner), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "mprl_tree_level_view": (C.c_int, [C.POINTER(MprlPlanner), C.c_int, C.c_int, C.c_int, C.POINTER(MprlLevelView)]),
    "crowd_step_f64": (C.c_int, [C.POINTER(CrowdSimConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "crowd_observe_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "crowd_orca_humans_f64": (C.c_int, [C.POINTER(CrowdOrcaParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "crowd_orca_robot_f64": (C.c_int, [C.POINTER(CrowdOrcaParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    "crowd_generate_scenes_f64": (C.c_int, [C.POINTER(CrowdSceneConfig), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rgl_replay_push_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "rgl_replay_push_f32": (C.c_int, [C.POINTER(RglReplayPushJob)]),
    "rgl_replay_push_sarl_f32": (C.c_int, [C.POINTER(RglReplayPushJob), C.POINTER(RglReplaySarlRows)]),
    "crowd_explore_seed_u32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "crowd_explore_select_f64": (C.c_int, [C.POINTER(CrowdExploreJob)]),
    "crowd_step_nonstop_f64": (C.c_int, [C.POINTER(CrowdNonstopJob)]),
    "sarl_occupancy_maps_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int,
                                          C.c_void_p, C.c_void_p]),
    "sarl_value_workspace_bytes": (C.c_size_t, [C.POINTER(SarlPlanner)]),
    "sarl_value_workspace_bytes_for": (C.c_size_t, [C.POINTER(SarlPlanner), C.c_int, C.c_int]),
    "sarl_value_f32": (C.c_int, [C.POINTER(SarlPlanner), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sarl_predict_workspace_bytes": (C.c_size_t, [C.POINTER(SarlPlanner), C.c_int, C.c_int]),
    "sarl_predict_f32": (C.c_int, [C.POINTER(SarlPlanner), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sarl_train_workspace_bytes": (C.c_size_t, [C.POINTER(SarlPlanner), C.c_int, C.c_int]),
    "sarl_value_train_f32": (C.c_int, [C.POINTER(SarlPlanner), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "sarl_value_backward_f32": (C.c_int, [C.POINTER(SarlPlanner), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                          C.POINTER(SarlGrads), C.c_void_p]),
    "lstm_value_workspace_bytes": (C.c_size_t, [C.POINTER(LstmPlanner)]),
    "lstm_value_f32": (C.c_int, [C.POINTER(LstmPlanner), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lstm_predict_workspace_bytes": (C.c_size_t, [C.POINTER(LstmPlanner), C.c_int, C.c_int]),
    "lstm_predict_f32": (C.c_int, [C.POINTER(LstmPlanner), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                   C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rgl_switch_name": (C.c_char_p, [C.c_int]),
    "rgl_switch_parse": (C.c_int, [C.c_int, C.c_char_p, C.POINTER(C.c_int)]),
    "rgl_abi_version": (C.c_int, []),
    "rgl_build_target": (C.c_char_p, []),
}

# Exports added within an ABI version (host-only planners, the replay push, the exploration kernels, the switch table): an older build of the same version (RGL_HIP_LIBRARY:
# the A/B of two builds under one Python tree) lacks them and still loads; asking such a build for one raises AttributeError.
ADDITIVE = {"rgl_plan_prologue_embedding", "rgl_plan_deep_children", "rgl_plan_two_stage_children", "rgl_plan_value_children", "rgl_plan_scene_forward", "rgl_plan_scene_backward", "rgl_replay_push_workspace_bytes", "rgl_replay_push_f32",
            "crowd_explore_seed_u32", "crowd_explore_select_f64", "crowd_step_nonstop_f64", "sarl_occupancy_maps_f32", "sarl_value_workspace_bytes",
            "sarl_value_f32", "sarl_predict_workspace_bytes", "sarl_predict_f32", "sarl_value_workspace_bytes_for",
            "sarl_train_workspace_bytes", "sarl_value_train_f32", "sarl_value_backward_f32", "rgl_replay_push_sarl_f32",
            "lstm_value_workspace_bytes", "lstm_value_f32", "lstm_predict_workspace_bytes", "lstm_predict_f32",
            "rgl_switch_name", "rgl_switch_parse"}

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def lib():
    """The loaded library; raises NativeLibraryError (never falls back) when it cannot be used."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                "librgl_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C relationalgraphlearning_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                if name in ADDITIVE:
                    continue
                raise NativeLibraryError("librgl_hip.so lacks symbol %s" % name) from e
            fn.restype = res
            fn.argtypes = args
        if handle.rgl_abi_version() != ABI_VERSION:
            raise NativeLibraryError("librgl_hip.so ABI %d != expected %d" % (handle.rgl_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


def poison_workspaces():
    """RGL_DEBUG_POISON_WORKSPACES=1 (tests): workspaces and output slabs are filled with NaN bit patterns before the kernels run, so
    that a read of memory no kernel has written shows up as NaN instead of as whatever the allocator handed out."""
    return os.environ.get("RGL_DEBUG_POISON_WORKSPACES", "0") == "1"


def check(rc, what):
    if rc == 0:
        return
    if rc in ERRORS:
        raise NativeLibraryError("%s failed: %s" % (what, ERRORS[rc]))
    raise NativeLibraryError("%s failed: hipError_t %d" % (what, rc))
