// rgl_tree.hip -- the model-predictive rollout on device (path M) and the one-step search of
// path G (its prepare and select steps: rgl_onestep.h).  Level-synchronous: every tree level is a handful of launches over ALL parents of
// that level, no host round trip, no allocation (caller-provided workspace) -> capturable in a
// hipGraph.
//
// Follows (reference paths): crowd_nav/policy/model_predictive_rl.py:192-357 (predict,
// action_clip, V_planning, estimate_reward), state_predictor.py:41-60,109-118,
// crowd_sim/envs/utils/utils.py:4-26, multi_human_rl.py:36-96, cadrl.py:113-138,241-276.
#include "rgl_scene_body.h"
#include "rgl_onestep.h"

#include <cstdlib>

namespace {

constexpr int kBlock = 256;

// One thread per (parent, action): next robot state + estimate_reward (rgl_children.h); a wave's 64 pairs share the far-human
// masks of their (at most two) parents when the table and the crowd allow it (children_wave).
__global__ void mprl_children_kernel(const ChildrenArgs ca) {
    const long long total = (long long)ca.P * ca.A;
    const long long idx0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) & ~63LL;      // my wave's first pair
    if (ca.A >= 64 && ca.H <= 64 && !ca.robot64) {
        if (idx0 < total) children_wave(ca, idx0, total, table_speed_bound(ca));
    } else {
        const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (idx < total) children_thread(ca, idx);
    }
}

__global__ void linear_humans_kernel(const float* __restrict__ humans, float* __restrict__ out, long long n_rows) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const float* h = humans + i * 5;
    float* o = out + i * 5;
    o[0] = __fadd_rn(h[0], h[2]);       // no time-step factor (state_predictor.py:115-116)
    o[1] = __fadd_rn(h[1], h[3]);
    o[2] = h[2];
    o[3] = h[3];
    o[4] = h[4];
}

__global__ void gather_parent_humans_kernel(const float* __restrict__ humans, int humans_per, int H, long long P,
                                            float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * H * 5) return;
    const long long p = i / (H * 5), rest = i - p * (H * 5);
    out[i] = humans[(p / humans_per) * H * 5 + rest];
}

// One WAVE per parent (tail_select, rgl_tail.h): one-step values, top-w clipping, next level's robot states; at the deepest
// level also the leaf values and the parent's own back-up step.
__global__ __launch_bounds__(256) void mprl_select_kernel(const TailArgs t) {
    __shared__ int kept_lds[4][kTailLdsInts];            // per wave: kept indices | V(child) | rewards (tail_select)
    const int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= t.lv[t.level].P) return;
    tail_select(t, p, kept_lds[threadIdx.x >> 6]);
}

// value1 = reward + gamma_bar * V(child), each op rounded to fp32 like the reference's tensor arithmetic
__global__ void one_step_value_kernel(const float* __restrict__ r, const float* __restrict__ v, float g, long long n,
                                      float* __restrict__ o) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = f32_add(r[i], f32_mul(g, v[i]));      // two roundings (rgl_common.h)
}

// Level l >= 1, one thread per parent (tail_backup); 16 lanes per root (tail_root).
__global__ void mprl_backup_kernel(const TailArgs t, int l) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < t.lv[l].P) tail_backup(t, l, p);
}

__global__ void mprl_root_kernel(const TailArgs t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = i / kRootLanes;
    tail_root(t, b, i % kRootLanes, b < t.B);
}

// ------------------------------------------------------------------------------------------------
// path G
// ------------------------------------------------------------------------------------------------
__global__ void gcn_rotate_kernel(const float* __restrict__ in14, float* __restrict__ out13, int R, int unicycle) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    float s[14], o[13];
#pragma unroll
    for (int k = 0; k < 14; ++k) s[k] = in14[(size_t)i * 14 + k];
    rotate_row(s, unicycle, o);
#pragma unroll
    for (int k = 0; k < 13; ++k) out13[(size_t)i * 13 + k] = o[k];
}

inline dim3 grid_for(long long n, int block = kBlock) { return dim3((unsigned)((n + block - 1) / block)); }

// ------------------------------------------------------------------------------------------------
// workspace layout of the tree search
// ------------------------------------------------------------------------------------------------
// Byte offsets into the search's workspace (MprlLevelView reports them): one Carver walk, its `off` before each take.
struct LevelLayout {
    long long P;
    long long robot, humans, humans_next, child_robot, reward, child_value, value1, keep, backup, best_slot;
    long long reward_clip;      // level 0 only (-1 elsewhere): the root rewards as upstream's action_clip reads them
};
struct TreeLayout {
    LevelLayout lv[8];
    long long scratch, scratch_bytes;      // the children workspace (rgl::carve_children) of the widest (= deepest) level, shared by all
    long long scene_image;                 // three-piece bf16 image of the state predictor's scene kernel, packed once per search unless
                                           // the caller hands one in (scene_image_bytes: 0 = none)
    long long bytes;
};

inline int plan_levels(const MprlPlanner& pl, int B, int H, TreeLayout* t) {
    const int A = pl.num_actions, D = pl.planning_depth;
    const int W = pl.do_action_clip ? pl.planning_width : A;
    Carver c{nullptr, 0};
    auto take = [&c](long long bytes) { const long long at = c.off; c.take<char>(bytes); return at; };
    long long P = B;
    for (int l = 0; l < D; ++l) {
        LevelLayout& L = t->lv[l];
        L.P = P;
        L.robot = take(l == 0 ? 0 : P * 9 * 4);                                     // level 0 reads the caller's arrays
        L.humans = l > 0 ? t->lv[l - 1].humans_next : -1;
        L.humans_next = take(P * H * 5 * 4);
        L.child_robot = take(P * A * 9 * 4);
        L.reward = take(P * A * 4);
        L.reward_clip = l == 0 ? take(P * A * 4) : -1;
        L.child_value = take(P * A * 4);
        L.value1 = take(P * A * 4);
        L.keep = take(P * W * 4);
        L.backup = take(P * W * 4);
        L.best_slot = take(P * 4);
        if (l + 1 < D) P *= W;
        if (P > (1ll << 31) / (A * 9)) return RGL_ERR_BAD_SHAPE;
    }
    t->scratch_bytes = (long long)rgl::carve_children(nullptr, &pl, (int)P, H).bytes;
    t->scratch = take(t->scratch_bytes);
    t->scene_image = take((long long)rgl::scene_image_bytes(&pl));
    t->bytes = c.off;
    return RGL_OK;
}

// The action table and the kinematics of a planner.  Path M reports a missing table as RGL_ERR_NULL, after the kinematics; path G
// (`path_g`) as a shape error, before them.
inline int validate_actions(int num_actions, const double* actions, int kinematics, bool path_g) {
    if (num_actions < 1 || num_actions > RGL_MAX_ACTIONS || (path_g && !actions)) return RGL_ERR_BAD_SHAPE;
    if (kinematics != RGL_HOLONOMIC && kinematics != RGL_UNICYCLE) return RGL_ERR_BAD_MODE;
    return actions ? RGL_OK : RGL_ERR_NULL;
}

inline int validate_planner(const MprlPlanner& pl, int H) {
    // (an action count out of range is a shape error like the two below: which of them answers first does not show)
    if (pl.planning_depth < 1 || pl.planning_depth > 8) return RGL_ERR_BAD_SHAPE;
    if (pl.do_action_clip && (pl.planning_width < 1 || pl.planning_width > pl.num_actions)) return RGL_ERR_BAD_SHAPE;
    int rc = validate_actions(pl.num_actions, pl.actions, pl.kinematics, false);
    if (rc) return rc;
    if (pl.do_action_clip && pl.sparse_search && !pl.action_groups) return RGL_ERR_NULL;
    rc = rgl::validate_graph(pl.value_graph, H);
    if (rc) return rc;
    rc = rgl::validate_mlp(pl.value_head, pl.value_graph.x_dim, 1);
    if (rc) return rc;
    if (pl.value_graph.w_r.dims[0] != 9 || pl.value_graph.w_h.dims[0] != 5) return RGL_ERR_BAD_SHAPE;
    if (!pl.linear_state_predictor) {
        rc = rgl::validate_graph(pl.predictor_graph, H);
        if (rc) return rc;
        rc = rgl::validate_mlp(pl.motion_head, pl.predictor_graph.x_dim, 5);
        if (rc) return rc;
        if (pl.predictor_graph.w_r.dims[0] != 9 || pl.predictor_graph.w_h.dims[0] != 5) return RGL_ERR_BAD_SHAPE;
    }
    return RGL_OK;
}

// The reward / next-state work of P parents (mprl_children_kernel and the launches that carry it): whole-level arrays
inline ChildrenArgs children_args_for(const MprlPlanner& pl, const float* robot, const float* humans, int humans_per, int P, int H,
                                      int joint, float* child_robot, float* reward, float* reward_clip) {
    ChildrenArgs ca;
    ca.reward_clip = reward_clip;
    ca.robot = robot; ca.humans = humans; ca.humans_per = humans_per; ca.actions = pl.actions;
    ca.P = P; ca.H = H; ca.A = pl.num_actions; ca.kinematics = pl.kinematics; ca.dt = pl.time_step; ca.joint = joint;
    ca.child_robot = child_robot; ca.reward = reward;
    ca.v_max = pl.action_speed_bound > 0.0 ? (float)pl.action_speed_bound * 1.0001f : 0.f;
    ca.p_base = ca.c_base = 0;
    const bool roots64 = joint && humans_per == 1 && pl.root_robot_f64 && pl.root_humans_f64;
    ca.robot64 = roots64 ? pl.root_robot_f64 : nullptr;
    ca.humans64 = roots64 ? pl.root_humans_f64 : nullptr;
    return ca;
}

// One level: steps 1-3 of the header comment of mprl_expand_f32.  `ca`: the level's parents and their reward / next-state work;
// `vc`: the value-of-children call behind it (vc.humans_next = humans_next); `before_children`: null, or an event of a traced search
int expand_level(const MprlPlanner& pl, const ChildrenArgs& ca, float* humans_next, const rgl::ChildrenCall& vc, const float* sp_image,
                 hipEvent_t before_children) {
    const float* humans = ca.humans;
    const int humans_per = ca.humans_per, P = ca.P, H = ca.H;
    hipStream_t st = vc.stream;
    int children_done = 0;              // set when the state predictor's scene kernel ran them on its extra workgroups
    // The level as ONE launch where the fused children kernel's prologue form covers it (bf16x6, 17..20-node crowds, softmax
    // similarity): each workgroup runs the state predictor and the reward / next-state pairs of the parents it owns, then their
    // children.  Traced searches keep the three launches (predictor_ms / children_ms).  RGL_LEVEL_PROLOGUE=0: the three launches.
    LevelPrologue lp;
    const bool fold = level_prologue_enabled() && !before_children &&
                      rgl::level_prologue_args(&pl, ca, humans_next, sp_image, &lp) &&
                      rgl::fused_prologue_fits(&pl, P, H, vc.workspace_bytes, lp.scene_floats);
    if (fold) {
        rgl::ChildrenCall folded = vc;
        folded.prologue = &lp;
        return rgl::launch_value_children(&pl, folded);
    }
    // (Round 6: the reward work inside the children launch -- every workgroup for the parents it owns, in its prologue under the
    // weight image's DMA, inputs staged in LDS -- was built and measured: the embedding launch drops from 13.6 / 15.6 to 7.9 / 7.3 us,
    // the children launches grow by 7.3 / 5.9: 277.6 against 279.0 us per 2048-root step, not worth a second home for that code;
    // profiles/r06_p_timeline_rewards_in_children_ab.md.  The step is ~2-3 us of divergent float64 arithmetic per wave wherever it runs.)
    // (Running mprl_children_kernel beside the state predictor on a side stream was measured: the two overlap -- 34 us together
    // instead of 27 + 15 -- but the event fork / join costs more than that on the critical path: 0.405 vs 0.398 ms per step.)
    if (pl.linear_state_predictor) {
        if (humans_per == 1) {
            hipLaunchKernelGGL(linear_humans_kernel, grid_for((long long)P * H), dim3(kBlock), 0, st, humans, humans_next,
                               (long long)P * H);
        } else {
            hipLaunchKernelGGL(gather_parent_humans_kernel, grid_for((long long)P * H * 5), dim3(kBlock), 0, st, humans,
                               humans_per, H, (long long)P, humans_next);
            hipLaunchKernelGGL(linear_humans_kernel, grid_for((long long)P * H), dim3(kBlock), 0, st, humans_next,
                               humans_next, (long long)P * H);
        }
        RGL_LAUNCH_CHECK();
    } else {
        const rgl::ChildrenWorkspace w = rgl::carve_children_call(&pl, vc);
        int rc = rgl::launch_predict_humans(&pl, ca, humans_next, w.region, w.region_bytes, st, &children_done, sp_image);
        if (rc) return rc;
    }
    if (!children_done) {
        hipLaunchKernelGGL(mprl_children_kernel, grid_for((long long)P * ca.A), dim3(kBlock), 0, st, ca);
        RGL_LAUNCH_CHECK();
    }
    if (before_children) RGL_HIP_TRY(hipEventRecord(before_children, st));     // traced searches: state predictor | children
    return rgl::launch_value_children(&pl, vc);
}

// the value-of-children call of P parents of this planner: no tail, no image in the workspace
inline rgl::ChildrenCall children_call_for(const MprlPlanner& pl, const float* child_robot, const float* humans_next, int P, int H,
                                           float* child_value, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    rgl::ChildrenCall c{};
    c.child_robot = child_robot; c.humans_next = humans_next; c.child_value = child_value;
    c.P = P; c.A = pl.num_actions; c.H = H;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    c.image = pl.children_image;
    return c;
}

}  // namespace

extern "C" int mprl_expand_f32(const MprlPlanner* planner, const float* robot, const float* humans, int P, int H,
                               int parents_are_joint_states, float* humans_next, float* child_robot, float* reward,
                               float* child_value, float* value1, void* workspace, size_t workspace_bytes,
                               rgl_stream_t stream) {
    if (!planner || !robot || !humans || !humans_next || !child_robot || !reward || !child_value) return RGL_ERR_NULL;
    if (P < 0) return RGL_ERR_BAD_SHAPE;
    int rc = validate_planner(*planner, H);
    if (rc) return rc;
    if (P == 0) return RGL_OK;
    hipStream_t st = (hipStream_t)stream;
    rc = expand_level(*planner, children_args_for(*planner, robot, humans, 1, P, H, parents_are_joint_states, child_robot, reward, nullptr),
                      humans_next, children_call_for(*planner, child_robot, humans_next, P, H, child_value, workspace, workspace_bytes, st),
                      planner->predictor_image, nullptr);
    if (rc) return rc;
    if (value1) {
        const long long n = (long long)P * planner->num_actions;
        hipLaunchKernelGGL(one_step_value_kernel, grid_for(n), dim3(kBlock), 0, st, reward, child_value,
                           (float)planner->gamma_bar, n, value1);
        RGL_LAUNCH_CHECK();
    }
    return RGL_OK;
}

extern "C" size_t mprl_value_children_workspace_bytes(const MprlPlanner* planner, int P, int H) {
    if (!planner || P < 1 || H < 1) return 0;
    return rgl::carve_children(nullptr, planner, P, H).bytes;
}

extern "C" int mprl_value_children_f32(const MprlPlanner* planner, const float* child_robot, const float* humans_next,
                                       int P, int H, float* child_value, void* workspace, size_t workspace_bytes,
                                       rgl_stream_t stream) {
    if (!planner || !child_robot || !humans_next || !child_value) return RGL_ERR_NULL;
    if (P < 0) return RGL_ERR_BAD_SHAPE;
    int rc = validate_planner(*planner, H);
    if (rc) return rc;
    if (P == 0) return RGL_OK;
    return rgl::launch_value_children(planner, children_call_for(*planner, child_robot, humans_next, P, H, child_value, workspace,
                                                                 workspace_bytes, (hipStream_t)stream));
}

extern "C" size_t mprl_predictor_image_bytes(const MprlPlanner* planner) { return rgl::scene_image_bytes(planner); }

extern "C" int mprl_pack_predictor_image_f32(const MprlPlanner* planner, float* image, size_t image_bytes, rgl_stream_t stream) {
    if (!planner || !image) return RGL_ERR_NULL;
    const size_t need = rgl::scene_image_bytes(planner);
    if (!need) return RGL_ERR_BAD_MODE;
    if (image_bytes < need) return RGL_ERR_WORKSPACE;
    return rgl::pack_scene_image(planner, image, (hipStream_t)stream);
}

extern "C" size_t mprl_tree_workspace_bytes(const MprlPlanner* planner, int B, int H) {
    if (!planner || B < 1 || planner->planning_depth < 1 || planner->planning_depth > 8) return 0;
    TreeLayout t;
    return plan_levels(*planner, B, H, &t) ? 0 : (size_t)t.bytes;
}

extern "C" int mprl_tree_level_view(const MprlPlanner* planner, int B, int H, int level, MprlLevelView* view) {
    if (!planner || !view) return RGL_ERR_NULL;
    if (planner->planning_depth < 1 || planner->planning_depth > 8 || level < 0 || level >= planner->planning_depth)
        return RGL_ERR_BAD_SHAPE;
    TreeLayout t;
    int rc = plan_levels(*planner, B, H, &t);
    if (rc) return rc;
    const LevelLayout& L = t.lv[level];
    view->n_parents = L.P;
    view->robot_off = level == 0 ? -1 : L.robot;
    view->humans_off = L.humans;
    view->humans_next_off = L.humans_next;
    view->child_robot_off = L.child_robot;
    view->reward_off = L.reward;
    view->reward_clip_off = level == 0 && planner->do_action_clip ? L.reward_clip : -1;
    view->child_value_off = L.child_value;
    view->value1_off = L.value1;
    view->keep_off = L.keep;
    view->backup_off = L.backup;
    view->best_slot_off = L.best_slot;
    return RGL_OK;
}

namespace {
// `events`: null, or 3 * planning_depth + 1 hipEvent_t of the caller's (mprl_tree_search_traced_f32)
int tree_search(const MprlPlanner* planner, const float* robot, const float* humans, int B, int H,
                int roots_are_joint_states, void* workspace, size_t workspace_bytes,
                int* best_action, float* best_value, float* root_values, int* root_kept,
                rgl_stream_t stream, void* const* events) {
    if (!planner || !robot || !humans || !workspace || !best_action || !best_value) return RGL_ERR_NULL;
    if (B < 1) return RGL_ERR_BAD_SHAPE;
    int rc = validate_planner(*planner, H);
    if (rc) return rc;
    const MprlPlanner& pl = *planner;
    const int A = pl.num_actions, D = pl.planning_depth;
    const int W = pl.do_action_clip ? pl.planning_width : A;
    if (pl.do_action_clip && pl.sparse_search) {
        // the select kernel keeps the ids of the groups taken so far in kMaxSparseWidth registers
        if (W > kMaxSparseWidth) return RGL_ERR_BAD_MODE;
    }
    TreeLayout t;
    rc = plan_levels(pl, B, H, &t);
    if (rc) return rc;
    if ((long long)workspace_bytes < t.bytes) return RGL_ERR_WORKSPACE;
    const LevelLayout* lv = t.lv;
    char* ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const float gamma_f = (float)pl.gamma_bar;

    // weight images of the value-of-children kernels: prepared once, every level copies them into LDS (0 = prepared)
    // (or handed in by the caller, packed once for fixed weights: MprlPlanner::children_image)
    const rgl::FusedImageMode image_mode = pl.contraction_dtype == RGL_CONTRACT_BF16X6 ? rgl::kModeBx : rgl::kModeF32;
    int image_ready = 0;
    if (pl.contraction_dtype == RGL_CONTRACT_F32 || image_mode != rgl::kModeF32) {
        const int P_max = (int)lv[D - 1].P;
        if (pl.children_image) image_ready = 1;
        else if (rgl::fused_children_covers(&pl.value_graph, &pl.value_head, P_max, A, H, image_mode)) {
            // (the slot's place does not depend on P: every level's call finds the image there)
            rc = rgl::pack_children_images(&pl.value_graph, &pl.value_head, P_max, A, H,
                                           rgl::carve_children(ws + t.scratch, &pl, P_max, H).image, st, image_mode);
            if (rc) return rc;
            image_ready = 1;
        }
    }
    const float* sp_image = pl.predictor_image;
    if (!sp_image && rgl::scene_image_bytes(&pl)) {
        float* img = (float*)(ws + t.scene_image);
        rc = rgl::pack_scene_image(&pl, img, st);
        if (rc) return rc;
        sp_image = img;
    }
    TailArgs tail{};
    tail.enabled = 1;
    tail.D = D; tail.A = A; tail.W = W; tail.clip = pl.do_action_clip; tail.sparse = pl.sparse_search;
    tail.gamma_f = gamma_f;
    tail.groups = pl.action_groups;
    for (int l = 0; l < D; ++l) {
        const LevelLayout& L = lv[l];
        tail.lv[l] = TailLevel{(const float*)(ws + L.reward), (const float*)(ws + L.child_value), (int*)(ws + L.keep),
                               (float*)(ws + L.backup), (int*)(ws + L.best_slot), (int)L.P};
    }
    tail.B = B;
    tail.best_action = best_action; tail.best_value = best_value; tail.root_values = root_values; tail.root_kept = root_kept;
    int chain_done = 0;              // the deepest level's children kernel also ran the back-up steps and the root step
    for (int l = 0; l < D; ++l) {
        const LevelLayout& L = lv[l];
        const int P = (int)L.P;
        const float* pr = l == 0 ? robot : (const float*)(ws + L.robot);
        const float* ph = l == 0 ? humans : (const float*)(ws + L.humans);
        const int humans_per = l == 0 ? 1 : W;
        const bool deepest = l + 1 == D;
        tail.level = l;
        tail.child_robot = (const float*)(ws + L.child_robot);
        tail.value1 = (float*)(ws + L.value1);
        tail.next_robot = deepest ? nullptr : (float*)(ws + lv[l + 1].robot);
        tail.chain = deepest;
        // Joint-state roots of a clipped search: upstream clips the root on the TENSOR state (model_predictive_rl.py:216-218 ->
        // :246-248, float32-born scalars) and prices the kept actions on the float64 JointState (:226) -- two reward arrays at
        // level 0, the first for the selection, the second for the root values.
        float* reward_clip = l == 0 && roots_are_joint_states && pl.do_action_clip ? (float*)(ws + L.reward_clip) : nullptr;
        tail.reward_sel = reward_clip;
        int tail_done = 0;           // 1: the children kernel selected for its parents; 2: ... and finished the search (deepest level)
        if (events) RGL_HIP_TRY(hipEventRecord((hipEvent_t)events[3 * l], st));
        float* humans_next = (float*)(ws + L.humans_next);
        rgl::ChildrenCall vc = children_call_for(pl, tail.child_robot, humans_next, P, H, (float*)(ws + L.child_value), ws + t.scratch,
                                                 (size_t)t.scratch_bytes, st);
        vc.image_ready = image_ready; vc.tail = &tail; vc.tail_done = &tail_done;
        rc = expand_level(pl, children_args_for(pl, pr, ph, humans_per, P, H, l == 0 ? roots_are_joint_states : 0,
                                                (float*)(ws + L.child_robot), (float*)(ws + L.reward), reward_clip),
                          humans_next, vc, sp_image, events ? (hipEvent_t)events[3 * l + 1] : nullptr);
        if (rc) return rc;
        if (!tail_done) {
            // the deepest level's selection also writes the leaf values and (below the root) does its own back-up step
            hipLaunchKernelGGL(mprl_select_kernel, grid_for(P, 4), dim3(256), 0, st, tail);
            RGL_LAUNCH_CHECK();
        }
        if (events) RGL_HIP_TRY(hipEventRecord((hipEvent_t)events[3 * l + 2], st));
        if (deepest && tail_done == 2) chain_done = 1;
    }
    if (!chain_done) {
        for (int l = D - 2; l >= 1; --l) {
            hipLaunchKernelGGL(mprl_backup_kernel, grid_for(lv[l].P, 64), dim3(64), 0, st, tail, l);
            RGL_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(mprl_root_kernel, grid_for((long long)B * kRootLanes, 256), dim3(256), 0, st, tail);
        RGL_LAUNCH_CHECK();
    }
    if (events) RGL_HIP_TRY(hipEventRecord((hipEvent_t)events[3 * D], st));
    return RGL_OK;
}
}  // namespace

extern "C" int mprl_tree_search_f32(const MprlPlanner* planner, const float* robot, const float* humans, int B, int H,
                                    int roots_are_joint_states, void* workspace, size_t workspace_bytes,
                                    int* best_action, float* best_value, float* root_values, int* root_kept,
                                    rgl_stream_t stream) {
    return tree_search(planner, robot, humans, B, H, roots_are_joint_states, workspace, workspace_bytes, best_action, best_value,
                       root_values, root_kept, stream, nullptr);
}

extern "C" int mprl_tree_search_traced_f32(const MprlPlanner* planner, const float* robot, const float* humans, int B, int H,
                                           int roots_are_joint_states, void* workspace, size_t workspace_bytes,
                                           int* best_action, float* best_value, float* root_values, int* root_kept,
                                           rgl_stream_t stream, float* predictor_ms, float* children_ms, float* total_ms) {
    if (!planner || !predictor_ms || !children_ms) return RGL_ERR_NULL;
    const int D = planner->planning_depth;
    if (D < 1 || D > 8) return RGL_ERR_BAD_SHAPE;
    hipEvent_t ev[3 * 8 + 1];
    const int n = 3 * D + 1;
    for (int i = 0; i < n; ++i) {
        const hipError_t e = hipEventCreate(&ev[i]);
        if (e != hipSuccess) {                                   // give back what was created
            for (int k = 0; k < i; ++k) (void)hipEventDestroy(ev[k]);
            return (int)e;
        }
    }
    int rc = tree_search(planner, robot, humans, B, H, roots_are_joint_states, workspace, workspace_bytes, best_action, best_value,
                         root_values, root_kept, stream, reinterpret_cast<void* const*>(ev));
    if (rc == RGL_OK) rc = (int)hipEventSynchronize(ev[3 * D]);
    for (int l = 0; l < D && rc == RGL_OK; ++l) {
        rc = (int)hipEventElapsedTime(&predictor_ms[l], ev[3 * l], ev[3 * l + 1]);
        if (rc == RGL_OK) rc = (int)hipEventElapsedTime(&children_ms[l], ev[3 * l + 1], ev[3 * l + 2]);
    }
    if (rc == RGL_OK && total_ms) rc = (int)hipEventElapsedTime(total_ms, ev[0], ev[3 * D]);
    for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]);
    return rc;
}

// estimate_reward + compute_next_state for every (parent, action) pair on their own (model_predictive_rl.py:304-357,
// state_predictor.py:41-60): the kernel every tree level runs, exported for ModelPredictiveRL.estimate_reward
extern "C" int mprl_estimate_reward_f32(const MprlPlanner* planner, const float* robot, const float* humans, int P, int H,
                                        int parents_are_joint_states, float* child_robot, float* reward, rgl_stream_t stream) {
    if (!planner || !robot || !humans || !child_robot || !reward) return RGL_ERR_NULL;
    if (P < 0 || H < 1 || H + 1 > RGL_MAX_NODES) return RGL_ERR_BAD_SHAPE;
    const MprlPlanner& pl = *planner;
    const int rc = validate_actions(pl.num_actions, pl.actions, pl.kinematics, false);
    if (rc) return rc;
    if (P == 0) return RGL_OK;
    const ChildrenArgs ca = children_args_for(pl, robot, humans, 1, P, H, parents_are_joint_states, child_robot, reward, nullptr);
    hipLaunchKernelGGL(mprl_children_kernel, grid_for((long long)P * pl.num_actions), dim3(kBlock), 0, (hipStream_t)stream, ca);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

// action_clip's selection on its own (model_predictive_rl.py:242-269): value1 = reward + gamma_bar * child_value, then the
// planning_width best actions per parent (argpartition semantics; sparse: one action per group) -- tail_select, the step every
// search level runs, without the gather of the next level's states
extern "C" int mprl_action_clip_f32(const MprlPlanner* planner, const float* reward, const float* child_value, int P,
                                    float* value1, int* keep, rgl_stream_t stream) {
    if (!planner || !reward || !child_value || !value1 || !keep) return RGL_ERR_NULL;
    if (P < 0) return RGL_ERR_BAD_SHAPE;
    const MprlPlanner& pl = *planner;
    const int A = pl.num_actions;
    if (A < 1 || A > RGL_MAX_ACTIONS) return RGL_ERR_BAD_SHAPE;
    if (pl.do_action_clip && (pl.planning_width < 1 || pl.planning_width > A)) return RGL_ERR_BAD_SHAPE;
    const int W = pl.do_action_clip ? pl.planning_width : A;
    if (pl.do_action_clip && pl.sparse_search) {
        if (!pl.action_groups) return RGL_ERR_NULL;
        if (W > kMaxSparseWidth) return RGL_ERR_BAD_MODE;
    }
    if (P == 0) return RGL_OK;
    TailArgs t{};
    t.enabled = 1;
    t.level = 0; t.D = 2;                       // "not the deepest level": no leaf values, no back-up step
    t.A = A; t.W = W; t.clip = pl.do_action_clip; t.sparse = pl.sparse_search;
    t.gamma_f = (float)pl.gamma_bar;
    t.groups = pl.action_groups;
    t.child_robot = nullptr; t.next_robot = nullptr;
    t.value1 = value1;
    t.lv[0] = TailLevel{reward, child_value, keep, nullptr, nullptr, P};
    t.B = P;
    hipLaunchKernelGGL(mprl_select_kernel, grid_for(P, 4), dim3(256), 0, (hipStream_t)stream, t);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

// ------------------------------------------------------------------------------------------------
// path G entry points
// ------------------------------------------------------------------------------------------------
extern "C" int gcn_rotate_f32(const float* joint14, float* rotated13, int n_rows, int kinematics,
                              rgl_stream_t stream) {
    if (!joint14 || !rotated13) return RGL_ERR_NULL;
    if (n_rows < 0) return RGL_ERR_BAD_SHAPE;
    if (kinematics != RGL_HOLONOMIC && kinematics != RGL_UNICYCLE) return RGL_ERR_BAD_MODE;
    if (n_rows == 0) return RGL_OK;
    hipLaunchKernelGGL(gcn_rotate_kernel, grid_for(n_rows), dim3(kBlock), 0, (hipStream_t)stream, joint14, rotated13,
                       n_rows, kinematics == RGL_UNICYCLE);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

// propagate + rotate + compute_reward for the B x A candidate scenes of a one-step search on their own (ABI 5): the first launch of
// gcn_predict_f32 (cadrl.py:113-138,241-276, multi_human_rl.py:46-51,73-96), exported for GCN.compute_reward / tests
extern "C" int gcn_prepare_f32(const GcnPlanner* planner, const float* robot, const float* humans, int B, int H,
                               float* self6, float* hum7, float* reward, rgl_stream_t stream) {
    if (!planner || !robot || !humans || !self6 || !hum7 || !reward) return RGL_ERR_NULL;
    if (B < 1 || H < 1 || H + 1 > RGL_MAX_NODES) return RGL_ERR_BAD_SHAPE;
    const int rc = validate_actions(planner->num_actions, planner->actions, planner->kinematics, true);
    if (rc) return rc;
    return launch_gcn_prepare(planner->kinematics, planner->num_actions, planner->time_step, planner->actions, planner->root_robot_f64,
                              planner->root_humans_f64, robot, humans, B, H, self6, hum7, reward, (hipStream_t)stream);
}

namespace {

constexpr long long kGcnImageBytes = 64 * 1024;      // >= scene_image_bytes_for(): Wa + 4 layer matrices + motion-head slots as 6-byte weights

// gcn_predict_f32's workspace: rotated features, rewards, values | the scratch of the MFMA forward (embeddings [S][32], [S][H][32],
// value rows [S][64]) | room for the scene kernel's three-piece bf16 weight image (RGL_CONTRACT_BF16X6: packed per call, 4 layer
// matrices at most)
struct GcnPredictScratch {
    OneStepScratch one;
    void* fwd;
    float* image;
    size_t fwd_bytes;
    long long bytes;
};

inline GcnPredictScratch carve_gcn_predict(void* base, long long S, int H) {
    GcnPredictScratch w;
    w.one = carve_onestep(base, S, H);
    Carver c{(char*)base, w.one.bytes};
    w.fwd = c.take<char>(S * (32 + (long long)H * 32 + 64) * 4);
    w.fwd_bytes = (size_t)(c.off - w.one.bytes);
    w.image = c.take<float>(kGcnImageBytes);
    w.bytes = c.off;
    return w;
}

}  // namespace

extern "C" size_t gcn_predict_workspace_bytes(int B, int H, int A) {
    if (B < 1 || H < 1 || A < 1) return 0;
    return (size_t)carve_gcn_predict(nullptr, (long long)B * A, H).bytes;
}

extern "C" int gcn_predict_f32(const GcnPlanner* planner, const float* robot, const float* humans, int B, int H,
                               void* workspace, size_t workspace_bytes, float* action_values, int* best_action,
                               float* best_value, rgl_stream_t stream) {
    if (!planner || !robot || !humans || !workspace || !action_values || !best_action) return RGL_ERR_NULL;
    if (B < 1) return RGL_ERR_BAD_SHAPE;
    const GcnPlanner& pl = *planner;
    int rc = validate_actions(pl.num_actions, pl.actions, pl.kinematics, true);
    if (rc) return rc;
    rc = rgl::validate_graph(pl.graph, H);
    if (rc) return rc;
    if (pl.graph.w_r.dims[0] != 6 || pl.graph.w_h.dims[0] != 7) return RGL_ERR_BAD_SHAPE;
    rc = rgl::validate_mlp(pl.value_head, pl.graph.x_dim, 1);
    if (rc) return rc;
    if (pl.contraction_dtype != RGL_CONTRACT_F32 && pl.contraction_dtype != RGL_CONTRACT_BF16X6) return RGL_ERR_BAD_MODE;
    const int A = pl.num_actions;
    const long long S = (long long)B * A;
    const GcnPredictScratch w = carve_gcn_predict(workspace, S, H);
    if (workspace_bytes < (size_t)w.bytes) return RGL_ERR_WORKSPACE;
    float *self6 = w.one.self6, *hum7 = w.one.hum7, *reward = w.one.reward, *value = w.one.value;
    hipStream_t st = (hipStream_t)stream;
    // RGL_CONTRACT_BF16X6: the graph's Wa / W_l as three-piece bf16 fragments for the scene kernel's value-rows mode, packed here
    // (one ~4 us launch beside a forward of hundreds; the weights may have changed since the last call)
    const float* rows_image = nullptr;
    if (pl.contraction_dtype == RGL_CONTRACT_BF16X6) {
        const size_t ib = rgl::scene_image_bytes_for(pl.graph, nullptr);
        if (ib && ib <= kGcnImageBytes) {
            rc = rgl::pack_scene_image_for(pl.graph, nullptr, w.image, st);
            if (rc) return rc;
            rows_image = w.image;
        }
    }
    rc = launch_gcn_prepare(pl.kinematics, A, pl.time_step, pl.actions, pl.root_robot_f64, pl.root_humans_f64, robot, humans, B, H, self6,
                            hum7, reward, st);
    if (rc) return rc;
    // the B x A rotated scenes: one wave per scene on the MFMA kernel where it covers the model (the shipped ValueNetwork: 6 / 7
    // inputs, 64-32 embeddings, head 150-100-100-1), else the general kernel
    bool taken = rgl::scene_forward_covers(&pl.graph, &pl.value_head, nullptr, (int)S, 1, H, w.fwd_bytes);
    if (taken)
        rc = rgl::launch_scene_forward(&pl.graph, &pl.value_head, nullptr, self6, hum7, (int)S, 1, H, value, nullptr, w.fwd, w.fwd_bytes,
                                       st, rows_image);
    else      // other embedding MLPs (x_dim 32: what this workspace is sized for): the tile kernels of rgl_tile_pipeline.hip
        rc = rgl::launch_tiles_forward(&pl.graph, &pl.value_head, nullptr, self6, hum7, (int)S, 1, H, nullptr, value, nullptr, w.fwd,
                                       w.fwd_bytes, st, &taken);
    if (rc) return rc;
    if (!taken) {
        if (require_mfma_forward()) return RGL_ERR_BAD_MODE;
        rc = rgl::launch_generic_forward(&pl.graph, &pl.value_head, nullptr, self6, hum7, (int)S, 1, H, nullptr, nullptr, value,
                                         nullptr, st);
        if (rc) return rc;
    }
    return launch_onestep_select(robot, reward, value, nullptr, B, A, H, pl.gamma, pl.time_step, action_values, best_action, best_value,
                                 nullptr, st);
}
