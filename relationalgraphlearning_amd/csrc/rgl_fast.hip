// rgl_fast.hip -- "value of the sibling children" (mprl_value_children_f32): which kernel family takes a call, decided ONCE on the
// host (route_value_children: the ladder fused -> rank-1 -> deep -> tile -> scene -> tile pipeline -> general kernel, each rung the
// owning unit's own `.._covers` question), and the launch that follows it (launch_value_children: the route plus a switch).  A
// launcher's int is RGL_OK or an error, never "not mine" (rgl_common.h).  The f32-MFMA kernels themselves live in
//   rgl_rank1.hip  shared-crowd rank-1 form, L = 2, N <= 32 (the shipped configuration)
//   rgl_deep.hip   shared-crowd form for L in {2, 3}, N <= 60, optional f16-input MFMA contractions
//   rgl_tile.hip   every child's graph in full, any depth, N <= 64 (softmax similarities)
//   rgl_head.hip   stage 2: last GCN layer on the robot row + value head
//   rgl_scene.hip  the state predictor's graph forward (one scene per wave)
// f32 MFMA (v_mfma_f32_16x16x4_f32) is exact fp32 at the vector-FMA rate; results differ from the general kernel
// (rgl_generic.hip) only by summation order.  Anything outside these envelopes runs on the general kernel (same
// numbers, lower speed) -- never on the CPU.
#include "rgl_mfma.h"

namespace rgl {

// Which kernel takes the value-of-children call of P parents -- the ladder, written once: launch_value_children switches on the
// answer, rgl_plan_value_children / rgl_plan_deep_children / fused_prologue_fits report it.  Every condition is the owning unit's
// own question (.._covers: its plan's answer); nothing is launched, no device data is read.
ChildrenRoute route_value_children(const MprlPlanner* pl, int P, int H, size_t workspace_bytes, bool image_at_hand,
                                   int prologue_scene_floats) {
    ChildrenRoute r{};
    auto refuse = [&](int code) { r.family = kChildrenRefused; r.refusal = code; return r; };
    auto take = [&](ChildrenFamily f) { r.family = f; return r; };
    const RglGraph* g = &pl->value_graph;
    const RglMlp* head = &pl->value_head;
    const int A = pl->num_actions;
    const bool want_f16 = pl->contraction_dtype == RGL_CONTRACT_F16;
    // RGL_CONTRACT_BF16X6 (round 5): f32-WIDTH products (three bf16 pieces per operand, six terms) on the matrix pipe where a kernel
    // offers them -- the first 64 input features of the fused kernel's last head matrix; plain f32 everywhere else
    const bool want_b6 = pl->contraction_dtype == RGL_CONTRACT_BF16X6;
    if (pl->contraction_dtype != RGL_CONTRACT_F32 && !want_f16 && !want_b6) return refuse(RGL_ERR_BAD_MODE);      // (2, the split-f16 mode of ABI 4..7, is gone)
    const ChildrenWorkspace need = carve_children(nullptr, pl, P, H);      // the sizes alone
    const bool fits = workspace_bytes >= need.bytes;
    r.staged = head_variant(*head) >= 0 && fits;
    // packed weight image of the value estimator (the caller's, or this search's in the workspace's image slot): the two-stage pair
    // copies its weight images from it instead of building them from the raw matrices (most of a small launch)
    r.pair_image = r.staged && !want_b6 && image_at_hand;      // (a three-piece bf16 image is in the fused kernel's layout only)
    const bool prologue = prologue_scene_floats >= 0;
    if (r.staged && !want_f16) {
        // one fused kernel over 16-child tiles (L = 2, N <= 32, default head): values come out directly, no stage 2
        r.fused_mode = want_b6 ? kModeBx : kModeF32;
        if (fused_children_covers(g, head, P, A, H, r.fused_mode, prologue_scene_floats)) return take(kChildrenFused);
        // the bf16 hybrid image is larger: crowds of 21..32 agents (lane = feature row pass, larger wave scratch), and of 17..20 with a
        // plain-weight similarity (unpacked row pass: 172 944 bytes), do not fit a CU with it -- they run the f32 form of this kernel on
        // an f32 image the call packs itself (the caller's image is in the other layout; tests/test_bf16x6_kernels.py pins the envelope)
        if (want_b6 && !prologue && fused_children_covers(g, head, P, A, H, kModeF32)) {
            r.fused_mode = kModeF32;
            r.own_image = true;
            return take(kChildrenFused);
        }
    }
    if (prologue) return refuse(RGL_ERR_BAD_MODE);      // the caller skipped the level's other launches: only the prologue form runs them
    // stage 1, in order of preference: rank-1 (L = 2, N <= 32), shared-crowd deep (L in {2,3}, N <= 60), tiles (softmax
    // similarities, any depth, N <= 64); everything else, or a head without a stage-2 kernel: the general kernel
    if (r.staged) {
        if (!want_f16 && rank1_children_covers(g, P, A, H)) return take(kChildrenRank1);
        if (want_f16) {      // the deep kernel's three-layer form or nothing
            r.f16 = true;
            return g->num_layer == 3 && deep_children_covers(g, P, A, H, true) ? take(kChildrenDeep) : refuse(RGL_ERR_BAD_MODE);
        }
        if (deep_children_covers(g, P, A, H, false)) return take(kChildrenDeep);
        if (tile_children_covers(g, P, A, H)) return take(kChildrenTile);
        // every child's graph in full, one wave per child: the remaining similarity functions and layerwise graphs (`staged`: a
        // stage-2 head, and a workspace whose region holds scene_children_workspace_bytes)
        if (scene_children_covers(pl, H)) return take(kChildrenScene);
    }
    if (want_f16) return refuse(RGL_ERR_BAD_MODE);
    // outside the shipped shapes (other embedding MLPs, x_dim = 64): the tile kernels, the children of a parent sharing its crowd's rows
    if (tiles_forward_covers(g, head, nullptr, P * A, A, H, false, fits ? need.region_bytes : 0)) return take(kChildrenTilesForward);
    // RGL_REQUIRE_MFMA_CHILDREN=1 (tests): refuse instead of running the general VALU kernel
    return require_mfma_children() ?refuse(RGL_ERR_BAD_MODE) : take(kChildrenGeneric);
}

// V(child) for the A children of each of P parents; children of one parent share humans_next[p].
int launch_value_children(const MprlPlanner* pl, ChildrenCall c) {
    if (c.tail_done) *c.tail_done = 0;      // the launcher that runs the tail sets it
    const RglGraph* g = &pl->value_graph;
    const RglMlp* head = &pl->value_head;
    const ChildrenRoute r = route_value_children(pl, c.P, c.H, c.workspace ? c.workspace_bytes : 0, c.image || c.image_ready,
                                                 c.prologue ? c.prologue->scene_floats : -1);
    const ChildrenWorkspace w = carve_children_call(pl, c);
    if (r.family == kChildrenFused) return launch_fused_children(g, head, c, w, r.fused_mode, r.own_image);
    c.image = !r.pair_image ? nullptr : c.image ? c.image : w.image;
    float* rows = (float*)w.region;
    int rc = RGL_OK, head_done = 0;
    switch (r.family) {
        case kChildrenRefused: return r.refusal;
        case kChildrenRank1: rc = launch_rank1_children(g, c, rows); break;
        case kChildrenDeep: rc = launch_deep_children(g, c, rows, r.f16, head, &head_done); break;      // (may run stage 2 and the tail itself)
        case kChildrenTile: rc = launch_tile_children(g, c, rows); break;
        case kChildrenScene: return launch_scene_children(pl, c, w.region, w.region_bytes);
        case kChildrenTilesForward: {
            bool taken = false;
            rc = launch_tiles_forward(g, head, nullptr, c.child_robot, c.humans_next, c.P * c.A, c.A, c.H, nullptr, c.child_value, nullptr,
                                      w.region, w.region_bytes, c.stream, &taken);
            return (rc || taken) ? rc : RGL_ERR_BAD_MODE;
        }
        default:
            return launch_generic_forward(g, head, nullptr, c.child_robot, c.humans_next, c.P * c.A, c.A, c.H, nullptr, nullptr,
                                          c.child_value, nullptr, c.stream);
    }
    if (rc || head_done) return rc;
    return launch_head_children(g, head, c, rows);      // stage 2
}

}  // namespace rgl

extern "C" int rgl_plan_value_children(const MprlPlanner* planner, int P, int H, int workspace_at_hand, int image_at_hand,
                                       RglValueChildrenPlan* plan) {
    if (!planner || !plan) return RGL_ERR_NULL;
    if (P < 1 || H < 1) return RGL_ERR_BAD_SHAPE;
    const rgl::ChildrenRoute r = rgl::route_value_children(planner, P, H, workspace_at_hand ? ~(size_t)0 : 0, image_at_hand != 0);
    *plan = RglValueChildrenPlan{r.family, r.refusal, r.fused_mode, r.own_image, r.f16, r.pair_image};
    return RGL_OK;
}

// A stand-alone call of P parents with a workspace of mprl_value_children_workspace_bytes: whether its route (route_value_children, the
// function launch_value_children itself follows) ends at the two-stage pair, and then the forms its two launchers give it.
extern "C" int rgl_plan_two_stage_children(const MprlPlanner* planner, int P, int H, int image_at_hand, RglTwoStageChildrenPlan* plan) {
    if (!planner || !plan) return RGL_ERR_NULL;
    if (P < 1 || H < 1) return RGL_ERR_BAD_SHAPE;
    *plan = RglTwoStageChildrenPlan{};
    const rgl::ChildrenRoute r = rgl::route_value_children(planner, P, H, ~(size_t)0, image_at_hand != 0);
    if (r.family != rgl::kChildrenRank1) return RGL_OK;
    rgl::Rank1Form s1;
    rgl::HeadForm s2;
    if (!rgl::rank1_children_form(&planner->value_graph, P, planner->num_actions, H, r.pair_image, &s1) ||
        !rgl::head_children_form(&planner->value_head, P * planner->num_actions, &s2))
        return RGL_OK;      // (the route asked both questions: not reached)
    plan->pair = 1;
    plan->hr = s1.hr;
    plan->node_tiles = s1.node_tiles;
    plan->child_tiles = s1.child_tiles;
    plan->sld = s1.sld;
    plan->norm = s1.norm;
    plan->skip = planner->value_graph.skip_connection != 0;
    plan->image = s1.image;
    plan->grid = s1.grid;
    plan->parents_per_wg = s1.parents_per_wg;
    plan->head_variant = s2.variant;
    plan->head_grid = s2.grid;
    plan->head_tiles = s2.tiles;
    plan->head_tiles_per_wave = s2.tiles_per_wave;
    plan->lds_bytes = s1.lds_bytes;
    plan->head_lds_bytes = s2.lds_bytes;
    return RGL_OK;
}
