// rgl_search_args.h -- the argument types of the search path that cross translation units, as named types of namespace rgl: the
// launchers of rgl_common.h take them as themselves.  The device code that reads them (rgl_tail.h, rgl_children.h, rgl_scene_body.h)
// names them through using-declarations; kernel-local structs (FusedArgs, HeadArgs, DeepArgs, ...) embed them by value.
#pragma once
#include <hip/hip_runtime.h>

#include "rgl_hip.h"

namespace rgl {

// weight image / products of the fused children kernel (launch_fused_children, pack_children_images)
enum FusedImageMode { kModeF32 = 0, kModeBx = 2 };      // (1 was the split-f16 mode of ABI 4..7)

struct TailLevel {
    const float* reward;      // [P][A]
    const float* child_value; // [P][A]   V(child)
    int* keep;                // [P][W]
    float* backup;            // [P][W]
    int* best_slot;           // [P]
    int P;
};

struct TailArgs {
    int enabled;              // 0: the kernel has no tail work (stand-alone value_children calls)
    int level, D, A, W, clip, sparse;
    float gamma_f;
    const int* groups;        // [A] or null
    const float* child_robot; // this level [P][A][9]
    float* value1;            // this level [P][A]
    const float* reward_sel;  // null, or [P][A]: the rewards THIS level's selection uses instead of lv[level].reward (joint-state
                              // roots: upstream's root action_clip reads the tensor state, the root values the JointState)
    float* next_robot;        // next level's robot rows [P*W][9]; null at the deepest level
    TailLevel lv[8];
    int chain;                // deepest level only: the launch also runs the back-up steps of the levels above and the root step
                              // (every workgroup owns the parents of whole roots)
    int B;
    int* best_action;         // [B]
    float* best_value;        // [B]
    float* root_values;       // [B][W] or null
    int* root_kept;           // [B][W] or null
};

// LDS ints private to a wave that runs the select step (tail_select, rgl_tail.h): kept indices | V(child) | reward of a parent's actions
constexpr int kTailLdsInts = 3 * RGL_MAX_ACTIONS;

// Who owns the tail's parents: workgroups take them in blocks that are multiples of the returned unit.  At the deepest level (t.chain)
// that is the W^level parents of one root where the launch still has `min_roots` such blocks; it then walks the whole back-up chain
// and decides the roots (*chain = 1).  A level whose roots are single parents chains with unit 1.
inline int tail_ownership(const TailArgs& t, int P, int min_roots, int* chain) {
    long u = 1;
    for (int l = 0; t.chain && l < t.level && u <= P; ++l) u *= t.W;
    const bool whole_roots = t.chain && u <= P && P % u == 0 && P / u >= min_roots;
    *chain = whole_roots || (t.chain && u == 1);
    return whole_roots ? (int)u : 1;
}

struct ChildrenArgs {
    const float* robot;        // [P][9]
    const float* humans;       // [P / humans_per][H][5]
    int humans_per;
    const double* actions;     // [A][2]
    int P, H, A, kinematics;
    double dt;
    int joint;                 // 1: position differences in float64 (JointState roots), 0: rounded to fp32 first
    float* child_robot;        // [P][A][9]
    float* reward;             // [P][A]
    const double* robot64;     // null, or the float64 states robot / humans were rounded from (joint roots): the reward reads these
    const double* humans64;
    float* reward_clip;        // null, or [P][A]: the same rewards read as a TENSOR-BORN state (joint = 0 on the fp32 rows) -- what
                               // upstream's root action_clip sees of a joint-state root (model_predictive_rl.py:216-218,246-248)
    int p_base, c_base;        // `robot` / `humans` start at parent p_base / crowd c_base (0 for whole-level arrays; a workgroup that staged
                               // its own parents' rows in LDS hands in its sub-range -- no pointer is ever rebased below its buffer:
                               // a flat LDS address that leaves the aperture faults, HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION)
    float v_max;               // > 0: an upper bound of the table's speeds (MprlPlanner::action_speed_bound, ABI 8); 0: every wave derives
                               // it from the table (two dependent float64 loads + a square root + a wave reduction: ~1.5 us of latency)
};

struct SceneArgs {
    // EMB kernels (few scenes: the embedding launch would cost more than its work): raw state rows + the two embedding MLPs
    const float* robot_rows;           // [P][9]
    const float* human_rows;           // [n_crowds][H][5]
    const float *er_w1, *er_b1, *er_w2, *er_b2;      // w_r, k-major [9][64], [64], [64][32], [32]
    const float *eh_w1, *eh_b1, *eh_w2, *eh_b2;      // w_h
    int off_er, off_eh;                // LDS: fragment sets of the two MLPs (kRowMlpSetFloats each)
    int bx;                            // launch the bf16 six-term (BX) form: the WEIGHT products (Wa, W_l, motion head) as layer_mfma_b6
                                       // over a packed image of three-piece fragments (RGL_CONTRACT_BF16X6); S and A H stay f32
    int ws_stride;                     // floats between the layer matrices in the LDS image
    int image_floats;                  // BX: floats of the packed image
    int off_rows;                      // WGE (the level prologue): LDS row buffer of a chunk of parents -- [crowd][H][32] human embeddings
                                       // of the chunk's distinct crowds (at most chunk_crowds), then at off_rows + chunk_crowds H 32 its
                                       // [parent][32] robot rows.  (This int and chunk_crowds sit where the struct had padding: the
                                       // scene kernels' kernel arguments keep their size and offsets.)
    const float* image;                // BX: the weight image in this kernel's LDS layout (pack_scene_image)
    const float* xh_rows;              // [n_crowds][H][32]  human embeddings
    const float* x0_rows;              // [P][32]            robot embeddings
    int crowds_per;                    // scene s uses crowd s / crowds_per
    const float* wa;                   // [32][32]
    const float* Ws[RGL_MAX_GCN_LAYERS];
    int L, skip;
    int sim;                           // SIM_* row normalisation
    int chunk_crowds;                  // WGE: most distinct crowds of a chunk (prologue_chunk_end)
    const float *wm1, *bm1, *wm2, *bm2;   // motion head, k-major [32][64], [64], [64][5], [5]
    float* humans_next;                // [P][H][5]   (state predictor)
    float* rows_out;                   // null, or [P][64]: value mode -- rows [ (A H_{L-1})[robot] | H_{L-1}[robot] ] for robot_head_kernel
    int layerwise;                     // adjacency recomputed from H_l in every layer (graph_model.py:119-122)
    const float *wc1, *bc1, *wc2, *bc2;   // concatenation: pair MLP, k-major [64][64], [64], [64][1], [1]
    int off_wc1, off_bc1, off_wc2;
    int P, H, N;
    int off_wa, off_ws, off_wm1, off_bm1, off_wm2, off_bm2, off_wave, wave_stride;
};

// The state predictor and the reward / next-state work of a tree level, as the fused children kernel's prologue runs them for the
// parents each workgroup owns (RGL_LEVEL_PROLOGUE): filled by level_prologue_args (rgl_scene.hip).
struct LevelPrologue {
    SceneArgs scene;          // unsplit BX + EMB form: 8 slots, embeddings inside, LDS offsets from the prologue's scene base
    ChildrenArgs children;
    int scene_floats;         // LDS floats of the scene region (image, embedding sets, wave slots)
};

// One "value of the sibling children" call: what launch_value_children receives and hands on to the kernel it chooses.
// Value-initialise it and name what the call has; the rest stays null / 0.
struct ChildrenCall {
    const float* child_robot;   // [P][A][9]
    const float* humans_next;   // [P][H][5]: the A children of a parent share its crowd
    int P, A, H;
    float* child_value;         // [P][A]
    void* workspace;
    size_t workspace_bytes;
    hipStream_t stream;
    const float* image;         // null, or the packed weight image of the value estimator (MprlPlanner::children_image)
    int image_ready;            // 1: the workspace's image slot (carve_children, rgl_common.h: the same place for every P) holds that
                                // image (pack_children_images), no call packs its own
    const TailArgs* tail;       // null, or the search's select / back-up / root steps for these parents: the kernel runs them in its tail
    int* tail_done;             // and reports 1 (selection done) or 2 (deepest level: back-up steps and root decision too); 0 = not run
    const LevelPrologue* prologue;   // null, or the level's state predictor and reward / next-state pairs, run first (fused_prologue_fits)
};

// Which kernel family takes a ChildrenCall: route_value_children's answer (rgl_fast.hip), decided on the host before anything is
// launched.  The ids are RglValueChildrenPlan::family's (rgl_hip.h).
enum ChildrenFamily {
    kChildrenRefused = RGL_CHILDREN_REFUSED,      // no launch: ChildrenRoute::refusal is the call's result
    kChildrenFused = RGL_CHILDREN_FUSED,
    kChildrenRank1 = RGL_CHILDREN_RANK1,
    kChildrenDeep = RGL_CHILDREN_DEEP,
    kChildrenTile = RGL_CHILDREN_TILE,
    kChildrenScene = RGL_CHILDREN_SCENE,
    kChildrenTilesForward = RGL_CHILDREN_TILES_FORWARD,
    kChildrenGeneric = RGL_CHILDREN_GENERIC,
};

struct ChildrenRoute {
    ChildrenFamily family;
    int refusal;                 // kChildrenRefused: the RGL_ERR_* code; RGL_OK otherwise
    bool staged;                 // a stage-2 head exists and the workspace holds carve_children's bytes (the image slot and the stage-1 rows)
    FusedImageMode fused_mode;   // kChildrenFused: the form that runs ...
    bool own_image;              // ... and whether the call packs an f32 image of its own (bf16x6 wanted, its form does not fit a CU)
    bool f16;                    // kChildrenDeep: the f16-input contractions
    bool pair_image;             // the two-stage pair and its head copy their weights from the packed image at hand (none when not
                                 // staged, or in bf16x6: a three-piece bf16 image is in the fused kernel's layout only)
};

}  // namespace rgl
