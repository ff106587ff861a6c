// Shared helpers of the librgl_hip translation units (host + device).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "rgl_hip.h"
#include "rgl_search_args.h"
#include "rgl_switches.h"

#define RGL_HIP_TRY(expr)                          \
    do {                                           \
        hipError_t e__ = (expr);                   \
        if (e__ != hipSuccess) return (int)e__;    \
    } while (0)

#define RGL_LAUNCH_CHECK()                         \
    do {                                           \
        hipError_t e__ = hipGetLastError();        \
        if (e__ != hipSuccess) return (int)e__;    \
    } while (0)

namespace rgl {

constexpr int kCuCount = 256;      // MI355X
constexpr int kLdsBytesPerCu = 160 * 1024;
// workgroups of `lds_bytes` each that a CU's LDS holds, `most` at the most (what the kernel's waves or registers allow)
inline int workgroups_per_cu_by_lds(size_t lds_bytes, int most) {
    const int fit = (int)((size_t)kLdsBytesPerCu / lds_bytes);
    return fit < most ? fit : most;
}

// A launch with dynamic LDS: above the size every kernel may ask for, the kernel's attribute is raised first.  Returns what
// hipGetLastError() says (hipSuccess is RGL_OK).
constexpr size_t kLdsBytesWithoutAttribute = 64 * 1024;
template <class K, class... A>
int launch_lds(K kern, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const A&... args) {
    if (lds_bytes > kLdsBytesWithoutAttribute)
        RGL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(kern, grid, block, lds_bytes, st, args...);
    return (int)hipGetLastError();
}

inline int validate_mlp(const RglMlp& m, int want_in, int want_out) {
    if (m.n_layers < 1 || m.n_layers > RGL_MAX_MLP_LAYERS) return RGL_ERR_BAD_SHAPE;
    for (int l = 0; l <= m.n_layers; ++l)
        if (m.dims[l] < 1 || m.dims[l] > RGL_MAX_WIDTH) return RGL_ERR_BAD_SHAPE;
    for (int l = 0; l < m.n_layers; ++l)
        if (!m.weight[l] || !m.bias[l]) return RGL_ERR_NULL;
    if (want_in > 0 && m.dims[0] != want_in) return RGL_ERR_BAD_SHAPE;
    if (want_out > 0 && m.dims[m.n_layers] != want_out) return RGL_ERR_BAD_SHAPE;
    return RGL_OK;
}

inline int validate_graph(const RglGraph& g, int H) {
    if (H < 1 || H + 1 > RGL_MAX_NODES) return RGL_ERR_BAD_SHAPE;
    if (g.x_dim < 1 || g.x_dim > RGL_MAX_XDIM) return RGL_ERR_BAD_SHAPE;
    if (g.num_layer < 0 || g.num_layer > RGL_MAX_GCN_LAYERS) return RGL_ERR_BAD_SHAPE;
    if (g.similarity < RGL_SIM_EMBEDDED_GAUSSIAN || g.similarity > RGL_SIM_DIAGONAL) return RGL_ERR_BAD_MODE;
    int rc = validate_mlp(g.w_r, 0, g.x_dim);
    if (rc) return rc;
    rc = validate_mlp(g.w_h, 0, g.x_dim);
    if (rc) return rc;
    if (g.similarity == RGL_SIM_EMBEDDED_GAUSSIAN && !g.w_a) return RGL_ERR_NULL;
    if (g.similarity == RGL_SIM_CONCATENATION) {
        rc = validate_mlp(g.w_a_mlp, 2 * g.x_dim, 1);
        if (rc) return rc;
        if (g.w_a_mlp.n_layers != 2) return RGL_ERR_BAD_SHAPE;   // 2X -> hidden -> 1, as the reference builds it
    }
    for (int l = 0; l < g.num_layer; ++l)
        if (!g.Ws[l]) return RGL_ERR_NULL;
    return RGL_OK;
}

// ---- internal launchers (one translation unit each) ------------------------------------------------------------------------------
// The result rule, for every launcher below: an `int` is RGL_OK, a negative RGL_ERR_* or a hipError_t -- never "not mine".  Whether a
// kernel takes a call is a host-only question of its own, asked BEFORE the launcher is called: a `bool ..._covers(..)` (a few integer
// operations: ask, then call), or -- where the plan is the larger part of the host work (the tile pipeline) -- a `bool* taken` that
// the launcher sets; it has launched nothing when it says false.  A launcher called although the answer was no returns
// RGL_ERR_BAD_MODE.
int validate_forward_call(const RglGraph* graph, const RglMlp* value_head, const RglMlp* motion_head, const float* robot,
                          const float* humans, int n_scenes, int scenes_per_crowd, int H, const float* value_out,
                          const float* humans_next);                                                                // rgl_generic.hip
// module forwards (values and / or next humans of S scenes) through the one-wave-per-scene MFMA kernel; 0 bytes = the kernel does
// not cover the configuration.  scene_forward_covers: it does, and this workspace holds its rows
size_t scene_forward_workspace_bytes(const RglGraph* g, const RglMlp* value_head, const RglMlp* motion_head, int S, int crowds_per,
                                     int H);                                                                        // rgl_scene.hip
bool scene_forward_covers(const RglGraph* g, const RglMlp* value_head, const RglMlp* motion_head, int S, int crowds_per, int H,
                          size_t workspace_bytes);      // (0: no workspace)                                        // rgl_scene.hip
int launch_scene_forward(const RglGraph* g, const RglMlp* value_head, const RglMlp* motion_head, const float* robot,
                         const float* humans, int S, int crowds_per, int H, float* value_out, float* humans_next, void* workspace,
                         size_t workspace_bytes, hipStream_t stream, const float* value_rows_image = nullptr);      // rgl_scene.hip
// `value_rows_image`: the three-piece bf16 image of the graph's matrices (scene_image_bytes_for / pack_scene_image_for with no motion
// head): the value forward's weight products then run as six bf16 MFMA terms where the scene kernel offers them
int launch_generic_forward(const RglGraph* graph, const RglMlp* value_head, const RglMlp* motion_head,
                           const float* robot, const float* humans, int n_scenes, int scenes_per_crowd, int H,
                           float* H_out, float* A_out, float* value_out, float* humans_next, hipStream_t stream);   // rgl_generic.hip
// ---- value of the sibling children: one ChildrenCall (rgl_search_args.h) from launch_value_children to the kernel it chooses ------
// `c.image` (the two-stage pair and the stage-2 head): null, or the packed weight image of these weights (FusedLds layout,
// pack_images_kernel) -- the kernels then copy their weight images instead of building them from the raw matrices
// `rows_out`: the stage-1 rows [P A][64], at the start of the workspace's shared region (carve_children below)
int launch_rank1_children(const RglGraph* g, const ChildrenCall& c, float* rows_out);                               // rgl_rank1.hip
int launch_deep_children(const RglGraph* g, const ChildrenCall& c, float* rows_out, int f16, const RglMlp* head,
                         int* head_done);                                                                           // rgl_deep.hip
int launch_tile_children(const RglGraph* g, const ChildrenCall& c, float* rows_out);                                // rgl_tile.hip
// their questions (host only, their own plans' answers), asked by route_value_children alone
bool rank1_children_covers(const RglGraph* g, int P, int A, int H);                                                 // rgl_rank1.hip
bool deep_children_covers(const RglGraph* g, int P, int A, int H, bool f16);                                        // rgl_deep.hip
bool tile_children_covers(const RglGraph* g, int P, int A, int H);                                                  // rgl_tile.hip
// the forms the two-stage pair gives a call (host only; rgl_plan_two_stage_children): each field from the function its launcher calls
struct Rank1Form { int hr, node_tiles, child_tiles, sld, norm, image, grid, parents_per_wg; size_t lds_bytes; };
bool rank1_children_form(const RglGraph* g, int P, int A, int H, bool image_at_hand, Rank1Form* out);             // rgl_rank1.hip
struct HeadForm { int variant, grid, tiles, tiles_per_wave; size_t lds_bytes; };
bool head_children_form(const RglMlp* head, int M, HeadForm* out);      // a stand-alone call's stage 2 (no tail)   // rgl_head.hip
// the fused kernel's form of `mode` itself (no second form is tried); prologue_scene_floats >= 0: and its level-prologue form, with
// a scene region of that many LDS floats
bool fused_children_covers(const RglGraph* g, const RglMlp* head, int P, int A, int H, FusedImageMode mode,
                           int prologue_scene_floats = -1);                                                         // rgl_fused.hip
// stage 2, rows [M][64] -> value; for the rows of a call's P * A children (launch_head_children) the head kernel's workgroups own
// whole parents and run the call's tail for them (*tail_done = 1 / 2 as for the fused children kernel; the generic-dims head has none)
int launch_head_rows(const RglGraph* g, const RglMlp* head, const float* rows, int M, float* value, hipStream_t stream);   // rgl_head.hip
int launch_head_children(const RglGraph* g, const RglMlp* head, const ChildrenCall& c, const float* rows);         // rgl_head.hip
// The children workspace (mprl_value_children_workspace_bytes), carved in ONE place: over a null base the same walk is its size.
//   image   the weight image slot of the fused kernel and the two-stage pair: the first kImageBytes (rgl_fused.h) when H + 1 <= 32,
//           absent (null) otherwise.  Its place depends on neither P nor the size the caller passed: a search packs it once for its
//           widest level and every level's call, at any smaller P, finds it there; an own_image call packs into the same slot.
//   region  one region behind it that its users share, one at a time: the stage-1 rows [P A][64], the fused kernel's partial-tile rows,
//           the state predictor's embeddings, the scene-children rows, the tile pipeline's forward.  As long as the largest of their
//           own carves; each user is handed (region, region_bytes), none the raw workspace.
struct ChildrenWorkspace {
    float* image;
    void* region;
    size_t region_bytes;
    size_t bytes;
};
ChildrenWorkspace carve_children(void* base, const MprlPlanner* pl, int P, int H);                                  // rgl_fused.hip
// the same for a call's own workspace: all null / 0 when the call has none or a shorter one (no user gets any of it)
inline ChildrenWorkspace carve_children_call(const MprlPlanner* pl, const ChildrenCall& c) {
    const ChildrenWorkspace w = carve_children(c.workspace, pl, c.P, c.H);
    return c.workspace && c.workspace_bytes >= w.bytes ? w : ChildrenWorkspace{};
}
// the fused tile kernel (rgl_fused_kernel.hip; its planner and this driver: rgl_fused.hip).  Its weight image is prepared in global memory by pack_images_kernel: by the caller once per
// parameter state (c.image = MprlPlanner::children_image), else once per tree search (c.image_ready = 1 on the per-level calls)
// or by the call itself, in the image slot of its workspace `w`.
// kModeBx: the six-term bf16 products (RGL_CONTRACT_BF16X6): the image then holds three-piece bf16 fragments for that kernel only
// own_image: the call packs the image of `mode` itself whatever c.image / c.image_ready offer (ChildrenRoute::own_image)
int launch_fused_children(const RglGraph* g, const RglMlp* head, const ChildrenCall& c, const ChildrenWorkspace& w, FusedImageMode mode,
                          bool own_image);                                                                          // rgl_fused.hip
// P = the largest launch; asked first: fused_children_covers(.., mode).  `image`: ChildrenWorkspace::image
int pack_children_images(const RglGraph* g, const RglMlp* head, int P, int A, int H, float* image, hipStream_t stream,
                         FusedImageMode mode);                                                                      // rgl_fused_image.hip
// The ladder of the kernels above, as ONE host function: what a call of these sizes will do.  Launches nothing, reads no device
// data.  prologue_scene_floats >= 0: the call carries a LevelPrologue with a scene region of that many LDS floats
// workspace_bytes: 0 = none; only ever compared against carve_children's sizes
ChildrenRoute route_value_children(const MprlPlanner* pl, int P, int H, size_t workspace_bytes, bool image_at_hand,
                                   int prologue_scene_floats = -1);                                                 // rgl_fast.hip
int launch_value_children(const MprlPlanner* pl, ChildrenCall c);                                                  // rgl_fast.hip
// `level`: the parents and crowds, and their independent next-state / reward work; when the MFMA scene kernel runs, it executes that
// work on extra workgroups of the same launch and sets *children_done.
// `sp_image`: the three-piece bf16 weight image of the scene kernel (scene_image_bytes, pack_scene_image) when the planner's mode is
// RGL_CONTRACT_BF16X6; without one the f32 form of the kernel runs
// `workspace`: a region of predict_humans_workspace_bytes (inside a search: ChildrenWorkspace::region)
int launch_predict_humans(const MprlPlanner* pl, const ChildrenArgs& level, float* humans_next, void* workspace,
                          size_t workspace_bytes, hipStream_t stream, int* children_done, const float* sp_image);   // rgl_scene.hip
size_t predict_humans_workspace_bytes(int P, int crowds_per, int H);                                                // rgl_scene.hip
// the level prologue of the fused children kernel (RGL_LEVEL_PROLOGUE) for the parents, crowds and reward work of `children`;
// false = the state predictor is outside the prologue's form (host only: nothing is launched either way)
bool level_prologue_args(const MprlPlanner* pl, const ChildrenArgs& children, float* humans_next, const float* sp_image,
                         LevelPrologue* out);                                                                       // rgl_scene.hip
// its form check and LDS layout alone (host only, no array): the scene region's floats, the crowds a chunk's row buffer holds
bool level_prologue_layout(const MprlPlanner* pl, int crowds_per, int P, int H, int* scene_floats, int* chunk_crowds);   // rgl_scene.hip
int fused_prologue_region_floats();      // LDS floats the prologue's scene region may take in the fused children kernel   // rgl_fused.hip
// true: launch_value_children takes a LevelPrologue of `scene_floats` LDS floats for these P parents (the bf16x6 fused kernel of
// 17..20-node crowds with a softmax similarity, and a workspace it can run in)
bool fused_prologue_fits(const MprlPlanner* pl, int P, int H, size_t workspace_bytes, int scene_floats);           // rgl_fused.hip
size_t scene_image_bytes(const MprlPlanner* pl);                      // 0: no six-term bf16 scene kernel for this planner
int pack_scene_image(const MprlPlanner* pl, float* image, hipStream_t stream);
size_t scene_image_bytes_for(const RglGraph& g, const RglMlp* motion_head);          // the same for a graph (+ optional motion head)
int pack_scene_image_for(const RglGraph& g, const RglMlp* motion_head, float* image, hipStream_t stream);

int launch_scene_children(const MprlPlanner* pl, const ChildrenCall& c, void* region, size_t region_bytes);       // rgl_scene.hip
bool scene_children_covers(const MprlPlanner* pl, int H);      // ... given a stage-2 head and a region of scene_children_workspace_bytes
size_t scene_children_workspace_bytes(int P, int A, int H);                                                        // rgl_scene.hip

// the backward pass of large batches as MFMA tile kernels; *taken = false (RGL_OK, nothing launched): outside its envelope, below
// its batch threshold, or the workspace cannot hold its intermediates -- RGL_ERR_BAD_MODE instead with RGL_BACKWARD_MFMA=2 (tests)
int launch_backward_mfma(const RglGraph* graph, const RglMlp* value_head, const RglMlp* motion_head, const float* robot,
                         const float* humans, int n_scenes, int H, int detach_graph, const float* d_value,
                         const float* d_humans_next, const float* d_H, float* grad_out, void* workspace, size_t workspace_bytes,
                         hipStream_t stream, int only_choice, bool* taken);                                        // rgl_tile_pipeline.hip

// forward of models outside the shipped shapes (other embedding MLPs, x_dim = 64) on the tile kernels of rgl_tile_pipeline.hip instead
// of the general VALU kernel: embedded_gaussian / gaussian, one adjacency, 1-3 layers, N <= 64.  0 bytes = not covered; *taken =
// false (RGL_OK, nothing launched) = not covered, switched off (RGL_TILES_FORWARD=0) or the workspace is short.  tiles_forward_covers:
// the same answer without a launch (for heads whose outputs are wanted: null otherwise)
size_t tiles_forward_workspace_bytes(const RglGraph* g, const RglMlp* value_head, const RglMlp* motion_head, int S, int crowds_per,
                                     int H, int want_H);
int launch_tiles_forward(const RglGraph* g, const RglMlp* value_head, const RglMlp* motion_head, const float* robot,
                         const float* humans, int S, int crowds_per, int H, float* H_out, float* value_out, float* humans_next,
                         void* workspace, size_t workspace_bytes, hipStream_t stream, bool* taken);                  // rgl_tile_pipeline.hip
bool tiles_forward_covers(const RglGraph* g, const RglMlp* value_head, const RglMlp* motion_head, int S, int crowds_per, int H,
                          bool want_H, size_t workspace_bytes);      // (0: no workspace)                            // rgl_tile_pipeline.hip

#ifdef RGL_PHASE_TIMING
// what a unit's rgl_debug_read_*_phase_cycles export does: its 16 counters (HIP_SYMBOL(g_phase_cycles)) out, zeroed on request
inline int read_phase_cycles(const void* symbol, unsigned long long* out16, int reset) {
    const unsigned long long z[16] = {0};
    RGL_HIP_TRY(hipDeviceSynchronize());
    RGL_HIP_TRY(hipMemcpyFromSymbol(out16, symbol, sizeof(z)));
    if (reset) RGL_HIP_TRY(hipMemcpyToSymbol(symbol, z, sizeof(z)));
    return 0;
}
#endif

inline int mlp_max_hidden(const RglMlp& m) {
    int w = 0;
    for (int l = 1; l < m.n_layers; ++l) w = m.dims[l] > w ? m.dims[l] : w;
    return w;
}

}  // namespace rgl

namespace {

// Workspaces are cut into 256-byte-aligned buffers.  A Carver walks one: take<T>(bytes) is the next buffer, `off` what has been
// taken so far.  Over a null base it only measures, so a workspace's size query and its pointers are one routine.
inline long long align_up256(long long x) { return (x + 255) & ~255ll; }

struct Carver {
    char* base;
    long long off;
    template <class T>
    T* take(long long bytes) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += align_up256(bytes);
        return p;
    }
};

// One operation, rounded on its own.  The search's bookkeeping, the rewards and path G's features follow the reference's chains of
// scalar / tensor operations -- a product and the sum that takes it are two roundings -- and tests/search_bookkeeping.py and
// tests/path_g_steps.py replay them bit for bit.  The toolchain's __fmul_rn / __fadd_rn are the plain operators, which the default
// -ffp-contract fuses into one fma (one rounding: a last-bit difference in a value, and a clearance of exactly 0 -- no collision --
// turned negative); an operation compiled under `contract(off)` takes no part in a fusion.
__device__ __forceinline__ float f32_mul(float x, float y) {
#pragma clang fp contract(off)
    return x * y;
}
__device__ __forceinline__ float f32_add(float x, float y) {
#pragma clang fp contract(off)
    return x + y;
}
__device__ __forceinline__ float f32_sub(float x, float y) {
#pragma clang fp contract(off)
    return x - y;
}
__device__ __forceinline__ float f32_div(float x, float y) {
#pragma clang fp contract(off)
    return x / y;
}
// x * y + z and a * b + c * d in float64, every product and the sum rounded
__device__ __forceinline__ double f64_mad(double x, double y, double z) {
#pragma clang fp contract(off)
    return x * y + z;
}
__device__ __forceinline__ double f64_dot2(double a, double b, double c, double d) {
#pragma clang fp contract(off)
    return a * b + c * d;
}

}  // namespace
