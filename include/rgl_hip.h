/*
 * rgl_hip.h -- C ABI of librgl_hip.so: the MI355X (gfx950) implementation of the RGL
 * relational-graph forward pass and the model-predictive rollout that calls it.
 *
 * The upstream project is pure Python + torch; it has no FFI of its own.  Each entry point
 * below therefore replaces a *Python* interface of the reference (cited per function, paths
 * relative to the upstream repo), and INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add to call it.
 *
 * Conventions (all entry points):
 *   - every `const float*` / `float*` / `int*` / `double*` argument that is documented as
 *     "device" is a DEVICE pointer owned by the caller (e.g. a contiguous fp32 torch tensor);
 *     the library never allocates, frees or retains device memory;
 *   - descriptor structs (RglMlp, RglGraph, MprlPlanner) live in HOST memory and are read
 *     during the call only; the device pointers inside them must stay valid until the work
 *     queued on `stream` has finished;
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream); no call synchronises the device, so all of them may be captured into a hipGraph
 *     (the one exception, by purpose: mprl_tree_search_traced_f32, a measurement call);
 *   - return value: 0 on success, a positive hipError_t if the runtime reported one, or one of
 *     the negative RGL_ERR_* codes below.  No exceptions cross this boundary;
 *   - thread safety: calls on distinct streams may run concurrently; there is no hidden
 *     global state.
 *
 * Matrix layouts:
 *   - MLP layer l maps dims[l] -> dims[l+1];  weight[l] is row-major [dims[l]][dims[l+1]]
 *     ("k-major", i.e. torch `linear.weight.t().contiguous()`); rgl_transpose_f32 produces it
 *     on device from the torch (out,in) layout.  bias[l] has dims[l+1] entries.
 *   - w_a and Ws[l] are row-major [x_dim][x_dim] exactly as the reference stores them
 *     (they multiply from the right: X @ w_a, (A H) @ Ws[l]).
 *   - agent states: robot rows are 9 floats [px,py,vx,vy,radius,gx,gy,v_pref,theta], human rows
 *     5 floats [px,py,vx,vy,radius] (crowd_sim/envs/utils/state.py:27-28,51-52).
 */
#ifndef RGL_HIP_H
#define RGL_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGL_ABI_VERSION 8

#define RGL_MAX_MLP_LAYERS 6
#define RGL_MAX_GCN_LAYERS 8
#define RGL_MAX_NODES 128   /* N = humans + 1 (64 until ABI 3) */
#define RGL_MAX_XDIM 64
#define RGL_MAX_WIDTH 256   /* widest MLP layer */
#define RGL_MAX_ACTIONS 256

#define RGL_OK 0
#define RGL_ERR_BAD_SHAPE (-1)      /* N, x_dim, widths or counts outside the limits above     */
#define RGL_ERR_BAD_MODE (-2)       /* unknown similarity / kinematics / inconsistent flags    */
#define RGL_ERR_NULL (-3)           /* a required pointer is NULL                              */
#define RGL_ERR_WORKSPACE (-4)      /* workspace too small (see mprl_tree_workspace_bytes)     */
#define RGL_CONTRACT_F32 0
#define RGL_CONTRACT_F16 1
/* 2 was RGL_CONTRACT_F16X3 (ABI 4..7: 22-23 operand bits as two f16 halves); superseded by RGL_CONTRACT_BF16X6 and removed in ABI 8:
 * a planner that asks for it gets RGL_ERR_BAD_MODE */
#define RGL_CONTRACT_BF16X6 3       /* ABI 6: f32-WIDTH products on the matrix pipe: three bf16 pieces per operand, six terms */

#define RGL_ERR_LDS (-5)            /* configuration does not fit the 160 KiB LDS of one CU    */

typedef void* rgl_stream_t;         /* hipStream_t */

/* similarity functions of RGL.compute_similarity_matrix (crowd_nav/policy/graph_model.py:63-97) */
enum {
    RGL_SIM_EMBEDDED_GAUSSIAN = 0,
    RGL_SIM_GAUSSIAN = 1,
    RGL_SIM_COSINE = 2,
    RGL_SIM_COSINE_SOFTMAX = 3,
    RGL_SIM_CONCATENATION = 4,
    RGL_SIM_SQUARED = 5,
    RGL_SIM_EQUAL_ATTENTION = 6,
    RGL_SIM_DIAGONAL = 7
};

enum { RGL_HOLONOMIC = 0, RGL_UNICYCLE = 1 };

/* Sequential[Linear, ReLU, ...]  (crowd_nav/policy/helpers.py:5-13) */
typedef struct RglMlp {
    int n_layers;                              /* 0 = absent                                   */
    int last_relu;                             /* ReLU after the last layer too                */
    int dims[RGL_MAX_MLP_LAYERS + 1];
    const float* weight[RGL_MAX_MLP_LAYERS];   /* device, [dims[l]][dims[l+1]]                 */
    const float* bias[RGL_MAX_MLP_LAYERS];     /* device, [dims[l+1]]                          */
} RglMlp;

/* parameters + flags of one relational graph model
 * (RGL.__init__, crowd_nav/policy/graph_model.py:11-61; gcn.ValueNetwork.__init__, gcn.py:11-47) */
typedef struct RglGraph {
    RglMlp w_r;                 /* robot/self-state embedding, dims[0] = robot_dim (9 | 6)     */
    RglMlp w_h;                 /* human embedding, dims[0] = human_dim (5 | 7)                */
    int x_dim;
    int num_layer;
    int similarity;             /* RGL_SIM_*                                                   */
    int layerwise_graph;
    int skip_connection;
    int reserved;
    const float* w_a;           /* device [x_dim][x_dim]; embedded_gaussian only               */
    RglMlp w_a_mlp;             /* concatenation only: 2*x_dim -> hidden -> 1, last_relu       */
    const float* Ws[RGL_MAX_GCN_LAYERS];   /* device, each [x_dim][x_dim]                      */
} RglGraph;

/* ---------------------------------------------------------------------------------------------
 * rgl_graph_forward_f32 -- batched relational-graph forward with optional heads.
 * Replaces: RGL.forward (graph_model.py:99-130), ValueEstimator.forward (value_estimator.py:11-20),
 *           the graph+motion part of StatePredictor.forward (state_predictor.py:20-39) and the
 *           network part of gcn.ValueNetwork.forward (gcn.py:95-128).
 *   robot      device [n_scenes][robot_dim]
 *   humans     device [n_scenes / scenes_per_crowd][H][human_dim]; scene s reads crowd
 *              s / scenes_per_crowd (sibling scenes of a rollout share their humans)
 *   value_head NULL or the MLP applied to node 0 of the last layer  -> value_out[n_scenes]
 *   motion_head NULL or the MLP applied to every node; rows 1..H    -> humans_next[n_scenes][H][out]
 *   H_out      NULL or device [n_scenes][N][x_dim]   (last-layer node features)
 *   A_out      NULL or device [n_scenes][N][N]       (first adjacency computed)
 *   workspace  NULL or device scratch of rgl_graph_forward_workspace_bytes(...) bytes (ABI 3).  With it, and with H_out = A_out =
 *              NULL, models the one-wave-per-scene MFMA kernel covers (the shipped path-M shapes: w_r 9-64-32, w_h 5-64-32,
 *              x_dim 32, <= 4 layers, N <= 128 (concatenation: N <= 64), every similarity function, layerwise graphs) run on
 *              it; other embedding MLPs and x_dim = 64 (embedded_gaussian / gaussian, one adjacency, 1-3 layers, N <= 64) run on
 *              the MFMA tile kernels (rgl_tile_pipeline.hip); everything else, and every call without workspace, runs on the
 *              general kernel -- same numbers up to summation order.
 * Limits: N = H+1 <= RGL_MAX_NODES, x_dim <= RGL_MAX_XDIM, widths <= RGL_MAX_WIDTH.
 * ------------------------------------------------------------------------------------------- */
size_t rgl_graph_forward_workspace_bytes(const RglGraph* graph, const RglMlp* value_head, const RglMlp* motion_head,
                                         int n_scenes, int scenes_per_crowd, int H);   /* 0: no MFMA path for this call */
int rgl_graph_forward_f32(const RglGraph* graph, const RglMlp* value_head, const RglMlp* motion_head,
                          const float* robot, const float* humans,
                          int n_scenes, int scenes_per_crowd, int H,
                          float* H_out, float* A_out, float* value_out, float* humans_next,
                          void* workspace, size_t workspace_bytes, rgl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * rgl_graph_backward_f32 -- gradients of rgl_graph_forward_f32's outputs with respect to every
 * parameter, summed over the n_scenes scenes (deterministic: per-scene slabs reduced in scene order, 256 scenes to a partial sum).
 * Replaces: torch autograd through RGL.forward / ValueEstimator.forward / StatePredictor.forward /
 * gcn.ValueNetwork.forward as driven by MPRLTrainer / VNRLTrainer (crowd_nav/utils/trainer.py:110-161,
 * 199-250).  Supported: all eight similarity functions, layerwise_graph 0 | 1.  Two implementations behind this entry point:
 * a per-scene kernel (one workgroup and one gradient slab per scene; RGL_ERR_LDS when a scene's activations exceed the 160 KB
 * LDS of a CU: N = 64 with deep MLPs) and, for embedded_gaussian / gaussian with one adjacency, x_dim 32 | 64, 1-3 layers,
 * N <= 64, a pipeline of MFMA tile kernels (rgl_tile_pipeline.hip) -- taken from 256 scenes, whenever `stream` is being
 * captured into a hipGraph, and where the per-scene kernel does not fit.  Environment: RGL_BACKWARD_MFMA = 0 | 1 forces a
 * path (2: RGL_ERR_BAD_MODE instead of the per-scene kernel where the pipeline does not apply), RGL_BACKWARD_MFMA_MIN moves the
 * threshold.  Both are deterministic (fixed summation order per shape) -- but they are TWO summation orders: the same call below the
 * threshold runs the per-scene kernel eagerly and the tile pipeline while `stream` is being captured, so an eager step and its
 * captured replay agree to rounding (~4e-8 relative on the shipped shapes), not bit for bit.  Force one path with
 * RGL_BACKWARD_MFMA where bitwise equality between the two forms is wanted (the switches are read on every call).
 *   d_value [n_scenes], d_humans_next [n_scenes][H][out], d_H [n_scenes][N][x_dim]: upstream gradients of the
 *   corresponding forward outputs (device; NULL = zero).  detach_graph = 1 reproduces
 *   StatePredictor(..., detach=True): only the heads receive gradients.
 *   grad_out device [rgl_graph_param_count()]: w_r (W0,b0,W1,b1,..), w_h, w_a (embedded_gaussian: the matrix;
 *   concatenation: its pair MLP W0,b0,W1,b1), Ws[0..L-1], value head, motion head; Linear weight gradients in
 *   torch's nn.Linear layout [out][in] (ABI 3; the forward's RglMlp weights stay k-major [in][out]).
 *   workspace device, >= rgl_graph_backward_workspace_bytes().  Each scene has its own crowd here
 *   (scenes_per_crowd = 1: the training batches are independent transitions).
 * ------------------------------------------------------------------------------------------- */
int rgl_graph_param_count(const RglGraph* graph, const RglMlp* value_head, const RglMlp* motion_head);
size_t rgl_graph_backward_workspace_bytes(const RglGraph* graph, const RglMlp* value_head,
                                          const RglMlp* motion_head, int n_scenes);
int rgl_graph_backward_f32(const RglGraph* graph, const RglMlp* value_head, const RglMlp* motion_head,
                           const float* robot, const float* humans, int n_scenes, int H, int detach_graph,
                           const float* d_value, const float* d_humans_next, const float* d_H,
                           float* grad_out, void* workspace, size_t workspace_bytes, rgl_stream_t stream);

/* rgl_plan_mlp_rows (ABI 8, additive) -- which launch form the MFMA row kernels (rgl_rows.hip) take for one MLP over
 * n_rows rows: the tile pipeline runs w_r (a row per scene), w_h (a row per human), the value head (a row per scene) and the
 * motion head (a row per human) as such jobs, in the backward pass and in the forward of models outside the shipped shapes.
 * HOST ONLY: no device call, no launch; reads n_layers and dims of `mlp` (the weight pointers are not read).  max_waves: the
 * most waves (= gradient slabs) the job may use: 2048, halved by the backward while the caller's workspace is short.
 *   kind          1: head_rows_kernel (weights from L2, a workgroup per 16-row tile); 10 T0 + T2: mlp2_rows_kernel<T0, T2>
 *                 (two layers, hidden width 64, T0 / T2 16-column tiles of input / output); 0: mlp_rows_kernel
 *   coop          1: a workgroup shares one tile; 2: the same with the weights staged a layer at a time; 0: a tile per wave
 *   waves_per_wg  waves (LDS slices) per workgroup; 0: the MLP fits none of the forms (the pipeline answers "not mine")
 *   n_tiles       16-row tiles; n_waves = min(n_tiles, max_waves) waves walk them (jobs of kinds >= 10 that share a launch are
 *                 rebalanced afterwards); n_wgs workgroups
 *   direct        the process's RGL_HEAD_ROWS_DIRECT setting as the planner read it (once): 0 = kind 1 is never chosen
 *   lds_bytes     dynamic LDS the job asks for (a launch of two jobs takes the larger)
 * Errors: RGL_ERR_NULL, RGL_ERR_BAD_SHAPE (depth or a width outside the limits above, n_rows < 1, max_waves < 1). */
typedef struct RglRowsPlan {
    int kind, coop, waves_per_wg, n_waves, n_tiles, n_wgs;
    int direct, reserved;
    size_t lds_bytes;
} RglRowsPlan;
int rgl_plan_mlp_rows(const RglMlp* mlp, int n_rows, int max_waves, RglRowsPlan* plan);

/* rgl_plan_graph_tiles (ABI 8, additive) -- which instantiation of the tile pipeline's graph kernel (graph_kernel<NT, XT, L, BWD,
 * COS, LW> of rgl_graph_kernel.h) a graph of n_scenes scenes of H humans launches, and on how many workgroups.  The answer
 * comes from the functions the launcher itself calls.  HOST ONLY: no device call, no launch; reads x_dim, num_layer, similarity
 * and layerwise_graph of `graph` (no pointer of it is read).  backward: 0 the forward build, 1 the backward build (the backward
 * pipeline launches both).  max_workgroups: the cap the backward applies to its graph launch while the caller's workspace is
 * short of a slab per workgroup; 2048 = none.
 *   covered        0: outside what the tile kernels cover (the other fields are 0 then) -- concatenation, layerwise graphs of the
 *                  cosine family, layerwise softmax / squared graphs beyond x_dim 32 or 32 nodes, x_dim other than 32 | 64,
 *                  more than 3 layers, more than 64 nodes, or a scene that does not fit the LDS of a CU
 *   node_tiles     NT: 1 (N <= 16), 2 (N <= 32), 4;   feature_tiles XT: x_dim / 16;   layers L
 *   family         0 plain (norm 0-3), 1 cosine (norm 4-5), 2 layerwise (an adjacency per layer; a layerwise equal_attention or
 *                  diagonal graph is family 0: its adjacency is a constant)
 *   norm           0 softmax (embedded_gaussian, gaussian), 1 squared, 2 equal_attention, 3 diagonal, 4 cosine, 5 cosine_softmax
 *   resident       workgroups resident at once (256 CUs x 1..6); grid = min(n_scenes, resident, max_workgroups): the kernel is
 *                  persistent, workgroup b walks scenes b, b + grid, ..
 *   lds_bytes      dynamic LDS of a workgroup
 * Errors: RGL_ERR_NULL, RGL_ERR_BAD_SHAPE (n_scenes, H or max_workgroups < 1). */
typedef struct RglGraphTilesPlan {
    int covered, node_tiles, feature_tiles, layers, family, norm, grid, resident;
    size_t lds_bytes;
} RglGraphTilesPlan;
int rgl_plan_graph_tiles(const RglGraph* graph, int n_scenes, int H, int backward, int max_workgroups, RglGraphTilesPlan* plan);

/* rgl_plan_scene_backward (ABI 8, additive) -- what the per-scene kernel of rgl_graph_backward_f32 (one workgroup per scene, every
 * activation of the scene in LDS) would launch for n_scenes scenes of H humans: the answers of the functions the launch itself
 * calls.  HOST ONLY: no device call, no launch.  The descriptors are validated as the launch validates them -- widths, depths and
 * non-NULL weight pointers -- but no pointer is read.  Whether rgl_graph_backward_f32 hands a call to the tile pipeline instead is
 * rgl_plan_graph_tiles' question, not this one's.
 *   fits           1: a scene's activations fit the 160 KB LDS of a CU; 0: the per-scene kernel answers RGL_ERR_LDS
 *   lds_bytes      dynamic LDS of a workgroup (also where it does not fit)
 *   n_params       floats of a gradient slab = rgl_graph_param_count()
 *   threads        of a workgroup
 *   grid           workgroups: min(n_scenes, 4096); workgroup b walks scenes b, b + grid, ..: scenes_per_wg is the most one walks
 * Errors: RGL_ERR_NULL, RGL_ERR_BAD_SHAPE, RGL_ERR_BAD_MODE as rgl_graph_backward_f32 gives them for the descriptors; n_scenes < 1. */
typedef struct RglSceneBackwardPlan {
    int fits, n_params, threads, grid, scenes_per_wg, reserved;
    size_t lds_bytes;
} RglSceneBackwardPlan;
int rgl_plan_scene_backward(const RglGraph* graph, const RglMlp* value_head, const RglMlp* motion_head, int n_scenes, int H,
                            RglSceneBackwardPlan* plan);

/* rgl_transpose_f32 -- dst[c][r] = src[r][c]; turns a torch Linear weight (out,in) into the
 * k-major layout RglMlp wants.  Host-side convenience of this ABI (no reference counterpart). */
int rgl_transpose_f32(const float* src, float* dst, int rows, int cols, rgl_stream_t stream);

/* rgl_transpose_many_f32 (ABI 4) -- the same for a LIST of matrices in one launch per 32 jobs: a module's descriptor holds
 * half a dozen Linear weights and is rebuilt after every optimizer step (crowd_nav/utils/trainer.py:110-161 steps two Adam
 * optimizers per batch), so one launch per weight was most of a training step's launch count.  `jobs` is a HOST array. */
typedef struct RglTransposeJob {
    const float* src;           /* device [rows][cols] */
    float* dst;                 /* device [cols][rows] */
    int rows, cols;
} RglTransposeJob;
int rgl_transpose_many_f32(const RglTransposeJob* jobs, int n_jobs, rgl_stream_t stream);

/* rgl_gather_rows_f32 (ABI 7) -- dst_j[i][:] = src_j[index[i]][:] for every field j of a replay memory in one launch per 8 fields:
 * the batch a trainer draws (crowd_nav/utils/trainer.py:120 `for data in self.data_loader`; crowd_nav/utils/memory.py keeps tuples,
 * this package's ReplayMemory mirrors them as one [capacity][row_floats] device array per field).  `jobs` is a HOST array; `index`
 * device int64 [n_index], every entry in [0, src_rows) -- a row of NaN is written for an entry outside (torch's index_select traps). */
typedef struct RglGatherJob {
    const float* src;           /* device [src_rows][row_floats] */
    float* dst;                 /* device [n_index][row_floats]  */
    int row_floats, src_rows;
} RglGatherJob;
int rgl_gather_rows_f32(const RglGatherJob* jobs, int n_jobs, const long long* index, int n_index, rgl_stream_t stream);

/* rgl_mse_step_f32 (ABI 7) -- the loss end of one optimisation step (crowd_nav/utils/trainer.py:130-137,145-153:
 * `loss = self.criterion(outputs, target_values)` with nn.MSELoss(), `loss.backward()`, `v_losses += loss.data.item()`):
 *   target_i  = target[i], or (target == NULL: the value update, :128-129) reward[i] + gamma * next_value[i] in two roundings
 *   grad[i]   = (float)(2 / n) * (out[i] - target_i)          -- d loss / d out, exactly torch's mse_backward arithmetic
 *   *loss_sum += (double)(float)(sum_i (out[i] - target_i)^2 / n)   -- float64 accumulation of the float32 loss upstream reports
 * all device pointers, n floats each (loss_sum: one double, read-modify-written: calls on one stream are ordered).
 * workspace: device, RGL_MSE_WORKSPACE_BYTES, ZEROED ONCE by the caller and then left to this function (partial sums and an arrival
 * counter that every launch leaves at zero); only touched when n > 8192 (several workgroups), may be NULL below that.  The partial
 * sums are added in a fixed order: the reported loss does not depend on scheduling. */
#define RGL_MSE_WORKSPACE_BYTES 2048
int rgl_mse_step_f32(const float* out, const float* target, const float* reward, const float* next_value, float gamma, int n,
                     float* grad, double* loss_sum, void* workspace, rgl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * gcn_rotate_f32 -- pairwise relation features: (R,14) [robot 9 | human 5] -> (R,13)
 * agent-centric rows [dg, v_pref, theta, radius, vx, vy, px1, py1, vx1, vy1, radius1, da,
 * radius_sum].  Replaces CADRL.rotate (crowd_nav/policy/cadrl.py:241-276).
 * ------------------------------------------------------------------------------------------- */
int gcn_rotate_f32(const float* joint14, float* rotated13, int n_rows, int kinematics,
                   rgl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * gcn_predict_f32 -- path G one-step lookahead for B scenes x A actions, fused on device:
 * propagate robot (action) and humans (constant velocity), compute_reward, rotate, ValueNetwork,
 * value = reward + gamma^(dt*v_pref) * V, first-max argmax.
 * Replaces the search loop of MultiHumanRL.predict (crowd_nav/policy/multi_human_rl.py:36-64),
 * compute_reward (:73-96) and CADRL.propagate (cadrl.py:113-138).
 *   robot  device [B][9], humans device [B][H][5], actions device [A][2] (float64; (vx,vy) or (v,r))
 *   workspace device, >= gcn_predict_workspace_bytes(B, H, A) bytes
 *   action_values device [B][A] (float32), best_action device [B] (int32), best_value device [B] (float32; may be NULL;
 *   ABI 8) = action_values[b][best_action[b]] (0 where no action was selected: best_action = -1)
 * ------------------------------------------------------------------------------------------- */
typedef struct GcnPlanner {
    RglGraph graph;             /* w_r.dims[0] = 6, w_h.dims[0] = 7                             */
    RglMlp value_head;          /* gcn.ValueNetwork.value_net                                   */
    int kinematics;
    int num_actions;
    double time_step;
    double gamma;               /* raw gamma; discount is gamma^(time_step * v_pref)            */
    const double* actions;      /* device [A][2]                                                */
    /* optional (NULL = absent): the float64 states robot[B][9] / humans[B][H][5] that the fp32 arrays passed to
     * gcn_predict_f32 were rounded from.  When set, propagate / compute_reward start from them -- the reference
     * works on the simulator's python floats (cadrl.py:113-138, multi_human_rl.py:73-96) and rounds once, at to_tensor. */
    const double* root_robot_f64;
    const double* root_humans_f64;
    int contraction_dtype;      /* ABI 8: RGL_CONTRACT_F32 (0, the reference's arithmetic) | RGL_CONTRACT_BF16X6: the weight products   *
                                 * (Wa, W_l) of the graph forward as six bf16 MFMA terms over three-piece operands where the scene kernel *
                                 * offers them (softmax similarities, 17..32 nodes); everything else plain f32; other values: BAD_MODE  */
    int reserved;
} GcnPlanner;

/* The first step of gcn_predict_f32 on its own (ABI 5): for every (root b, action a) CADRL.propagate (cadrl.py:113-138) of the
 * robot, constant-velocity humans, CADRL.rotate (:241-276) into the pairwise relation features and compute_reward
 * (multi_human_rl.py:73-96; float64, reading planner->root_*_f64 when set).  Reads planner->actions, num_actions, kinematics,
 * time_step only.  self6 device [B*A][6], hum7 device [B*A][H][7], reward device [B*A]. */
int gcn_prepare_f32(const GcnPlanner* planner, const float* robot, const float* humans, int B, int H,
                    float* self6, float* hum7, float* reward, rgl_stream_t stream);
size_t gcn_predict_workspace_bytes(int B, int H, int A);
int gcn_predict_f32(const GcnPlanner* planner, const float* robot, const float* humans, int B, int H,
                    void* workspace, size_t workspace_bytes,
                    float* action_values, int* best_action, float* best_value, rgl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Path M: model-predictive rollout (crowd_nav/policy/model_predictive_rl.py:192-357).
 * ------------------------------------------------------------------------------------------- */
typedef struct MprlPlanner {
    RglGraph value_graph;       /* ValueEstimator.graph_model                                   */
    RglMlp value_head;          /* ValueEstimator.value_network                                 */
    RglGraph predictor_graph;   /* StatePredictor.graph_model (may alias value_graph's weights) */
    RglMlp motion_head;         /* StatePredictor.human_motion_predictor                        */
    int linear_state_predictor; /* 1: humans' = humans + v (no dt; state_predictor.py:109-118)  */
    int kinematics;
    int num_actions;
    int planning_depth;
    int planning_width;
    int do_action_clip;
    int sparse_search;
    int contraction_dtype;      /* RGL_CONTRACT_F32 (reference arithmetic) | RGL_CONTRACT_F16: f16 inputs, f32   *
                                 * accumulate for the dense products of the middle GCN layer of the children's  *
                                 * value graph (BASELINE configs[4]); RGL_ERR_BAD_MODE when the configuration   *
                                 * has no such kernel (needs embedded_gaussian, L = 3, N <= 64)                 *
                                 * | RGL_CONTRACT_BF16X6 (ABI 6): products whose operands keep all 24 significand   *
                                 * bits -- x = hi + mid + lo exactly, three bf16 pieces by round-to-nearest, f32's  *
                                 * exponent range, no scaling -- as the six terms W_lo a_hi + W_mid a_mid + W_hi    *
                                 * a_lo + W_mid a_hi + W_hi a_mid + W_hi a_hi of v_mfma_f32_16x16x32_bf16 with f32  *
                                 * accumulation; the dropped terms W_mid a_lo + W_lo a_mid + W_lo a_lo are at most   *
                                 * 2^-23 |W||a| (|mid| <= 2^-8 |x|, |lo| <= 2^-16 |x| in the worst case; ~2^-25      *
                                 * typically) -- the size of one f32 rounding of the product, and unbiased.          *
                                 * Offered by the value-of-children kernel of the shipped shape for 13 312 of the  *
                                 * 14 224 products of its three value-head matrices (what its LDS holds) *
                                 * and by the state predictor's scene kernel (softmax similarity, 17..32 nodes) for *
                                 * its weight products (Wa, W_l, motion head); everything else computes plain f32. */
    double time_step;
    double gamma_bar;           /* gamma^(time_step * v_pref), get_normalized_gamma (:104-105)  */
    const double* actions;      /* device [A][2] float64, table of build_action_space (:155-190)*/
    const int* action_groups;   /* device [A], action_group_index (sparse search); may be NULL.  Any int32 ids: the
                                 * kernel compares ids (no range to validate); a sparse search supports planning_width
                                 * <= 16, wider requests return RGL_ERR_BAD_MODE                                  */
    /* optional (NULL = absent): the float64 JointStates robot[B][9] / humans[B][H][5] that the fp32 ROOT arrays were
     * rounded from.  When set and the roots are joint states, estimate_reward of the ROOT level reads them: the reference
     * evaluates it on the simulator's python floats (model_predictive_rl.py:226,304-357) while the networks see the
     * fp32 tensors.  Deeper levels are tensor-born in the reference too. */
    const double* root_robot_f64;
    const double* root_humans_f64;
    /* optional (NULL = absent; ABI 3): device buffer of mprl_children_image_bytes() bytes holding the value-of-children
     * kernel's LDS weight image, prepared by mprl_pack_children_image_f32 from THIS planner's value_graph / value_head
     * weights.  The image depends on the weights only, so a caller that keeps them fixed over many searches (inference,
     * a captured decision graph) packs once and re-packs after a parameter update; without it every search (or
     * stand-alone mprl_value_children_f32 call) packs the image into its workspace first (~5 us). */
    const float* children_image;
    /* optional (NULL = absent; ABI 4): device buffer of mprl_predictor_image_bytes() bytes holding the state predictor's scene
     * kernel weight image in the layout of the planner's split mode --
     * three-piece bf16 fragments for RGL_CONTRACT_BF16X6 (ABI 6: the scene kernel's weight products Wa, W_l and the motion head as
     * six bf16 MFMA terms; S and A H stay f32) -- prepared by mprl_pack_predictor_image_f32 from THIS planner's predictor_graph /
     * motion_head.  NULL: a search in such a mode packs it into its workspace itself. */
    const float* predictor_image;
    /* optional (0 = absent; ABI 8): an upper bound of the action table's speeds -- max |(vx, vy)| (holonomic) or max |v| (unicycle)
     * over `actions`, any value >= the true maximum.  The reward step uses it to rule out, per parent, the humans no action can bring
     * within reach; without it every wave of that step derives it from the table (same results, ~1.5 us more latency per launch). */
    double action_speed_bound;
} MprlPlanner;

/* rgl_plan_prologue_embedding (ABI 8, additive) -- how a tree level of P parents (crowds of H humans, crowds_per sibling parents
 * per crowd) runs its embeddings when the fused children kernel's level prologue takes it: every workgroup embeds the rows of the
 * parents it owns in chunks, the human rows of a chunk's distinct crowds once per crowd and packed densely into 16-row tiles, the
 * chunk's robot rows as one tile.  The answer comes from the functions the launcher itself calls.  HOST ONLY: no launch; reads
 * the dimensions and modes of `planner` (no pointer of it is read), the process's RGL_LEVEL_PROLOGUE setting (once) and the
 * device's CU count (256 without a device).  unit: parents go to workgroups in multiples of it -- 1, or the parents per root at the
 * deepest level of a search whose back-up chain runs in the kernel's tail.
 *   prologue        0: the level keeps its three launches (the other fields are 0 then) -- outside the prologue's form (bf16x6,
 *                   17..20 nodes, softmax similarity, a graph state predictor), fewer than 4 parents per CU, or switched off.
 *                   (A traced search keeps the three launches whatever this says.)
 *   parents_per_wg  workgroup b owns parents [b k, (b + 1) k); workgroups of them
 *   chunk_parents   parents of a workgroup's first chunk: min(16, parents_per_wg, what chunk_crowds allows)
 *   chunk_crowds    most distinct crowds of a chunk (12, fewer for a predictor of 3 or 4 layers); a chunk ends before one more
 *   human_tiles, robot_tiles   16-row tiles of that first chunk when it starts on a crowd boundary
 *   row_floats      LDS floats of the row buffer, [chunk_crowds][H][32] + [16][32]
 *   chunks_per_wg   chunks a full workgroup walks
 * Errors: RGL_ERR_NULL, RGL_ERR_BAD_SHAPE (P, H, crowds_per or unit < 1, P no multiple of crowds_per). */
typedef struct RglPrologueEmbeddingPlan {
    int prologue, parents_per_wg, workgroups, chunk_parents, chunk_crowds, human_tiles, robot_tiles, row_floats, chunks_per_wg, reserved;
} RglPrologueEmbeddingPlan;
int rgl_plan_prologue_embedding(const MprlPlanner* planner, int P, int H, int crowds_per, int unit, RglPrologueEmbeddingPlan* plan);

/* rgl_plan_deep_children (ABI 8, additive) -- whether a stand-alone mprl_value_children_f32 call for P parents (crowds of H humans,
 * planner->num_actions children each, a workspace of mprl_value_children_workspace_bytes) reaches the shared-crowd deep kernel
 * (children_deep_kernel<NT, F16, SKIP, SOFT, T4> of rgl_deep.hip: three-layer graphs, and two-layer graphs beyond 32 nodes), and in
 * which form.  The answer comes from the functions the launcher itself calls, asked in the launcher's order: the fused and the
 * rank-1 kernel first, then the deep kernel's own plan.  HOST ONLY: no device call, no launch; reads the dimensions and modes of
 * `planner` (no pointer of it is read) and the process's RGL_DEEP_T4, RGL_DEEP_FUSE_HEAD, RGL_CHILDREN_TILE_KERNEL,
 * RGL_FORCE_GENERIC and RGL_FUSED_* settings (once each).  image_at_hand: the call has a packed value-estimator image
 * (MprlPlanner.children_image, or the search's own) -- what stage 2 inside the launch needs.
 *   covered            0: another kernel takes the call, or none of this kind does (the other fields are 0 then) -- two layers
 *                      and at most 32 nodes (rank-1 / fused), more than 64 nodes or 96 children, a similarity outside the five
 *                      row normalisations below, a layerwise graph, embeddings or x_dim outside the shipped shapes, tables
 *                      beyond a CU's LDS (the tile kernel answers), f16 without three layers or a softmax similarity (the call
 *                      answers RGL_ERR_BAD_MODE), RGL_CHILDREN_TILE_KERNEL=1
 *   node_tiles         NT = ceil(N / 16), N = H + 1;   child_tiles CT = ceil(A / 16): the crowd waves join the child tiles of
 *                      phases A and B when CT > 8 - NT;   table_stride TLD: row stride of the per-child tables;   layers L: 2 | 3
 *   norm               0 softmax (embedded_gaussian, gaussian), 1 squared, 2 equal_attention, 3 diagonal
 *   f16, skip, t4      the instantiation: f16-input MFMA for layer 1's dense products; skip connections; the last node tile (at
 *                      most four valid nodes) on the 4 x 4 x 1 MFMA
 *   fuse_head          1: stage 2 runs inside the launch and workgroup b owns the parents [b k, (b + 1) k), k = parents_per_wg
 *                      (a search's level may raise k to whole roots); 0: workgroup b walks parents b, b + grid, .. and
 *                      robot_head_kernel follows (parents_per_wg = 1)
 *   grid               workgroups;   workgroups_per_cu 1 | 2;   lds_bytes dynamic LDS of a workgroup
 * Errors: RGL_ERR_NULL, RGL_ERR_BAD_SHAPE (P or H < 1). */
typedef struct RglDeepChildrenPlan {
    int covered, node_tiles, child_tiles, table_stride, layers, norm, f16, skip, t4, fuse_head, parents_per_wg, grid;
    int workgroups_per_cu, reserved;
    size_t lds_bytes;
} RglDeepChildrenPlan;
int rgl_plan_deep_children(const MprlPlanner* planner, int P, int H, int image_at_hand, RglDeepChildrenPlan* plan);

/* rgl_plan_two_stage_children (ABI 8, additive) -- whether a stand-alone mprl_value_children_f32 call for P parents (crowds of H
 * humans, planner->num_actions children each, a workspace of mprl_value_children_workspace_bytes) reaches the two-stage pair --
 * stage 1 children_rank1_kernel<HR, NT, SKIP, SOFT> of rgl_rank1.hip (two layers, at most 32 nodes), stage 2 robot_head_kernel /
 * robot_head_any_kernel of rgl_head.hip -- and in which forms.  The answer comes from the functions the launchers themselves call:
 * the route of the call, stage 1's plan and grid, stage 2's variant, grid and cap.  HOST ONLY: no device call, no launch; reads the
 * dimensions and modes of `planner` (no pointer of it is read) and the process's RGL_CHILDREN_TWO_STAGE, RGL_CHILDREN_FUSED,
 * RGL_FUSED_MIN_TILES, RGL_CHILDREN_TILE_KERNEL and RGL_FORCE_GENERIC settings (once each).  image_at_hand: the call has a packed
 * value-estimator image (MprlPlanner.children_image).
 *   pair                 0: another kernel takes the call, or none (the other fields are 0 then) -- the fused kernel (the shipped head
 *                        from 1200 child tiles, bf16x6 up to 20 nodes), three layers, more than 32 nodes or 96 children, a
 *                        similarity outside the four row normalisations, a layerwise graph, a head without a stage-2 kernel
 *   hr                   HR 8 | 20 | 32: human rows a lane holds in registers (N <= 8, <= 20, <= 32);   node_tiles NT = ceil(N / 16):
 *                        the crowd waves;   child_tiles CT = ceil(A / 16): the child waves (CT + NT of the 8 waves carry a tile)
 *   sld                  row stride of the per-child (a, b) table;   norm 0 softmax (embedded_gaussian, gaussian), 1 squared,
 *                        2 equal_attention, 3 diagonal;   skip: skip connections
 *   image                1: stage 1 copies its weights from the packed image; 0: from the raw matrices (no image at hand, bf16x6)
 *   grid                 stage 1's workgroups; workgroup b walks parents b, b + grid, ..: parents_per_wg of them in the busiest
 *   lds_bytes            dynamic LDS of a stage-1 workgroup
 *   head_variant         0 robot_head_kernel<32,100,100>, 1 robot_head_kernel<150,100,100>, 2 robot_head_any_kernel
 *   head_grid, head_tiles, head_tiles_per_wave   stage 2's workgroups, the 16-row tiles of the P * A rows, the most one wave walks
 *   head_lds_bytes       dynamic LDS of a stage-2 workgroup
 * Errors: RGL_ERR_NULL, RGL_ERR_BAD_SHAPE (P or H < 1). */
typedef struct RglTwoStageChildrenPlan {
    int pair, hr, node_tiles, child_tiles, sld, norm, skip, image, grid, parents_per_wg;
    int head_variant, head_grid, head_tiles, head_tiles_per_wave;
    size_t lds_bytes, head_lds_bytes;
} RglTwoStageChildrenPlan;
int rgl_plan_two_stage_children(const MprlPlanner* planner, int P, int H, int image_at_hand, RglTwoStageChildrenPlan* plan);

/* rgl_plan_value_children (ABI 8, additive) -- which kernel family takes a stand-alone mprl_value_children_f32 call for P parents
 * (crowds of H humans, planner->num_actions children each): the one host function that decides it for the call itself, written
 * into a plain struct.  HOST ONLY: no device call, no launch; reads the dimensions and modes of `planner` (no pointer of it is
 * read) and the process's environment switches.  workspace_at_hand: the call has a workspace of
 * mprl_value_children_workspace_bytes;  image_at_hand: it has a packed value-estimator image (MprlPlanner.children_image).
 *   family        RGL_CHILDREN_*: REFUSED (the call returns `refusal` and launches nothing), FUSED (one launch, values directly),
 *                 RANK1 / DEEP / TILE (stage 1, then the stage-2 head -- inside the deep launch where it fuses the head), SCENE
 *                 (one wave per child, then the head), TILES_FORWARD (the tile pipeline), GENERIC (the general kernel)
 *   refusal       REFUSED: RGL_ERR_BAD_MODE (an unknown contraction mode, f16 without the deep kernel's three-layer form,
 *                 RGL_REQUIRE_MFMA_CHILDREN=1 where only the general kernel is left); 0 otherwise
 *   fused_mode    FUSED: 0 the f32 form, 2 the bf16x6 form;   own_image  FUSED: bf16x6 was asked for, its form does not fit a CU,
 *                 the f32 form runs on an image the call packs itself
 *   f16           DEEP: the f16-input contractions
 *   pair_image    RANK1 / DEEP / TILE and their head copy their weights from the packed image (at hand, staged, not bf16x6: that
 *                 image is in the fused kernel's layout only); with it and the shipped head the deep launch runs stage 2 itself
 * Errors: RGL_ERR_NULL, RGL_ERR_BAD_SHAPE (P or H < 1). */
#define RGL_CHILDREN_REFUSED 0
#define RGL_CHILDREN_FUSED 1
#define RGL_CHILDREN_RANK1 2
#define RGL_CHILDREN_DEEP 3
#define RGL_CHILDREN_TILE 4
#define RGL_CHILDREN_SCENE 5
#define RGL_CHILDREN_TILES_FORWARD 6
#define RGL_CHILDREN_GENERIC 7
typedef struct RglValueChildrenPlan {
    int family, refusal, fused_mode, own_image, f16, pair_image;
} RglValueChildrenPlan;
int rgl_plan_value_children(const MprlPlanner* planner, int P, int H, int workspace_at_hand, int image_at_hand,
                            RglValueChildrenPlan* plan);

/* rgl_plan_scene_forward (ABI 8, additive) -- the form in which the one-wave-per-scene MFMA forward (scene_graph_kernel<NT, SK, WAVES,
 * CH, SPLIT, EMB, BX> of rgl_scene.hip) takes n_scenes scenes of H humans, scenes_per_crowd sibling scenes per crowd: the state
 * predictor of a tree level (motion_head 1), path G's value rows, the module forwards of rgl_graph_forward_f32 and the children the
 * shared-crowd kernels do not cover (motion_head 0: value rows, a row kernel applies the head).  The answer comes from the functions
 * the launcher itself calls -- run_scene_kernels and the launch_scene* templates run with a plan in place of the launches.  HOST
 * ONLY: no device call, no launch; reads the dimensions and modes of `graph` (no pointer of it is read) and the process's
 * RGL_SCENE_SPLIT_BELOW, RGL_SCENE_EMBED_INSIDE, RGL_SCENE_CHILDREN_BELOW, RGL_SCENE_WIDE_SLOTS and RGL_FORCE_GENERIC settings (once
 * each).  Which kernel family a CALL asks first (RGL_TILES_FORWARD, the shared-crowd children kernels) is not this plan's matter.
 * image_at_hand: the call is in the bf16x6 mode with its packed three-piece image.  reward_offered: a tree level offers its reward /
 * next-state work to the launch (mprl_expand_f32 and the searches; never the other callers).
 *   covered          0: not this kernel (the other fields are 0 then) -- embeddings other than 9|6 / 5|7 -> 64 -> 32, x_dim other
 *                    than 32, more than 4 layers, more than 128 nodes, concatenation beyond 64 nodes, an unknown similarity,
 *                    RGL_FORCE_GENERIC=1
 *   node_tiles       NT: ceil(N / 16) for N = H + 1 <= 64, 8 beyond
 *   family           SK: 0 softmax (embedded_gaussian, gaussian), 1 plain weights (squared, equal_attention, diagonal), 2 cosine
 *                    (cosine, cosine_softmax), 3 concatenation
 *   waves            waves of a workgroup: 8, or 4 for the unsplit NT 3 | 4 forms
 *   split            1: the NT column tiles of a scene go to NT waves -- NT 2 | 4 (SK 0..2) below 3072 | 4096 scenes, NT 8 always
 *   embed_inside     1: the kernel embeds its own rows -- softmax family, 9-wide robot rows, NT 1 | 2 | 4, at most 512 scenes, no
 *                    reward work in the embedding launch; 0: rows from the launch that precedes (embed_launch 1)
 *   bx               1: the six-term bf16 weight products (image_at_hand, softmax family, NT 2)
 *   slots            scenes in flight per workgroup: waves, or waves / NT when split; workgroup b takes scenes slots b + k (k <
 *                    slots), then walks on by grid slots: a split workgroup whose last scenes run out recomputes the launch's
 *                    last scene in the idle slots and writes nothing from them
 *   grid, grid_cap   scene workgroups min(ceil(n_scenes / slots), grid_cap); grid_cap = 256 x (2 when two workgroups' LDS fit a
 *                    CU, else 1) x (2 for 4-wave workgroups)
 *   last_steps       k steps of A H over the last node tile that reach a valid node: ceil((N - 16 (NT - 1)) / 4), at least 0 (NT 8
 *                    up to 112 nodes); 4 for the concatenation family, whose last tile keeps the plain node order
 *   children_riding  1: the offered reward work rides on extra workgroups of THIS launch (fewer than 3072 scenes; 1100 in the
 *                    bf16x6 mode); offered and 0: it rides in the embedding launch
 *   embed_launch     1: a row_mlp2_pair_kernel launch precedes
 *   lds_bytes        dynamic LDS of a scene workgroup: the weight image (Wa, L x W_l, the motion head: 32 x 36 (1 + L) + 32 x 80 +
 *                    64 + 64 x 20 + 16 floats; bx: its bf16 fragments), for concatenation the pair MLP (64 x 80 + 64 + 64), with
 *                    the embeddings inside two sets of 3168 floats, and the node rows 16 NT x 36 floats per region slot -- 8 / NT
 *                    with the embeddings inside and NT 2 | 4, else 8 (NT 1 | 2), 4 (NT 3 | 4), 1 (NT 8)
 * Errors: RGL_ERR_NULL, RGL_ERR_BAD_SHAPE (n_scenes, scenes_per_crowd or H < 1, n_scenes no multiple of scenes_per_crowd, more than
 * RGL_MAX_NODES nodes). */
typedef struct RglSceneForwardPlan {
    int covered, node_tiles, family, waves, split, embed_inside, bx, slots, grid, grid_cap, last_steps, children_riding;
    int embed_launch, reserved;
    size_t lds_bytes;
} RglSceneForwardPlan;
int rgl_plan_scene_forward(const RglGraph* graph, int motion_head, int n_scenes, int scenes_per_crowd, int H, int image_at_hand,
                           int reward_offered, RglSceneForwardPlan* plan);

/* Bytes of the weight image above; 0 when the configuration has no image-based children kernel (the searches then ignore
 * `children_image`).  Depends on the architecture only (not on the weights, P, A or H).  Round 4: also offered for three-layer
 * graphs and crowds beyond 32 agents with the shipped embedding / head shapes (f32 layout): there the
 * image feeds the stage-2 head, which with an image at hand runs inside the stage-1 launch (children_deep_kernel) instead of in
 * a launch of its own. */
size_t mprl_children_image_bytes(const MprlPlanner* planner);
/* Builds the image from the planner's current value_graph / value_head weights on `stream` (planner->children_image is not
 * read).  RGL_ERR_BAD_MODE when mprl_children_image_bytes() is 0, RGL_ERR_WORKSPACE when `image_bytes` is too small. */
int mprl_pack_children_image_f32(const MprlPlanner* planner, float* image, size_t image_bytes, rgl_stream_t stream);
/* The same for MprlPlanner::predictor_image (ABI 4).  0 bytes: the planner's mode / predictor has no such image. */
size_t mprl_predictor_image_bytes(const MprlPlanner* planner);
int mprl_pack_predictor_image_f32(const MprlPlanner* planner, float* image, size_t image_bytes, rgl_stream_t stream);

/* One tree level for P parent states (the unit `action_clip` evaluates, :242-269):
 *   humans_next[p]      = StatePredictor humans of parent p (or the linear approximation)
 *   child_robot[p][a]   = compute_next_state(robot[p], action a)        (state_predictor.py:41-60)
 *   reward[p][a]        = estimate_reward(parent p, action a)           (:304-357)
 *   child_value[p][a]   = ValueEstimator(child_robot[p][a], humans_next[p])
 *   value1[p][a]        = reward + gamma_bar * child_value
 * parents_are_joint_states: 1 for root states that came from float64 JointStates (position
 * differences taken in float64), 0 for tensor-born states (differences rounded to float32 first,
 * as tensor_to_joint_state + numpy scalars do).
 * All outputs device; child_robot [P][A][9], the others [P][A] / [P][H][5].  `workspace` as for
 * mprl_value_children_f32 (NULL allowed: general kernel). */
int mprl_expand_f32(const MprlPlanner* planner, const float* robot, const float* humans, int P, int H,
                    int parents_are_joint_states,
                    float* humans_next, float* child_robot, float* reward, float* child_value,
                    float* value1, void* workspace, size_t workspace_bytes, rgl_stream_t stream);

/* The dominant kernel of the rollout on its own: child_value[p][a] = ValueEstimator(child_robot[p][a],
 * humans_next[p]) for the A sibling children of each of P parents (siblings share their crowd).
 * Same code path mprl_expand_f32 / mprl_tree_search_f32 use; exported so it can be timed and
 * tested in isolation.  `workspace` (device, mprl_value_children_workspace_bytes) is the MFMA kernels' scratch: first (crowds of
 * at most 31 humans) the slot of the one-launch kernel's weight image, packed there unless planner->children_image is set; then one
 * region for the rows of the partial 16-child tiles, or the [P*A][64] hand-off between the two stages of the small-launch pair.
 * The size grows with P and the slot's place does not depend on P or on workspace_bytes: one workspace sized for the largest P
 * serves calls of any smaller P.  workspace_bytes is only compared against that size; a shorter workspace counts as none.
 * Without one (NULL) the general kernel runs (value_estimator.py:11-20 applied to model_predictive_rl.py:245-250's loop). */
size_t mprl_value_children_workspace_bytes(const MprlPlanner* planner, int P, int H);
int mprl_value_children_f32(const MprlPlanner* planner, const float* child_robot, const float* humans_next,
                            int P, int H, float* child_value, void* workspace, size_t workspace_bytes,
                            rgl_stream_t stream);

/* Whole depth-D search for B root scenes: level-synchronous expansion, top-w clipping
 * (argpartition / sparse grouped variant), V_planning back-up (:271-302), first-max argmax.
 *   best_action device [B] int32, best_value device [B] float32
 *   root_values NULL or device [B][W0] float32, root_kept NULL or device [B][W0] int32, with
 *   W0 = planning_width if do_action_clip else num_actions; kept actions are ordered by
 *   descending one-step value (ties: lower action index first).
 * roots_are_joint_states = 1 (ABI 6 semantics): the roots are JointStates (predict(), :192-240).  Upstream then prices every
 * root action TWICE: action_clip is handed the float32 TENSOR of the state (:216-218 -> :246-248 -> tensor_to_joint_state,
 * crowd_sim/envs/utils/state.py:82-92: float32-born scalars, position differences rounded to float32), while the values of the
 * kept actions read the float64 JointState (:226).  The search does the same: level 0's selection uses the tensor-born rewards
 * (kept in the workspace at MprlLevelView::reward_clip_off), root_values / best_value the float64 ones (reward_off; read from
 * planner->root_*_f64 when set).  Without do_action_clip only the second exists.  roots_are_joint_states = 0: the roots are
 * tensor states themselves (V_planning's view of a state), one reward array. */
size_t mprl_tree_workspace_bytes(const MprlPlanner* planner, int B, int H);
int mprl_tree_search_f32(const MprlPlanner* planner, const float* robot, const float* humans, int B, int H,
                         int roots_are_joint_states, void* workspace, size_t workspace_bytes,
                         int* best_action, float* best_value, float* root_values, int* root_kept,
                         rgl_stream_t stream);

/* The same search with timing marks (ABI 5) -- a MEASUREMENT call, the one entry point that synchronises: the library records
 * HIP events on `stream` around the launches of every level l and, after waiting for the last one, reports (host arrays of
 * planning_depth floats, milliseconds)
 *   predictor_ms[l]  the level's state-predictor / next-state / reward launches,
 *   children_ms[l]   its value-of-children launch(es) AS THEY RUN IN THE SEARCH: with the selection -- and at the deepest level
 *                    the back-up chain and the root decision -- in the kernel's tail where the fused kernel takes the level
 *                    (the stand-alone select kernel included where it does not): what bench.py's `roofline` prices,
 *   *total_ms        (NULL allowed) first record to last record.
 * Not capturable into a hipGraph (event records, a host wait). */
int mprl_tree_search_traced_f32(const MprlPlanner* planner, const float* robot, const float* humans, int B, int H,
                                int roots_are_joint_states, void* workspace, size_t workspace_bytes,
                                int* best_action, float* best_value, float* root_values, int* root_kept,
                                rgl_stream_t stream, float* predictor_ms, float* children_ms, float* total_ms);

/* estimate_reward (model_predictive_rl.py:304-357) and compute_next_state (state_predictor.py:41-60) for every (parent,
 * action) pair on their own (ABI 5) -- the float64 reward kernel every tree level runs:
 *   child_robot device [P][A][9], reward device [P][A]; robot [P][9], humans [P][H][5] (each parent its own crowd);
 *   parents_are_joint_states as for mprl_expand_f32 (with planner->root_*_f64 set the float64 states are read).
 * Reads planner->actions, num_actions, kinematics, time_step only. */
int mprl_estimate_reward_f32(const MprlPlanner* planner, const float* robot, const float* humans, int P, int H,
                             int parents_are_joint_states, float* child_robot, float* reward, rgl_stream_t stream);

/* action_clip's selection on its own (model_predictive_rl.py:242-269; ABI 5): value1[p][a] = reward + gamma_bar * child_value
 * (each op rounded to fp32), keep[p][0..W-1] = the planning_width best actions of parent p in descending one-step value
 * (ties: lower index first; sparse_search: one action per action_groups id) -- W = num_actions and keep = 0..A-1 without
 * do_action_clip.  value1 device [P][A], keep device [P][W] int32.  A sparse search whose table has FEWER distinct group ids than
 * planning_width fills the tail of a row by repeating the last action kept (rows have a fixed width; upstream returns the shorter
 * list there: the first <number of distinct groups> entries of the row are that list). */
int mprl_action_clip_f32(const MprlPlanner* planner, const float* reward, const float* child_value, int P,
                         float* value1, int* keep, rgl_stream_t stream);

/* Where level `level` keeps its arrays inside the workspace (byte offsets), so a host can read
 * back the best trajectory (ModelPredictiveRL.traj) or any intermediate without a second pass. */
typedef struct MprlLevelView {
    long long n_parents;
    long long robot_off, humans_off;          /* parent states of this level                   */
    long long humans_next_off, child_robot_off, reward_off, child_value_off, value1_off;
    long long keep_off;                       /* int32 [P][W]                                  */
    long long backup_off;                     /* float32 [P][W] returns of the kept children   */
    long long best_slot_off;                  /* int32 [P] first-max slot among the kept       */
    long long reward_clip_off;                /* ABI 6: float32 [B][A], level 0 of a clipped search, else -1: the root rewards as
                                               * upstream's root action_clip reads them (see mprl_tree_search_f32); written by
                                               * searches with roots_are_joint_states = 1                                 */
} MprlLevelView;
int mprl_tree_level_view(const MprlPlanner* planner, int B, int H, int level, MprlLevelView* view);

/* ---------------------------------------------------------------------------------------------
 * Batched crowd simulator (next row of the scope table): B independent environments, float64 state.
 * crowd_step_f64 replaces CrowdSim.step (crowd_sim/envs/crowd_sim.py:252-368) incl. Agent.step /
 * compute_position (crowd_sim/envs/utils/agent.py:113-139) and, for human_policy LINEAR, Linear.predict
 * (crowd_sim/envs/policy/linear.py:16-22).  ORCA humans: crowd_orca_humans_f64 (below) computes their
 * actions on device, which crowd_step_f64 then applies with human_policy GIVEN.
 *   robot [B][9], humans [B][H][5], time [B], done [B] (int, in/out): updated in place when update != 0
 *   (update = 0 is the reference's onestep_lookahead: outputs only); environments with done != 0 are frozen.
 *   human_goals [B][H][2], human_vpref [B][H] (LINEAR); human_actions [B][H][2] (GIVEN); robot_action [B][2]
 *   = (vx,vy) or (v,r).  Outputs: reward [B] fp32, info [B] CROWD_INFO_*, dmin [B] (closest approach; -1 on collision).
 * crowd_observe_f32: the fp32 (robot [B][9], humans [B][H][5]) view policies consume (JointState.to_tensor,
 * crowd_sim/envs/utils/state.py:64-79).
 * ------------------------------------------------------------------------------------------- */
enum { CROWD_INFO_NOTHING = 0, CROWD_INFO_DISCOMFORT = 1, CROWD_INFO_COLLISION = 2, CROWD_INFO_REACH_GOAL = 3,
       CROWD_INFO_TIMEOUT = 4, CROWD_INFO_DONE = 5 };
enum { CROWD_HUMAN_GIVEN = 0, CROWD_HUMAN_LINEAR = 1, CROWD_HUMAN_CONSTANT_VELOCITY = 2 };

typedef struct CrowdSimConfig {
    double time_step, time_limit;
    double success_reward, collision_penalty, discomfort_dist, discomfort_penalty_factor;
    int kinematics;             /* of the robot: RGL_HOLONOMIC | RGL_UNICYCLE */
    int human_policy;           /* CROWD_HUMAN_* */
} CrowdSimConfig;

int crowd_step_f64(const CrowdSimConfig* cfg, double* robot, double* humans, const double* human_goals,
                   const double* human_vpref, const double* robot_action, const double* human_actions,
                   double* time, int* done, int B, int H, int update, float* reward, int* info, double* dmin,
                   rgl_stream_t stream);
int crowd_observe_f32(const double* robot, const double* humans, int B, int H, float* robot32, float* humans32,
                      rgl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ORCA on device (ABI 8, additive): RVO2 2.0's doStep for agents without obstacles, as Python-RVO2 runs it
 * (crowd_sim/envs/policy/orca.py:75-161).  Every agent quantity is rounded from float64 to float32 once; the
 * arithmetic is float32 with no contraction and correctly rounded division and square root, so the velocities
 * are Python-RVO2's (RVO2 finds neighbours with a kd-tree, these kernels in agent index order: the two differ only
 * on exact distance ties at the max_neighbors cut-off).  Outputs are float32 values widened to float64.
 *   Agent radii are radius + 0.01 + safety_space (added in float64, then rounded); a preferred velocity points at
 *   the agent's goal, (g - p) / |g - p| when |g - p| > 1 and g - p otherwise (float64, then rounded).
 *   done [B] may be NULL; environments with done != 0 are skipped (their output rows are not written).
 *
 * crowd_orca_humans_f64: CentralizedORCA.predict as CrowdSim.step calls it (crowd_sim/envs/crowd_sim.py:256-262):
 *   the agents are the H humans, plus the robot appended last when robot_visible (its own answer is discarded).
 *   max_speed_rule CROWD_ORCA_MAX_SPEED_ONE: every agent's max_speed is 1 (centralized planning);
 *   CROWD_ORCA_MAX_SPEED_VPREF: a human's max_speed is its v_pref (human_vpref [B][H], required): decentralized
 *   planning, where each human's own ORCA.predict depends only on its own preferred velocity and max_speed.
 *   robot [B][9], humans [B][H][5], human_goals [B][H][2]; out [B][H][2] (vx, vy).
 * crowd_orca_robot_f64: ORCA.predict for the robot (orca.py:75-125; the imitation-learning expert): agent 0 is the
 *   robot with max_speed = v_pref (robot[7]) and its preferred velocity toward its goal, the humans follow with
 *   preferred velocity (0, 0).  out [B][2].
 * Errors: RGL_ERR_NULL for a missing pointer, RGL_ERR_BAD_SHAPE for B, H < 1 or max_neighbors outside
 * [0, CROWD_ORCA_MAX_NEIGHBORS], RGL_ERR_BAD_MODE for an unknown max_speed_rule.
 * ------------------------------------------------------------------------------------------- */
#define CROWD_ORCA_MAX_NEIGHBORS 32
enum { CROWD_ORCA_MAX_SPEED_ONE = 0, CROWD_ORCA_MAX_SPEED_VPREF = 1 };

typedef struct CrowdOrcaParams {
    double time_step;           /* the simulator's (0.25); the collision case's horizon                     */
    double neighbor_dist;       /* 10 (ORCA.__init__, orca.py:58-67)                                         */
    double time_horizon;        /* 5                                                                          */
    double safety_space;        /* 0; added to every radius with the 0.01 pad                                 */
    int max_neighbors;          /* 10; at most CROWD_ORCA_MAX_NEIGHBORS                                       */
    int max_speed_rule;         /* CROWD_ORCA_MAX_SPEED_* (crowd_orca_humans_f64; ignored by the robot entry) */
    int reserved;
} CrowdOrcaParams;

int crowd_orca_humans_f64(const CrowdOrcaParams* params, const double* robot, const double* humans, const double* human_goals, const double* human_vpref, const int* done, int B, int H, int robot_visible, double* out, rgl_stream_t stream);
int crowd_orca_robot_f64(const CrowdOrcaParams* params, const double* robot, const double* humans, const int* done, int B, int H, double* out, rgl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Seeded scenes on device (ABI 8, additive): CrowdSim.reset's generate_human loop (crowd_sim/envs/crowd_sim.py:117-169,
 * 185-203) for B cases in one launch.  Case b replays np.random.RandomState(seeds[b]) -- MT19937 seeded by init_genrand,
 * random_sample() as the 53-bit double of two outputs -- bit for bit and makes the accept / reject decisions of the sequential
 * loop in float64 without contraction, so positions, radii and v_pref are the host generator's; circle_crossing positions
 * differ from it only by the device's sin / cos against the host libm's (a few ulp).
 *   seeds device [B]; robot [B][9], humans [B][H][5], goals [B][H][2], vpref [B][H] (the layout crowd_step_f64 takes)
 *   status [B]: 0, or 1 when some human was not placed within max_attempts attempts (upstream's loop has no exit): that
 *     case's other outputs are unspecified.  draws [B]: random_sample / uniform calls consumed.
 * Errors: RGL_ERR_NULL for a missing pointer, RGL_ERR_BAD_SHAPE for B, H < 1, H + 1 > RGL_MAX_NODES or max_attempts < 1,
 * RGL_ERR_BAD_MODE for an unknown scenario.
 * ------------------------------------------------------------------------------------------- */
enum { CROWD_SCENARIO_CIRCLE_CROSSING = 0, CROWD_SCENARIO_SQUARE_CROSSING = 1 };

typedef struct CrowdSceneConfig {
    double circle_radius;       /* sim.circle_radius (4): robot at (0, -R) heading for (0, R)                */
    double square_width;        /* sim.square_width (20)                                                      */
    double discomfort_dist;     /* reward.discomfort_dist (0.2): part of the clearance margin                 */
    double robot_radius, robot_v_pref;
    double human_radius, human_v_pref;   /* replaced by uniform(0.3, 0.5) / uniform(0.5, 1.5) draws when randomize_attributes */
    int scenario;               /* CROWD_SCENARIO_*                                                           */
    int randomize_attributes;
    int max_attempts;           /* per human, position and goal attempts together                             */
    int reserved;
} CrowdSceneConfig;

int crowd_generate_scenes_f64(const CrowdSceneConfig* cfg, const unsigned* seeds, int B, int H, double* robot, double* humans, double* goals, double* vpref, int* status, int* draws, rgl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Replay memory filled on device (ABI 8, additive): Explorer.update_memory (crowd_nav/utils/explorer.py:113-140) and
 * ReplayMemory.push (crowd_nav/utils/memory.py) for a whole batch of finished episodes in one call of three launches.
 *   robot [T][B][9], humans [T][B][H][5], rewards [T][B] float32, info [T][B] int32 (CROWD_INFO_*): row t is the state the
 *   policy saw at step t of the B lock-step episodes and the reward / info that step returned.  Episode b has L_b steps with
 *   info != CROWD_INFO_DONE (a prefix of its column); it is stored when its last code in COLLISION..TIMEOUT is COLLISION or
 *   REACH_GOAL and then gives the L_b - 1 tuples (state i, value i, rewards[i][b], state i + 1), numbered episode-major:
 *   j = (tuples of the stored episodes before b) + i.  No row of a step t >= L_b is read.
 *   value i = imitation_learning ? (float)togo[i], togo[t] = rewards[t] + step_discount * togo[t + 1] in float64 from
 *   t = L_b - 1 down, product and sum rounded on their own : 0.
 *   layout RGL_REPLAY_MPRL: fields = robot [capacity][9], humans [capacity][H][5], value [capacity], reward [capacity],
 *   next robot, next humans.  RGL_REPLAY_GCN: fields = state [capacity][H][13], value, reward, next state, a state being the
 *   H rows gcn_rotate_f32 makes of [robot | human h] under `kinematics` (the same bits).
 *   runs: where the tuples go.  Tuple j with first <= j < first + count is stored in slot `slot + (j - first)`; a tuple no
 *   run names is skipped.  The caller derives them from ReplayMemory.push's ring arithmetic for the N pushes of the call
 *   and trims them so that no slot is named twice (a tuple overwritten later in the same call is skipped): an append run
 *   after clear() with the write position ahead of the length, and the ring run from the write position, wrapping at most
 *   once after the trim.  The ring run that follows an append run starts at slot 0 and, if it wraps, has overwritten the
 *   append run entirely, so at most RGL_REPLAY_MAX_RUNS = 2 runs survive.  n_runs = 0: nothing is stored, nothing launched.
 *   workspace device, >= rgl_replay_push_workspace_bytes(T, B) bytes (0 for T, B < 1 or T * B > INT_MAX).
 * Errors, checked on the host before any launch: RGL_ERR_NULL; RGL_ERR_BAD_SHAPE for T, B, H < 1, H + 1 > RGL_MAX_NODES,
 * capacity < 1, T * B > INT_MAX, n_runs outside [0, RGL_REPLAY_MAX_RUNS] or a run that leaves [0, capacity);
 * RGL_ERR_BAD_MODE for an unknown layout or kinematics; RGL_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
#define RGL_REPLAY_MAX_RUNS 2
#define RGL_REPLAY_MAX_FIELDS 6
enum { RGL_REPLAY_MPRL = 0, RGL_REPLAY_GCN = 1 };

typedef struct RglReplayRun {
    long long first, slot, count;
} RglReplayRun;

typedef struct RglReplayPushJob {
    const float* robot;         /* device [T][B][9]                                                           */
    const float* humans;        /* device [T][B][H][5]                                                        */
    const float* rewards;       /* device [T][B]                                                              */
    const int* info;            /* device [T][B]                                                              */
    int T, B, H;
    int layout;                 /* RGL_REPLAY_*                                                               */
    int kinematics;             /* RGL_HOLONOMIC | RGL_UNICYCLE (RGL_REPLAY_GCN: the rotation's)              */
    int imitation_learning;
    double step_discount;       /* gamma^(time_step * v_pref)                                                 */
    long long capacity;
    float* fields[RGL_REPLAY_MAX_FIELDS];   /* device, the memory's stacked fields (4 for RGL_REPLAY_GCN)     */
    int n_runs, reserved;
    RglReplayRun runs[RGL_REPLAY_MAX_RUNS];
    void* workspace;
    size_t workspace_bytes;
    rgl_stream_t stream;
} RglReplayPushJob;

size_t rgl_replay_push_workspace_bytes(int T, int B);
int rgl_replay_push_f32(const RglReplayPushJob* job);

/* rgl_replay_push_sarl_f32 (ABI 8, additive) -- the same push with the rows SARL / OM-SARL train on.  `job` is the struct above;
 * `layout` is not read.  fields = state [capacity][H][D], value [capacity], reward [capacity], next state [capacity][H][D], a
 * state being what SARL.transform makes of (robot, humans): row h = the 13 features gcn_rotate_f32 makes of [robot | human h]
 * under `kinematics` and, with maps (channels 1..3, D = 13 + cell_num^2 channels), behind them the slots
 * sarl_occupancy_maps_f32 gives human h from the float32 human states with time_step = 0 -- the same bits in both parts.
 * channels = 0: no maps, D = 13, cell_num and cell_size are not read.  Rows are built only for states of which a tuple lands in
 * the memory; no buffer of rows exists outside the fields.  Workspace: rgl_replay_push_workspace_bytes(T, B).
 * Errors, in the order of rgl_replay_push_f32 (the map parameters stand where its layout does): RGL_ERR_NULL (`rows` too);
 * RGL_ERR_BAD_SHAPE as above; channels outside 0..3 RGL_ERR_BAD_MODE, cell_num outside 1..8 or cell_size <= 0
 * RGL_ERR_BAD_SHAPE (what sarl_occupancy_maps_f32 accepts), maps with H = 1 RGL_ERR_BAD_SHAPE (upstream's np.concatenate of no
 * other human); the kinematics, the four fields, the runs and the workspace as above.  n_runs = 0: RGL_OK, nothing launched. */
typedef struct RglReplaySarlRows { int cell_num; double cell_size; int channels; } RglReplaySarlRows;   /* channels 0: no maps, D = 13 */
int rgl_replay_push_sarl_f32(const RglReplayPushJob* job, const RglReplaySarlRows* rows);

/* ---------------------------------------------------------------------------------------------
 * Epsilon-greedy exploration on device with each case's own numpy stream (ABI 8, additive).  Upstream seeds numpy per case in
 * CrowdSim.reset (crowd_sim/envs/crowd_sim.py:185-191), generate_human consumes doubles, and every predict of the episode
 * continues that stream: `probability = np.random.random()` and, when `probability < epsilon`,
 * `np.random.choice(len(action_space))` (crowd_nav/policy/model_predictive_rl.py:208-210, multi_human_rl.py:34-36).
 *   The stream rule.  Case b has seed s and its scene consumed d doubles (crowd_generate_scenes_f64's draws[b]), so the first
 *   2 d 32-bit outputs of init_genrand(s) are spent.  Each decision of a LIVE environment (done[b] == 0):
 *     u = random_sample() = ((a >> 5) * 2^26 + (b >> 6)) / 2^53 of two outputs a, b;  explored = u < epsilon (strict, float64);
 *     explored, n = n_actions: n = 1 gives index 0 and consumes nothing; otherwise mask = the smallest 2^k - 1 >= n - 1 and one
 *     output at a time, v = output & mask, until v <= n - 1: index = v (numpy's legacy masked rejection on 32-bit draws);
 *     not explored: the policy's greedy index is kept.
 *   A finished environment (done[b] != 0) draws nothing and its state is untouched: upstream no longer calls predict for it.
 *   Upstream's reach_destination early return (no draw) is not implemented: it cannot occur for a live environment of a seeded
 *   scene (step ends an episode whose next position is within the robot's radius of the goal; start and goal are 2R apart).
 *   state device [B][CROWD_EXPLORE_STATE_WORDS]: the 624 MT19937 words, then the position of the next word (0..624; 624 = twist
 *   first).
 * crowd_explore_seed_u32: state[b] = init_genrand(seeds[b]) advanced past 2 * max(draws[b], 0) outputs: ceil(2 d / 624) twists and
 *   position 2 d - 624 (twists - 1); d = 0: the seeded words and position 624.
 * crowd_explore_select_f64: one decision for every environment.  chosen[b] = the index taken, action[b][0..1] = table[chosen[b]]
 *   (the float64 bits copied), explored[b] = 0 | 1 (nullable), state[b] advanced in place.  A finished environment gets
 *   chosen = greedy, its action row and explored = 0.  A chosen index outside [0, n_actions) -- only a greedy one can be -- gives
 *   a NaN action row, like rgl_gather_rows_f32, and chosen = greedy; a live environment still draws.
 * Both calls are asynchronous, allocate nothing and launch kernels only (safe under stream capture).
 * Errors, decided on the host before any launch: RGL_ERR_NULL for a missing required pointer; RGL_ERR_BAD_SHAPE for B < 1,
 * n_actions < 1 or n_actions > RGL_MAX_ACTIONS; RGL_ERR_BAD_MODE for an epsilon that is NaN or outside [0, 1].
 * ------------------------------------------------------------------------------------------- */
#define CROWD_EXPLORE_STATE_WORDS 625
int crowd_explore_seed_u32(const unsigned* seeds, const int* draws, int B, unsigned* state, rgl_stream_t stream);

typedef struct CrowdExploreJob {
    const int* greedy;      /* device [B]: the policy's choice                         */
    const int* done;        /* device [B]: crowd_step_f64's flags, != 0 = finished     */
    const double* table;    /* device [n_actions][2]                                   */
    unsigned* state;        /* device [B][625], advanced in place                      */
    int* chosen;            /* device [B]                                              */
    double* action;         /* device [B][2] = table[chosen]                           */
    int* explored;          /* device [B] 0 | 1; nullable                              */
    double epsilon;
    int B, n_actions;
    rgl_stream_t stream;
} CrowdExploreJob;
int crowd_explore_select_f64(const CrowdExploreJob* job);

/* ---------------------------------------------------------------------------------------------
 * Nonstop humans (ABI 8, additive): CrowdSim.step with sim.nonstop_human on (crowd_sim/envs/crowd_sim.py:96, 346-349).
 * crowd_step_nonstop_f64 is crowd_step_f64 with update = 1 -- the same robot move, closest-approach loop, reward ladder, human
 * actions and clock, from the same device functions -- and, in the same launch, upstream's regeneration of every human that
 * arrives, drawn from the environment's own numpy stream (`state`, the layout of crowd_explore_seed_u32, which the exploration
 * kernel shares: one stream, two consumers).  One wave per environment.  For a LIVE environment (done[b] == 0 on entry):
 *   1. the stream is advanced past policy_draws doubles (2 outputs each, twists included): what the robot's policy drew on the
 *      host for this decision (`predict` takes one random() in every phase; 0 when crowd_explore_select_f64 made the draw on
 *      `state` itself, or for a policy that draws nothing);
 *   2. the robot steps; then the humans in index order: human i moves by its action (decided on the state before anyone moved) and
 *      ARRIVES when sqrt(dx * dx + dy * dy) < radius_i for its new position against its goal (float64, numpy's roundings);
 *   3. an arrived human is regenerated at once (generate_human(human), crowd_sim.py:117-169): with scene.randomize_attributes
 *      v_pref = 0.5 + u, radius = 0.3 + 0.2 u' (two doubles) replace its own; then the scenario's rejection loop (circle: three
 *      doubles per attempt, goal = the mirrored position; square: one sign double, then position attempts, then goal attempts, two
 *      doubles each) with its own v_pref as the circle's noise scale.  The clearance list is [robot] + humans as upstream holds
 *      them at that moment: the robot at its NEW position; humans before i as their steps (and regenerations) left them; human i
 *      ITSELF at the position it just reached, with its old goal and its new radius; humans after i where they stood BEFORE the
 *      step.  Accepted: position, goal, zero velocity (and radius, v_pref) are written; the stream stands after the accepted
 *      attempt.  This happens on the episode's last step too.
 *   scene.max_attempts bounds the attempts of ONE regeneration (position and goal attempts of a square add up).  At the cap the
 *   human stays where its step left it (position, velocity, goal; redrawn attributes are kept), status[b] is set to 1 and the
 *   stream stands after the attempts consumed; later humans of the environment are still processed.  status is only ever SET: the
 *   caller zeroes it and may read it after many steps.
 *   A finished environment draws and moves nothing (reward 0, CROWD_INFO_DONE, dmin inf, attempts 0).
 *   attempts (nullable) [B][H]: attempts consumed by human h's regeneration in this step, 0 = it did not arrive.
 *   Of `scene` the fields circle_radius, square_width, discomfort_dist, scenario, randomize_attributes and max_attempts are read.
 * Asynchronous, allocates nothing, one launch.  Errors: RGL_ERR_NULL for a missing required pointer (human_goals, human_vpref and
 * state included); RGL_ERR_BAD_SHAPE for B < 1, H < 1, H + 1 > RGL_MAX_NODES, policy_draws < 0 or max_attempts < 1;
 * RGL_ERR_BAD_MODE for unknown kinematics, human policy or scenario.
 * ------------------------------------------------------------------------------------------- */
typedef struct CrowdNonstopJob {
    CrowdSimConfig sim;
    CrowdSceneConfig scene;
    double* robot;                  /* device [B][9], in place                                          */
    double* humans;                 /* device [B][H][5], in place                                       */
    double* human_goals;            /* device [B][H][2], in place                                       */
    double* human_vpref;            /* device [B][H], in place                                          */
    const double* robot_action;     /* device [B][2]                                                    */
    const double* human_actions;    /* device [B][H][2]; required for CROWD_HUMAN_GIVEN                 */
    double* time;                   /* device [B]                                                       */
    int* done;                      /* device [B]                                                       */
    unsigned* state;                /* device [B][CROWD_EXPLORE_STATE_WORDS], advanced in place         */
    int* status;                    /* device [B]: set to 1 where a regeneration reached the cap        */
    int* attempts;                  /* device [B][H]; nullable                                          */
    float* reward;                  /* device [B]                                                       */
    int* info;                      /* device [B]                                                       */
    double* dmin;                   /* device [B]                                                       */
    int B, H, policy_draws, reserved;
    rgl_stream_t stream;
} CrowdNonstopJob;
int crowd_step_nonstop_f64(const CrowdNonstopJob* job);

/* ---------------------------------------------------------------------------------------------
 * SARL / OM-SARL (ABI 8, additive): the one-step search of MultiHumanRL.predict (crowd_nav/policy/multi_human_rl.py:
 * 12-71) with the attention value network of crowd_nav/policy/sarl.py:28-73 and, with_om, the occupancy maps of
 * build_occupancy_maps (multi_human_rl.py:117-171).  The calls of this block evaluate; the value network's gradient is the
 * training block below (sarl_value_train_f32 / sarl_value_backward_f32).
 *
 * Supported shapes -- every other request returns RGL_ERR_BAD_SHAPE / RGL_ERR_BAD_MODE before anything is launched:
 *   mlp1 D-150-100 (last_relu), mlp2 100-100-50, attention (200 | 100)-100-100-1 (200: with_global_state), mlp3 56-150-100-100-1;
 *   D = 13 + cell_num^2 om_channel_size in {13, 29, 45, 61} (om_channel_size 0 = no maps; 1..3 with cell_num 4);
 *   2 <= H with maps (upstream's np.concatenate raises for a single human), 1 <= H without, H <= RGL_SARL_MAX_HUMANS;
 *   contraction_dtype RGL_CONTRACT_F32 only; n_scenes = B num_actions <= 2^26.
 * ------------------------------------------------------------------------------------------- */
#define RGL_SARL_MAX_HUMANS 127     /* RGL_MAX_NODES - 1, the limit of gcn_prepare_f32.  The value kernel parks a tile's per-human
                                     * mlp1 outputs (7 424 bytes per human): in LDS up to 20 humans, above that in the workspace. */

typedef struct SarlPlanner {
    RglMlp mlp1, mlp2, attention, mlp3;     /* sarl.ValueNetwork.{mlp1, mlp2, attention, mlp3}                          */
    int with_global_state;                  /* the mean of mlp1's outputs over the humans joins every attention input   */
    int om_channel_size;                    /* 0: no occupancy maps; 1 | 2 | 3                                          */
    int cell_num;
    int kinematics;
    double cell_size;
    int num_actions;
    int contraction_dtype;                  /* RGL_CONTRACT_F32                                                         */
    double time_step;
    double gamma;                           /* raw gamma; the discount is gamma^(time_step * v_pref)                    */
    const double* actions;                  /* device [A][2]                                                            */
    const double* root_robot_f64;           /* optional, as in GcnPlanner: the float64 states the fp32 arrays were      */
    const double* root_humans_f64;          /* rounded from (propagate, reward and the maps start from them)            */
} SarlPlanner;

/* Occupancy maps of B crowds: maps device [B][H][cell_num^2 om_channel_size] float32, row (b, i) = the map of human i among the
 * other humans j != i of crowd b (by index), built from the NEXT states p + v time_step (time_step = 0: the states themselves,
 * what MultiHumanRL.transform hands over).  Reads humans_f64 (device [B][H][5] float64) when set, else humans (float32, widened).
 * All arithmetic is float64 with every operation rounded on its own, as numpy's: frame rotated by arctan2(vy, vx) of human i,
 * indices floor(p / cell_size + cell_num / 2), out-of-range humans dropped; one channel: 0 / 1; two and three channels: per-slot
 * means (sum in other-human order / count) with the slot base 2 * cell in BOTH cases, so with three channels neighbouring cells
 * share a slot and the slots above 2 (cell_num^2 - 1) + 2 stay zero.  One launch.
 * Errors: RGL_ERR_NULL; RGL_ERR_BAD_MODE (om_channel_size outside 1..3); RGL_ERR_BAD_SHAPE (B < 1, H < 2, H + 1 > RGL_MAX_NODES,
 * cell_num outside 1..8, cell_size <= 0). */
int sarl_occupancy_maps_f32(const double* humans_f64, const float* humans, int B, int H, double time_step, int cell_num,
                            double cell_size, int om_channel_size, float* maps, rgl_stream_t stream);

/* The value network for n_scenes scenes of H humans in one launch (plus one that lays the weights out as MFMA fragments in
 * `workspace`, device, >= sarl_value_workspace_bytes_for(planner, n_scenes, H); 0 = outside the supported shapes).
 * sarl_value_workspace_bytes(planner) is the packed weights alone: enough for H <= 20, whose parking slots are LDS.  For
 * 21 <= H <= RGL_SARL_MAX_HUMANS the workspace also holds the parking slots, H x 7 424 bytes for each workgroup of the launch's
 * persistent grid (at most 512 workgroups), and sarl_value_f32 returns RGL_ERR_WORKSPACE when given less.  The environment switch
 * RGL_SARL_PARK=global (read per launch, like RGL_SARL_GRID_CAP) takes that form at any H, and the size functions that take H
 * then report it for small H too.  Input, either
 *   rows   device [n_scenes][H][D]: the rows sarl.ValueNetwork.forward takes (the other three pointers are not read), or
 *   self6  device [n_scenes][6], hum7 device [n_scenes][H][7] as gcn_prepare_f32 writes them, and (D > 13) maps device
 *          [n_scenes / scenes_per_root][H][D - 13]: scene s reads the maps of root s / scenes_per_root.
 * value device [n_scenes], attention device [n_scenes][H] (the softmax weights of sarl.py:57-63).  Up to 20 humans no
 * activation passes through global memory; above, the parked ones do, between waves of one workgroup.  The last, partial tile of
 * sixteen scenes is masked.  Reads the four MLPs, with_global_state, om_channel_size,
 * cell_num and contraction_dtype of `planner`. */
size_t sarl_value_workspace_bytes(const SarlPlanner* planner);
size_t sarl_value_workspace_bytes_for(const SarlPlanner* planner, int n_scenes, int H);
int sarl_value_f32(const SarlPlanner* planner, const float* rows, const float* self6, const float* hum7, const float* maps,
                   int n_scenes, int scenes_per_root, int H, void* workspace, size_t workspace_bytes, float* value,
                   float* attention, rgl_stream_t stream);

/* The search for B roots: gcn_prepare_f32, the maps (once per root and human: without query_env they do not depend on the action,
 * multi_human_rl.py:52-55), the value network over the B x A scenes, value = reward + gamma^(time_step v_pref) V in float64 (:58)
 * and the strict `>` walk of :60-64.
 *   robot device [B][9], humans device [B][H][5]; workspace device, >= sarl_predict_workspace_bytes(planner, B, H) (0: unsupported)
 *   action_values device [B][A], best_action device [B] int32 (-1 where no value beats -inf), best_value device [B] (nullable; 0
 *   where best_action = -1), best_attention device [B][H] (nullable): the attention weights of the selected action (zeros where
 *   best_action = -1) -- what get_attention_weights() returns after predict. */
size_t sarl_predict_workspace_bytes(const SarlPlanner* planner, int B, int H);
int sarl_predict_f32(const SarlPlanner* planner, const float* robot, const float* humans, int B, int H, void* workspace,
                     size_t workspace_bytes, float* action_values, int* best_action, float* best_value, float* best_attention,
                     rgl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SARL / OM-SARL training (ABI 8, additive): the value network over replay rows with its gradient with respect to the 22
 * parameter tensors.  Shapes as above (f32 only, 1 <= H <= RGL_SARL_MAX_HUMANS, 2 <= H with maps), n_scenes * H <= 2^20; anything
 * else returns RGL_ERR_BAD_SHAPE / RGL_ERR_BAD_MODE / RGL_ERR_NULL before a launch, a workspace below
 * sarl_train_workspace_bytes(planner, n_scenes, H) (0: outside the supported shapes) RGL_ERR_WORKSPACE.
 *   rows device [n_scenes][H][D] (what sarl.ValueNetwork.forward takes); there is no gradient with respect to them.
 * sarl_value_train_f32 is sarl_value_f32 on those rows: the same launches, so `value` [n_scenes] and `attention` [n_scenes][H]
 * (nullable) hold the same bits at every H -- an online network and its frozen target cannot drift apart by kernel choice.
 * sarl_value_backward_f32 recomputes the activations row-major in the workspace (about 1 700 floats per scene and human), walks the
 * pre-activation gradients from grad_value [n_scenes] down to mlp1 and writes every weight and bias gradient in one last launch.
 * The gradients are OVERWRITTEN, not accumulated.  It reads nothing sarl_value_train_f32 left behind except through `planner`, so
 * the two calls may use different workspaces of that size.  Every gradient is a sum in a fixed order (no atomics): two calls on the
 * same inputs give the same bits.  Neither call allocates, synchronises, reads device data on the host or launches on another
 * stream: both can be recorded into a hipGraph.
 * ------------------------------------------------------------------------------------------- */
#define RGL_SARL_LAYERS 11          /* mlp1.{0,2} mlp2.{0,2} attention.{0,2,4} mlp3.{0,2,4,6}, in this order */
typedef struct SarlGrads {
    float* weight[RGL_SARL_LAYERS]; /* device [out][in]: torch's nn.Linear.weight layout */
    float* bias[RGL_SARL_LAYERS];   /* device [out]                                      */
} SarlGrads;
size_t sarl_train_workspace_bytes(const SarlPlanner* planner, int n_scenes, int H);
int sarl_value_train_f32(const SarlPlanner* planner, const float* rows, int n_scenes, int H, void* workspace, size_t workspace_bytes,
                         float* value, float* attention, rgl_stream_t stream);
int sarl_value_backward_f32(const SarlPlanner* planner, const float* rows, const float* grad_value, int n_scenes, int H,
                            void* workspace, size_t workspace_bytes, const SarlGrads* grads, rgl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * LSTM-RL / OM-LSTM-RL (ABI 8, additive): the one-step search of MultiHumanRL.predict behind the distance sort of LstmRL.predict
 * (crowd_nav/policy/lstm_rl.py:94-108) with the recurrent value networks of lstm_rl.py:9-69.  Evaluation only: there is no
 * gradient call.
 *
 * Supported shapes -- every other request returns RGL_ERR_BAD_SHAPE / RGL_ERR_BAD_MODE before anything is launched:
 *   lstm_hidden_dim 50; mlp 56-150-100-100-1; with_interaction_module: mlp1 D-150-100-100-50 (no ReLU after its last layer) in
 *   front of nn.LSTM(50, 50) (ValueNetwork2), otherwise nn.LSTM(D, 50) on the rows themselves (ValueNetwork1);
 *   D = 13 + cell_num^2 om_channel_size in {13, 29, 45, 61}; 2 <= H with maps, 1 <= H without, H <= RGL_SARL_MAX_HUMANS;
 *   contraction_dtype RGL_CONTRACT_F32 only; n_scenes = B num_actions <= 2^26.
 * ------------------------------------------------------------------------------------------- */
typedef struct LstmPlanner {
    RglMlp mlp1;                            /* ValueNetwork2.mlp1; not read when with_interaction_module is 0           */
    RglMlp mlp;                             /* the head on [six self features | h_n]                                    */
    const float* weight_ih;                 /* device, torch's layout: lstm.weight_ih_l0 [200][50 | D], gate rows i f g o */
    const float* weight_hh;                 /* device, lstm.weight_hh_l0 [200][50]                                      */
    const float* bias_ih;                   /* device [200]                                                             */
    const float* bias_hh;                   /* device [200]                                                             */
    int with_interaction_module;
    int lstm_hidden_dim;                    /* 50                                                                       */
    int om_channel_size;                    /* 0: no occupancy maps; 1 | 2 | 3                                          */
    int cell_num;
    double cell_size;
    int kinematics;
    int num_actions;
    int contraction_dtype;                  /* RGL_CONTRACT_F32                                                         */
    int reserved;
    double time_step;
    double gamma;                           /* raw gamma; the discount is gamma^(time_step * v_pref)                    */
    const double* actions;                  /* device [A][2]                                                            */
} LstmPlanner;

/* The value network for n_scenes sequences of H rows in one launch (plus one that lays the weights out as MFMA fragments in
 * `workspace`, device, >= lstm_value_workspace_bytes(planner); 0 = outside the supported shapes; the size depends on neither
 * n_scenes nor H: h and c stay in registers).  The LSTM runs over the rows of a scene in row order from h = c = 0, gates
 * W_ih x + b_ih + W_hh h + b_hh in torch's order i, f, g, o; the value is the head on [row 0's first six features | h_n].  Input,
 * either
 *   rows   device [n_scenes][H][D] (the other three pointers are not read; scenes_per_root is taken as 1), or
 *   self6  device [n_scenes][6], hum7 device [n_scenes][H][7] as gcn_prepare_f32 writes them, and (D > 13) maps device
 *          [n_scenes / scenes_per_root][H][D - 13]: scene s reads the maps of root s / scenes_per_root.
 * D must be the planner's 13 + cell_num^2 om_channel_size.  lengths: null (every scene runs H steps), or device [n_scenes] int32,
 * each in 1..H -- NOT checked: scene s stops updating h and c after lengths[s] steps (pack_padded_sequence's hn).  The rows
 * behind a scene's length are read and must be addressable; their content does not reach the value.  value device [n_scenes].
 * The gate non-linearities saturate: no pre-activation produces NaN or Inf.  RGL_SARL_GRID_CAP caps the launch's grid (tests).
 * Reads the two MLPs, the four LSTM tensors, with_interaction_module, lstm_hidden_dim, om_channel_size, cell_num and
 * contraction_dtype of `planner`. */
size_t lstm_value_workspace_bytes(const LstmPlanner* planner);
int lstm_value_f32(const LstmPlanner* planner, const float* rows, const float* self6, const float* hum7, const float* maps,
                   const int* lengths, int n_scenes, int H, int D, int scenes_per_root, void* workspace, size_t workspace_bytes,
                   float* value, rgl_stream_t stream);

/* The search for B roots.  One launch sorts every root's humans by DECREASING float64 distance sqrt(dx dx + dy dy) to the robot
 * (every operation rounded on its own; from robot_f64 / humans_f64 when BOTH are given, else from the widened float32 rows), ties
 * in their given order as python's sorted(.., reverse=True) leaves them.  On the sorted humans: gcn_prepare_f32, the maps (once per
 * root), the value network over the B x A scenes, value = reward + gamma^(time_step v_pref) V in float64 and the strict `>` walk.
 *   robot device [B][9], humans device [B][H][5]; robot_f64 [B][9] / humans_f64 [B][H][5] device float64, nullable: the states the
 *   float32 arrays were rounded from; workspace device, >= lstm_predict_workspace_bytes(planner, B, H) (0: unsupported)
 *   action_values device [B][A], best_action device [B] int32 (-1 where no value beats -inf), best_value device [B] (nullable; 0
 *   where best_action = -1), order device [B][H] int32 (nullable): order[b][k] = the given index of the human at sorted place k. */
size_t lstm_predict_workspace_bytes(const LstmPlanner* planner, int B, int H);
int lstm_predict_f32(const LstmPlanner* planner, const float* robot, const float* humans, const double* robot_f64,
                     const double* humans_f64, int B, int H, void* workspace, size_t workspace_bytes, float* action_values,
                     int* best_action, float* best_value, int* order, rgl_stream_t stream);

/* The library's RGL_* environment switches ("Environment switches"), host only (added within ABI 8): the name of
 * switch i (NULL past the end), and the value the library would read for it from `text_or_null` -- the variable's text, NULL when it
 * is unset.  Nothing is read from the environment; RGL_ERR_BAD_SHAPE: no such switch. */
const char* rgl_switch_name(int i);
int rgl_switch_parse(int i, const char* text_or_null, int* value);

/* library identification: ABI version and the gfx target the device code was built for */
int rgl_abi_version(void);
const char* rgl_build_target(void);

#ifdef __cplusplus
}
#endif
#endif /* RGL_HIP_H */
