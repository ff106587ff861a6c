// rgl_tiles.h -- internal interface of the tile pipeline (rgl_tile_pipeline.hip): the argument blocks of its kernels and what
// the driver calls across translation units -- the MLP row kernels (rgl_rows.hip) and the persistent graph kernel (rgl_graph.hip
// and a unit per family: rgl_graph_plain.hip, rgl_graph_cos.hip, rgl_graph_lw.hip).  Included by those units only.
#pragma once
#include "rgl_common.h"

#include <cstdlib>

// The launchers of the tile pipeline answer 1 for "not this path" -- and hipErrorInvalidValue is 1 as well (a launch that asks for more LDS
// than a CU has): a runtime failure must never read as "not covered" and fall through to another kernel with the error still pending.
#undef RGL_HIP_TRY
#undef RGL_LAUNCH_CHECK
#define RGL_HIP_TRY(expr)                                                          \
    do {                                                                           \
        hipError_t e__ = (expr);                                                   \
        if (e__ != hipSuccess) return e__ == hipErrorInvalidValue ? (int)hipErrorLaunchFailure : (int)e__; \
    } while (0)
#define RGL_LAUNCH_CHECK() RGL_HIP_TRY(hipGetLastError())

namespace rgl {
namespace tiles {

// row r of a [groups][per][width] tensor embedded in a larger one: p + (r / per) * group_stride + (r % per) * row_stride
struct RowMap {
    float* p;
    int per, row_stride;
    long long group_stride;
};

constexpr int kMaxRowJobs = 2;
struct RowsJob {
    RglMlp m;
    int w_off[RGL_MAX_MLP_LAYERS], b_off[RGL_MAX_MLP_LAYERS];   // inside the job's slab (torch layout [out][in], then the bias)
    int act_off[RGL_MAX_MLP_LAYERS + 1];                        // column of layer l's input inside a row of the activation tile
    int w_lds[RGL_MAX_MLP_LAYERS], w_ld[RGL_MAX_MLP_LAYERS];    // layer l's weights in the workgroup's LDS: float offset, row stride
    int b_lds[RGL_MAX_MLP_LAYERS];
    int weight_floats;                                          // weights + biases of all layers
    int act_ld, d_ld, n_params;
    int n_rows, n_tiles, n_waves;
    int wg_begin, n_wgs, waves_per_wg;
    int coop;                                                   // mlp_rows_kernel: one tile per WORKGROUP (n_waves counts workgroups)
    int wave_floats;                                            // LDS of one wave
    int kind;                                                   // 0: mlp_rows_kernel; 1: head_rows_kernel; 10 T0 + T2: mlp2_rows_kernel<T0, T2>
    int need_din, din_add;
    RowMap in, out, d_out, d_in;      // out: forward-only launches; d_out (null = zeros) / d_in: backward launches
    float* slabs;                     // [n_waves][n_params]
};
struct RowsArgs {
    RowsJob job[kMaxRowJobs];
    int n_jobs, backward;
};

struct GraphArgs {
    const float* Xr;             // [S][X]            embedded robot rows
    const float* Xh;             // [S / spc][H][X]   embedded human rows; the spc sibling scenes of a rollout share their crowd
    const float* dHL;            // [S][N][X]   (backward)
    float* HL;                   // [S][N][X], or [S][X] (row 0 only: hl_row0)   (forward)
    float* dXr;                  // [S][X]      (backward)
    float* dXh;                  // [S][H][X]   (backward)
    const float* w_a;            // [X][X] or null (gaussian: S = X X^T)
    const float* Ws[3];
    float* slabs;                // [workgroups][(has w_a + L) * X * X]
    int S, N, skip, spc, hl_row0;
    int norm;                    // row normalisation of the similarity block (graph_model.py:63-93): 0 softmax(S) (embedded_gaussian,
                                 // gaussian); 1 squared: S^2 / sum_row S^2 (:86-89); 2 equal_attention: 1 / N (:90-91); 3 diagonal: I (:92-93);
                                 // 4 cosine: C_ij = S_ij / (m_i m_j), m_i = |row i of S| (:70-74); 5 cosine_softmax: softmax(C) (:75-79)
    // floats between the robot rows of consecutive scenes / the human rows of consecutive crowds, in Xr / Xh and in dXr / dXh: X and
    // (N - 1) X for the compact arrays above, N X for both when a scene's rows are one [N][X] block (Xh = Xr + X)
    int xr_stride, xh_stride;
    int lw;                      // layerwise graph (graph_model.py:118-122): an adjacency per layer, A_l = softmax(S(H_l))
};

struct GraphForm { int nt, xt, family; };       // family: 0 plain (norm 0-3), 1 cosine (COS: norm 4-5), 2 layerwise (LW)
struct GraphPlan { int grid; size_t lds; int resident; };       // resident: the grid before min(S, .)

// ---- the row kernels (rgl_rows.hip) ----
void plan_rows_job(RowsJob& J, const RglMlp& m, int n_rows, int max_waves);
size_t rows_job_lds(const RowsJob& J);
void balance_narrow(RowsJob* const* jobs, int n, int max_waves);
int launch_rows(RowsArgs& all, hipStream_t st);

// ---- the graph kernel (rgl_graph.hip) ----
GraphForm graph_form(int N, int X, int norm, bool lw);
GraphPlan plan_graph(int S, int N, int X, int L, bool bwd, bool lw = false);
GraphPlan cap_graph_plan(GraphPlan p, int max_workgroups);
int launch_graph(const GraphArgs& ga, int X, int L, bool bwd, const GraphPlan& p, hipStream_t st);
// one per family of GraphForm (a translation unit each): every graph_kernel<NT, XT, L, BWD, ..> of the family, chosen by f.nt, f.xt, L, bwd
int launch_graph_plain(const GraphArgs& ga, const GraphForm& f, int L, bool bwd, size_t lds, int grid, hipStream_t st);
int launch_graph_cos(const GraphArgs& ga, const GraphForm& f, int L, bool bwd, size_t lds, int grid, hipStream_t st);
int launch_graph_lw(const GraphArgs& ga, const GraphForm& f, int L, bool bwd, size_t lds, int grid, hipStream_t st);

}  // namespace tiles
}  // namespace rgl
