// rgl_tile_pipeline.hip -- driver of the MFMA tile pipeline: (1) the training path's backward pass on LARGE batches and (2) the forward of models
// outside the shipped shapes.
//
// (1) crowd_nav/utils/trainer.py:110-161,199-250 drive forward + backward over replay batches; the reference's own batch is 100, the
// vector explorer of this build feeds thousands.  rgl_backward.hip gives every scene a 1024-thread workgroup, a VALU loop per product
// and a gradient slab of its own; its time per scene does not shrink with the batch.  Here the same gradients are computed as a
// pipeline of tile kernels, every dense product an fp32 MFMA (v_mfma_f32_16x16x4_f32: exact products, fp32 accumulation -- the
// arithmetic of the VALU kernel up to summation order):
//
//   1. mlp rows (forward only)          X = [w_r(robot); w_h(humans)]              one wave per 16-row tile
//   2. graph_kernel<.., false>          H_L = layers(softmax(X Wa X^T), X)          one workgroup per scene, activations in its LDS
//   3. mlp rows (backward)              value head on H_L[:, 0] / motion head on H_L[:, 1:]  ->  dH_L, head gradients
//   4. graph_kernel<.., true>           recomputes 2., back-propagates  ->  dX, and dWa / dW_l accumulated in REGISTERS over the
//                                       workgroup's scenes (one slab per workgroup, not per scene)
//   5. mlp rows (backward)              w_r / w_h from dX (forward recomputed inside)
//   6. reduce_ranges_kernel             slabs summed in a fixed order (fixed tile -> wave -> slab assignment: deterministic)
//
// "mlp rows" (rgl_rows.hip) is mlp2_rows_kernel<T0, T2> for the shipped narrow MLPs (in -> 64 -> out, in / out <= 32: weight gradients in
// registers) and mlp_rows_kernel for everything else (any MLP of the ABI; the value head: one workgroup per tile).  The intermediates
// X, H_L, dH_L, dX travel through HBM ([S][N][x_dim] floats each: 10 MB at 4096 scenes of 20 nodes, ~1.3 us of traffic apiece) so that
// each kernel keeps one job; everything else lives in LDS / registers.  Below RGL_BACKWARD_MFMA_MIN scenes of an eager step
// rgl_backward.hip runs.
//
// (2) launch_tiles_forward chains 1., 2. and head rows forward-only for models the shipped-shape kernels (rgl_scene.hip, rgl_fused_kernel.hip,
// ...) do not cover -- other embedding MLPs, x_dim = 64 -- instead of the general VALU kernel; sibling scenes of a rollout share
// their crowd's embedded rows.
//
// Envelope of both: embedded_gaussian, gaussian, squared, equal_attention or diagonal similarity (round 5: the three plain-weight
// normalisations), one adjacency for all layers -- or, round 6, one per layer (layerwise graphs) for the softmax and squared
// normalisations at x_dim 32 and N <= 32 --, x_dim 32 | 64, 1-3 layers, N <= 64; any embedding MLPs and heads within the ABI limits.  Outside it: *taken = false before any launch (the caller falls back to rgl_backward.hip / the general kernel).
//
// Differentiated forward: graph_model.py:99-130, value_estimator.py:11-20, state_predictor.py:28-36, gcn.py:95-128.
//
// The kernels live in units of their own: the row kernels and their planner in rgl_rows.hip, graph_kernel in rgl_graph_kernel.h
// (planned and launched by rgl_graph.hip); rgl_tiles.h is the interface between them and this driver.
#include "rgl_tiles.h"

using namespace rgl::tiles;

namespace {

// ------------------------------------------------------------------------------------------------
// slabs -> gradient vector
// ------------------------------------------------------------------------------------------------
constexpr int kMaxRanges = 8;
struct Range {
    const float* slabs;     // [count][n]; count = 0: the range is zero (detached parameters)
    int count, n, dst;
};
struct RangeArgs {
    Range r[kMaxRanges];
    int n_ranges, n_params;
};
// 256 threads = 32 parameters x 8 slab lanes: lane q sums slabs q, q + 8, .. in order (16 loads in flight), the eight partial sums
// are added in lane order -- a fixed summation tree, so the result is deterministic.
__global__ __launch_bounds__(256) void reduce_ranges_kernel(const RangeArgs a, float* __restrict__ out) {
    __shared__ float part[8][33];
    const int c = threadIdx.x & 31, q = threadIdx.x >> 5;
    const int k = blockIdx.x * 32 + c;
    float acc = 0.f;
    if (k < a.n_params) {
        int ri = 0;
        for (int i = 1; i < a.n_ranges; ++i)
            if (k >= a.r[i].dst) ri = i;
        const Range& R = a.r[ri];
        const float* src = R.slabs + (k - R.dst);
        int s = q;
        for (; s + 15 * 8 < R.count; s += 16 * 8) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = src[(size_t)(s + 8 * u) * R.n];
#pragma unroll
            for (int u = 0; u < 16; ++u) acc += v[u];
        }
        for (; s < R.count; s += 8) acc += src[(size_t)s * R.n];
    }
    part[q][c] = acc;
    __syncthreads();
    if (q == 0 && k < a.n_params) {
        float t = part[0][c];
#pragma unroll
        for (int u = 1; u < 8; ++u) t += part[u][c];
        out[k] = t;
    }
}

int mlp_params(const RglMlp& m) {
    int n = 0;
    for (int l = 0; l < m.n_layers; ++l) n += m.dims[l] * m.dims[l + 1] + m.dims[l + 1];
    return n;
}

// dst[0..n) = src[0..n), or zero (src == null); grid-stride
__global__ __launch_bounds__(256) void init_rows_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src ? src[i] : 0.f;
}

// what the tile kernels cover: embedded_gaussian / gaussian (softmax of S) and -- round 5 -- squared / equal_attention / diagonal
// (plain weights: graph_model.py:86-93) and cosine / cosine_softmax (:70-79), one adjacency for all layers, x_dim 32 or 64, 1-3
// layers, N <= 64; any embedding MLPs and heads within the ABI limits; layerwise graphs (round 6) with embedded_gaussian / gaussian
// / squared at x_dim 32, N <= 32 (and equal_attention / diagonal, whose adjacency is a constant).  The pair-MLP similarity
// (concatenation) and layerwise graphs of the cosine family stay on the per-scene kernels.
int tiles_norm(const RglGraph& g) {
    switch (g.similarity) {
        case RGL_SIM_EMBEDDED_GAUSSIAN: case RGL_SIM_GAUSSIAN: return 0;
        case RGL_SIM_SQUARED: return 1;
        case RGL_SIM_EQUAL_ATTENTION: return 2;
        case RGL_SIM_DIAGONAL: return 3;
        case RGL_SIM_COSINE: return 4;
        case RGL_SIM_COSINE_SOFTMAX: return 5;
        default: return -1;
    }
}
bool tiles_cover(const RglGraph& g, int H) {
    const int N = H + 1, L = g.num_layer;
    if ((g.x_dim != 32 && g.x_dim != 64) || L < 1 || L > 3 || N > 64 || H < 1) return false;
    // layerwise graphs (round 6): the softmax and the squared normalisations at the shipped feature width, up to 32 nodes; the
    // constant adjacencies (equal_attention, diagonal) do not depend on the layer's input at all -- the one-adjacency kernels
    if (g.layerwise_graph) {
        const int nm = tiles_norm(g);
        if (!(nm == 2 || nm == 3 || ((nm == 0 || nm == 1) && g.x_dim == 32 && N <= 32))) return false;
    }
    return tiles_norm(g) >= 0;
}

// the layerwise build (an adjacency per layer); constant adjacencies: layerwise or not is the same graph
bool tiles_layerwise(const RglGraph& g) { return g.layerwise_graph != 0 && tiles_norm(g) <= 1; }

void graph_args(GraphArgs& ga, const RglGraph& g, int S, int N, int spc) {
    ga = GraphArgs{};
    ga.w_a = g.similarity == RGL_SIM_EMBEDDED_GAUSSIAN ? g.w_a : nullptr;
    for (int l = 0; l < g.num_layer; ++l) ga.Ws[l] = g.Ws[l];
    ga.S = S; ga.N = N; ga.skip = g.skip_connection ? 1 : 0; ga.spc = spc;
    ga.norm = tiles_norm(g);
    ga.lw = tiles_layerwise(g) ? 1 : 0;
    ga.xr_stride = g.x_dim; ga.xh_stride = (N - 1) * g.x_dim;
}

// The forward's workspace, one Carver walk (null base: its size): robot rows [S][X] | human rows [crowds][H][X] (sibling scenes share
// their crowd's rows) | H_L -- all rows [S][N][X] for the motion head, the robot rows [S][X] for the value head alone; none when the
// caller's H_out doubles as H_L
struct TilesForwardRows { float *Xr, *Xh, *HL; size_t bytes; };
TilesForwardRows carve_tiles_forward(void* base, long long S, long long crowds, int H, int X, bool has_m, bool want_H) {
    Carver c{(char*)base, 0};
    TilesForwardRows w;
    w.Xr = c.take<float>(S * X * sizeof(float));
    w.Xh = c.take<float>(crowds * H * X * sizeof(float));
    w.HL = want_H ? nullptr : c.take<float>((has_m ? S * (H + 1) * X : S * X) * sizeof(float));
    w.bytes = (size_t)c.off;
    return w;
}

}  // namespace

extern "C" int rgl_plan_graph_tiles(const RglGraph* graph, int n_scenes, int H, int backward, int max_workgroups,
                                    RglGraphTilesPlan* plan) {
    if (!graph || !plan) return RGL_ERR_NULL;
    if (n_scenes < 1 || H < 1 || max_workgroups < 1) return RGL_ERR_BAD_SHAPE;
    *plan = RglGraphTilesPlan{};
    const RglGraph& g = *graph;
    if (!tiles_cover(g, H)) return RGL_OK;
    const bool lw = tiles_layerwise(g);
    const GraphPlan p = cap_graph_plan(plan_graph(n_scenes, H + 1, g.x_dim, g.num_layer, backward != 0, lw), max_workgroups);
    if (p.grid < 1) return RGL_OK;              // a scene does not fit the LDS of a CU: the pipeline does not take it
    const GraphForm f = graph_form(H + 1, g.x_dim, tiles_norm(g), lw);
    plan->covered = 1; plan->node_tiles = f.nt; plan->feature_tiles = f.xt; plan->layers = g.num_layer;
    plan->family = f.family; plan->norm = tiles_norm(g); plan->grid = p.grid; plan->resident = p.resident;
    plan->lds_bytes = p.lds;
    return RGL_OK;
}

namespace rgl {

// ------------------------------------------------------------------------------------------------
// forward on the same tile kernels: models the shipped-shape MFMA kernels (rgl_scene.hip, rgl_fused_kernel.hip, ..) do not cover -- other
// embedding MLPs (wr_dims / wh_dims), x_dim = 64 -- instead of the general VALU kernel.  0 bytes / *taken = false: not covered.
//   1. mlp rows (forward): robot rows [S][X], human rows [S / spc][H][X] (sibling scenes share their crowd's rows)
//   2. graph_kernel<.., false>: H_L -- all rows (motion head, H_out) or the robot row only (value head)
//   3. mlp rows (forward): value head on row 0 -> value_out, motion head on rows 1.. -> humans_next
// ------------------------------------------------------------------------------------------------
size_t tiles_forward_workspace_bytes(const RglGraph* g, const RglMlp* vh, const RglMlp* mh, int S, int spc, int H, int want_H) {
    if (!g || !tiles_cover(*g, H) || S < 1 || spc < 1 || S % spc) return 0;
    return carve_tiles_forward(nullptr, S, S / spc, H, g->x_dim, mh && mh->n_layers > 0, want_H != 0).bytes;
}

}  // namespace rgl

namespace {

// The forward's plan: whether the pipeline takes the call (ok) and, if so, its graph launch and row jobs.  vh / mh: the heads whose
// outputs are wanted (null otherwise); workspace_bytes: 0 = no workspace
struct TilesForwardPlan {
    bool ok;
    GraphPlan gp;
    RowsJob j_wr, j_wh, j_v, j_m;
};

TilesForwardPlan plan_tiles_forward(const RglGraph* graph, const RglMlp* vh, const RglMlp* mh, int S, int spc, int H, bool want_H,
                                    size_t workspace_bytes) {
    TilesForwardPlan p;
    p.ok = false;
    const bool has_v = vh && vh->n_layers > 0, has_m = mh && mh->n_layers > 0;
    if (!graph || !workspace_bytes || !tiles_cover(*graph, H) || S < 1 || spc < 1 || S % spc) return p;
    if (tiles_forward_mode() == 0) return p;          // measurements: the general kernel instead
    if (workspace_bytes < rgl::tiles_forward_workspace_bytes(graph, vh, mh, S, spc, H, want_H)) return p;
    const RglGraph& g = *graph;
    p.gp = plan_graph(S, H + 1, g.x_dim, g.num_layer, false, tiles_layerwise(g));
    if (p.gp.grid < 1) return p;
    plan_rows_job(p.j_wr, g.w_r, S, 2048);
    plan_rows_job(p.j_wh, g.w_h, S / spc * H, 2048);
    if (has_v) plan_rows_job(p.j_v, *vh, S, 2048);
    if (has_m) plan_rows_job(p.j_m, *mh, S * H, 2048);
    {
        RowsJob* emb[2] = {&p.j_wr, &p.j_wh};
        RowsJob* heads[2] = {has_v ? &p.j_v : nullptr, has_m ? &p.j_m : nullptr};
        balance_narrow(emb, 2, 2048);
        balance_narrow(heads, 2, 2048);
    }
    for (const RowsJob* J : {&p.j_wr, &p.j_wh, has_v ? &p.j_v : nullptr, has_m ? &p.j_m : nullptr})
        if (J && J->waves_per_wg < 1) return p;
    p.ok = true;
    return p;
}

}  // namespace

namespace rgl {

bool tiles_forward_covers(const RglGraph* g, const RglMlp* vh, const RglMlp* mh, int S, int spc, int H, bool want_H,
                          size_t workspace_bytes) {
    return plan_tiles_forward(g, vh, mh, S, spc, H, want_H, workspace_bytes).ok;
}

int launch_tiles_forward(const RglGraph* graph, const RglMlp* vh, const RglMlp* mh, const float* robot, const float* humans, int S,
                         int spc, int H, float* H_out, float* value_out, float* humans_next, void* workspace, size_t workspace_bytes,
                         hipStream_t st, bool* taken) {
    const bool has_v = vh && vh->n_layers > 0 && value_out, has_m = mh && mh->n_layers > 0 && humans_next;
    TilesForwardPlan tp = plan_tiles_forward(graph, has_v ? vh : nullptr, has_m ? mh : nullptr, S, spc, H, H_out != nullptr,
                                             workspace ? workspace_bytes : 0);
    *taken = tp.ok;
    if (!tp.ok) return RGL_OK;
    const RglGraph& g = *graph;
    const int N = H + 1, L = g.num_layer, X = g.x_dim, crowds = S / spc;
    const GraphPlan& gp = tp.gp;
    RowsJob &j_wr = tp.j_wr, &j_wh = tp.j_wh, &j_v = tp.j_v, &j_m = tp.j_m;
    const TilesForwardRows ws = carve_tiles_forward(workspace, S, crowds, H, X, has_m, H_out != nullptr);
    float *Xr = ws.Xr, *Xh = ws.Xh;
    const bool row0 = !has_m && !H_out;
    float* HL = H_out ? H_out : ws.HL;
    j_wr.in = RowMap{(float*)robot, 1, 0, (long long)g.w_r.dims[0]};
    j_wr.out = RowMap{Xr, 1, 0, (long long)X};
    j_wh.in = RowMap{(float*)humans, H, g.w_h.dims[0], (long long)H * g.w_h.dims[0]};
    j_wh.out = RowMap{Xh, H, X, (long long)H * X};
    {
        RowsArgs ra{};
        ra.job[0] = j_wr; ra.job[1] = j_wh; ra.n_jobs = 2; ra.backward = 0;
        const int rc = launch_rows(ra, st);
        if (rc) return rc;
    }
    GraphArgs ga;
    graph_args(ga, g, S, N, spc);
    ga.Xr = Xr; ga.Xh = Xh; ga.HL = HL; ga.hl_row0 = row0 ? 1 : 0;
    int rc = launch_graph(ga, X, L, false, gp, st);
    if (rc) return rc;
    if (has_v || has_m) {
        const long long hs = row0 ? X : (long long)N * X;
        RowsArgs ra{};
        ra.backward = 0;
        if (has_v) {
            j_v.in = RowMap{HL, 1, 0, hs};
            j_v.out = RowMap{value_out, 1, 0, 1};
            ra.job[ra.n_jobs++] = j_v;
        }
        if (has_m) {
            const int od = mh->dims[mh->n_layers];
            j_m.in = RowMap{HL + X, H, X, (long long)N * X};
            j_m.out = RowMap{humans_next, H, od, (long long)H * od};
            ra.job[ra.n_jobs++] = j_m;
        }
        rc = launch_rows(ra, st);
        if (rc) return rc;
    }
    return RGL_OK;
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// *taken = false, nothing launched: not this path (outside the envelope, below the batch threshold, or the caller's workspace
// cannot hold the intermediates): the per-scene VALU kernel of rgl_backward.hip runs.  Every such answer comes before the first
// launch.  Slab order of grad_out as documented in rgl_hip.h.
static int backward_tiles(const RglGraph* graph, const RglMlp* vh, const RglMlp* mh, const float* robot, const float* humans,
                         int S, int H, int detach_graph, const float* d_value, const float* d_humans_next, const float* d_H,
                         float* grad_out, void* workspace, size_t workspace_bytes, hipStream_t st, int only_choice, bool* taken) {
    *taken = false;
    // RGL_BACKWARD_MFMA = 0: never, 1: whenever the structure allows; default: by batch size, and whenever the per-scene kernel cannot
    // hold a scene in LDS (only_choice)
    const int mode = backward_mfma_mode();
    if (mode == 0) return RGL_OK;
    if (mode < 1 && !only_choice && S < backward_mfma_min()) {
        // Below the threshold the pipeline's device time is still the shorter one (84 vs 94 us at 100 scenes of 6 nodes, 95 vs 125 us
        // at 20 nodes), but it is seven launches instead of two and an eager training step is bound by the host.  While the stream
        // is being captured into a hipGraph only the device time counts.
        // (never asked of the legacy NULL stream: querying it while another stream captures would invalidate that capture)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (!st || hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusActive) return RGL_OK;
    }
    const RglGraph& g = *graph;
    if (!tiles_cover(g, H)) return RGL_OK;
    const int N = H + 1, L = g.num_layer, X = g.x_dim;
    const bool has_v = vh && vh->n_layers > 0, has_m = mh && mh->n_layers > 0;
    const bool embedded = g.similarity == RGL_SIM_EMBEDDED_GAUSSIAN, lw = tiles_layerwise(g);
    const GraphPlan gpf = plan_graph(S, N, X, L, false, lw), gp_full = plan_graph(S, N, X, L, true, lw);
    if (gp_full.grid < 1 || gpf.grid < 1) return RGL_OK;

    // gradient vector: w_r | w_h | w_a | Ws | value head | motion head
    const int n_wr = mlp_params(g.w_r), n_wh = mlp_params(g.w_h), n_graph = ((embedded ? 1 : 0) + L) * X * X;
    const int n_v = has_v ? mlp_params(*vh) : 0, n_m = has_m ? mlp_params(*mh) : 0;
    const int o_wr = 0, o_wh = n_wr, o_graph = o_wh + n_wh, o_v = o_graph + n_graph, o_m = o_v + n_v, n_params = o_m + n_m;

    // workspace: X | H_L | dH_L, each [S][N][X] | slabs of the row jobs and of the graph kernel.  dX replaces dH_L in place (a scene's
    // upstream rows are in the workgroup's LDS long before its dX rows are written, and no other workgroup touches them)
    Carver ws{(char*)workspace, 0};
    const size_t feat = (size_t)S * N * X;
    float* Xs = ws.take<float>(feat * sizeof(float));
    float* HL = ws.take<float>(feat * sizeof(float));
    float* dHL = ws.take<float>(feat * sizeof(float));
    float* dXs = dHL;
    // one slab per wave: fewer waves per row job (more tiles each) when the caller's workspace -- sized for the per-scene kernel's
    // slabs, n_scenes x n_params floats -- is short (few scenes of many nodes)
    RowsJob j_wr, j_wh, j_v, j_m;
    float* g_slabs = nullptr;
    const long long off_feat = ws.off;
    GraphPlan gp = gp_full;
    for (int max_waves = 2048; max_waves >= 1; max_waves >>= 1) {
        ws.off = off_feat;
        gp = cap_graph_plan(gp_full, max_waves);
        plan_rows_job(j_wr, g.w_r, S, max_waves);
        plan_rows_job(j_wh, g.w_h, S * H, max_waves);
        if (has_v) plan_rows_job(j_v, *vh, S, max_waves);
        if (has_m) plan_rows_job(j_m, *mh, S * H, max_waves);
        {   // the launches: (w_r, w_h) forward and backward, (value head, motion head)
            RowsJob* emb[2] = {&j_wr, &j_wh};
            RowsJob* heads[2] = {has_v ? &j_v : nullptr, has_m ? &j_m : nullptr};
            balance_narrow(emb, 2, max_waves);
            balance_narrow(heads, 2, max_waves);
        }
        auto slabs_for = [&](RowsJob& J) { J.slabs = ws.take<float>((long long)J.n_waves * J.n_params * sizeof(float)); };
        // (a detached graph's slabs are set aside all the same: the heads' waves, and with them the order in which their gradients
        // are summed, must not depend on detach_graph -- the motion head's gradients of a detached step are bit for bit those of
        // the step that is not)
        slabs_for(j_wr); slabs_for(j_wh);
        if (has_v) slabs_for(j_v);
        if (has_m) slabs_for(j_m);
        g_slabs = ws.take<float>((long long)gp.grid * n_graph * sizeof(float));
        if ((size_t)ws.off <= workspace_bytes) break;
    }
    if ((size_t)ws.off > workspace_bytes) return RGL_OK;
    for (const RowsJob* J : {&j_wr, &j_wh, has_v ? &j_v : nullptr, has_m ? &j_m : nullptr})
        if (J && J->waves_per_wg < 1) return RGL_OK;
    *taken = true;

    // 1. embeddings
    j_wr.in = RowMap{(float*)robot, 1, 0, (long long)g.w_r.dims[0]};
    j_wr.out = RowMap{Xs, 1, 0, (long long)N * X};
    j_wh.in = RowMap{(float*)humans, H, g.w_h.dims[0], (long long)H * g.w_h.dims[0]};
    j_wh.out = RowMap{Xs + X, H, X, (long long)N * X};
    {
        RowsArgs ra{};
        ra.job[0] = j_wr; ra.job[1] = j_wh; ra.n_jobs = 2; ra.backward = 0;
        const int rc = launch_rows(ra, st);
        if (rc) return rc;
    }
    // 2. graph forward
    GraphArgs ga;
    graph_args(ga, g, S, N, 1);
    ga.Xr = Xs; ga.Xh = Xs + X; ga.dHL = dHL; ga.HL = HL; ga.dXr = dXs; ga.dXh = dXs + X; ga.slabs = g_slabs;
    ga.xr_stride = ga.xh_stride = N * X;
    if (has_v || has_m) {
        const int rc = launch_graph(ga, X, L, false, gpf, st);
        if (rc) return rc;
    }
    // 3. heads: dH_L starts as the caller's d_H (or zero) and receives the heads' input gradients
    // (a kernel, not hipMemsetAsync / hipMemcpyAsync: recorded into a captured training step and replayed, the memset NODE was not
    // reliably ordered against the kernel nodes around it -- on some boxes the heads' `+=` into dH_L met garbage (NaN parameters), on
    // others the zeros arrived after it and a step lost the heads' gradient (sporadic 2e-3 deviations of the parameters; never in an
    // eager step, never with the per-scene kernel, which has no memset: tools/micro/captured_step_repeatability.py))
    {
        const size_t n4 = (feat + 3) / 4;
        const int blocks = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
        hipLaunchKernelGGL(init_rows_kernel, dim3(blocks), dim3(256), 0, st, dHL, d_H, feat);
        RGL_LAUNCH_CHECK();
    }
    if (has_v || has_m) {
        RowsArgs ra{};
        ra.backward = 1;
        if (has_v) {
            j_v.in = RowMap{HL, 1, 0, (long long)N * X};
            j_v.d_out = RowMap{(float*)d_value, 1, 0, 1};
            j_v.d_in = RowMap{dHL, 1, 0, (long long)N * X};
            j_v.need_din = detach_graph ? 0 : 1; j_v.din_add = 1;
            ra.job[ra.n_jobs++] = j_v;
        }
        if (has_m) {
            const int od = mh->dims[mh->n_layers];
            j_m.in = RowMap{HL + X, H, X, (long long)N * X};
            j_m.d_out = RowMap{(float*)d_humans_next, H, od, (long long)H * od};
            j_m.d_in = RowMap{dHL + X, H, X, (long long)N * X};
            j_m.need_din = detach_graph ? 0 : 1; j_m.din_add = 1;
            ra.job[ra.n_jobs++] = j_m;
        }
        const int rc = launch_rows(ra, st);
        if (rc) return rc;
    }
    if (!detach_graph) {
        // 4. graph backward
        int rc = launch_graph(ga, X, L, true, gp, st);
        if (rc) return rc;
        // 5. embeddings backward
        j_wr.d_out = RowMap{dXs, 1, 0, (long long)N * X};
        j_wh.d_out = RowMap{dXs + X, H, X, (long long)N * X};
        RowsArgs ra{};
        ra.job[0] = j_wr; ra.job[1] = j_wh; ra.n_jobs = 2; ra.backward = 1;
        rc = launch_rows(ra, st);
        if (rc) return rc;
    }
    // 6. slabs -> grad_out
    RangeArgs rr{};
    auto range = [&](const float* slabs, int count, int n, int dst) {
        if (n > 0) rr.r[rr.n_ranges++] = Range{slabs, count, n, dst};
    };
    range(detach_graph ? nullptr : j_wr.slabs, detach_graph ? 0 : j_wr.n_waves, n_wr, o_wr);
    range(detach_graph ? nullptr : j_wh.slabs, detach_graph ? 0 : j_wh.n_waves, n_wh, o_wh);
    range(g_slabs, detach_graph ? 0 : gp.grid, n_graph, o_graph);
    if (has_v) range(j_v.slabs, j_v.n_waves, n_v, o_v);
    if (has_m) range(j_m.slabs, j_m.n_waves, n_m, o_m);
    rr.n_params = n_params;
    hipLaunchKernelGGL(reduce_ranges_kernel, dim3((n_params + 31) / 32), dim3(256), 0, st, rr, grad_out);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}


// *taken = false: not this path, the per-scene VALU kernel of rgl_backward.hip runs -- unless RGL_BACKWARD_MFMA=2 (tests), which
// turns "not this path" into an error.
int launch_backward_mfma(const RglGraph* graph, const RglMlp* vh, const RglMlp* mh, const float* robot, const float* humans,
                         int S, int H, int detach_graph, const float* d_value, const float* d_humans_next, const float* d_H,
                         float* grad_out, void* workspace, size_t workspace_bytes, hipStream_t st, int only_choice, bool* taken) {
    const int rc = backward_tiles(graph, vh, mh, robot, humans, S, H, detach_graph, d_value, d_humans_next, d_H, grad_out, workspace,
                                  workspace_bytes, st, only_choice, taken);
    return (!rc && !*taken && backward_mfma_mode() == 2) ? RGL_ERR_BAD_MODE : rc;
}

}  // namespace rgl
