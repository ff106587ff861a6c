// rgl_sarl_backward.hip -- SARL / OM-SARL training: the gradient of the attention value network of crowd_nav/policy/sarl.py:28-73 with
// respect to its 22 parameter tensors.
//
// sarl_value_train_f32 IS sarl_value_f32 (rgl_sarl.hip) on the same rows -- the same launches, hence the same bits as the frozen
// target network computes -- and saves nothing: sarl_value_backward_f32 recomputes the activations, row-major, into the workspace.
// The forward kernel keeps a scene in an MFMA column and an activation in the lane that made it; the weight gradients contract over
// the scenes, which wants the operands the other way round, so the backward works on plain row-major matrices throughout:
//
//   recompute   Y = relu(X Wt + b) layer by layer (rows x features; Wt is the planner's k-major weight copy), the mean over the
//               humans written behind every mlp1 row (the attention input [y | mean] is then one matrix), the softmax and the
//               weighted sum;
//   row pass    dX = (dY W) masked by the ReLU of the layer that made X, from mlp3.6 down to mlp1.2, with the softmax, weighted-sum
//               and mean gradients as element-wise kernels between the products;
//   weights     dW = dY^T X and db = the column sums of dY for all eleven layers in ONE launch.
//
// All three are the same kernel: C = A B over arbitrary strides, one wave per 16 x 16 tile of C, 16 x 16 x 4 f32 MFMA, the
// contraction walked in index order by every wave on its own.  No atomics and no split contraction: a gradient is a fixed-order sum
// and two calls give the same bits.  Independent products share a launch (a job list in the kernel arguments); a call is 21
// launches, none of which allocates, synchronises or reads device data on the host.
#include "rgl_mfma.h"
#include "rgl_sarl_shapes.h"

namespace {

constexpr int kLayers = RGL_SARL_LAYERS;            // mlp1.{0,2} mlp2.{0,2} attention.{0,2,4} mlp3.{0,2,4,6}
constexpr int kMaxJobs = kLayers;
constexpr long long kTrainMaxRows = 1ll << 20;     // n_scenes x H: every offset below stays far inside 2^31 floats per buffer

// C[i][j] = epilogue(sum_k A(i, k) B(k, j)): A(i, k) = A[i sai + k sak], B(k, j) = B[k sbk + j sbj], C[i ldc + j]
struct SarlGemmJob {
    const float* A;
    const float* B;
    float* C;
    const float* bias;          // [J] or null: the accumulator starts from it
    const float* mask;          // [I][ldmask] or null: C is zeroed where mask <= 0 (the ReLU of the layer that made the input)
    float* rowsum;              // [I] or null: sum_k A(i, k) -- the bias gradient, A being dY^T
    long long sai, sak, sbk, sbj, ldc, ldmask;
    int I, J, K, relu;
};
struct SarlGemmArgs {
    SarlGemmJob job[kMaxJobs];
};

// A contraction longer than this many k is summed span by span: each span in an accumulator that starts from zero, the spans'
// totals added in order with the rounding error of every addition carried along and added at the end.  The MFMA rounds once per
// k, so one accumulator over the 13120 rows of a batch of 2624 scenes walks 2.8e-6 of a weight gradient's largest element away from
// float64 (mlp1.2.weight), five times upstream's float32 figure; span by span it stays at a span's own error.  Still one wave, one
// fixed order: two calls give the same bits.  Every product of at most kSarlGemmSpan k -- all but the weight gradients over more
// than 256 rows -- is one span and keeps the bits it had.
constexpr int kSarlGemmSpan = 256;

// what the float addition s + x drops (Knuth's TwoSum: additions only, any magnitudes)
__device__ __forceinline__ float two_sum_error(float s, float x) {          // the caller then sets s = s + x
    const float t = s + x;
    const float xr = t - s;
    return (s - (t - xr)) + (x - xr);
}

// Lane (g, n) of a wave (g = lane / 16, n = lane % 16) feeds row 16 ti + n of A and column 16 tj + n of B at k = k0 + 4 g + i in
// step i of a 16-wide k block (the k order of sarl_layer), and owns C rows 16 ti + 4 g + {0..3} of column 16 tj + n.
__global__ __launch_bounds__(256) void sarl_gemm_kernel(const SarlGemmArgs ga) {
    const SarlGemmJob& j = ga.job[blockIdx.y];
    const int wave = threadIdx.x >> 6;
    const unsigned lane = threadIdx.x & 63;
    const int g = lane >> 4, n = lane & 15;
    const int tj_n = (j.J + 15) / 16;
    const long long total = (long long)((j.I + 15) / 16) * tj_n;
    for (long long tile = (long long)blockIdx.x * 4 + wave; tile < total; tile += (long long)gridDim.x * 4) {
        const int ti = (int)(tile / tj_n), tj = (int)(tile % tj_n);
        const int row = 16 * ti + n, col = 16 * tj + n;
        const bool row_ok = row < j.I, col_ok = col < j.J;
        const float* a_row = j.A + (size_t)(row_ok ? row : 0) * j.sai;
        const float* b_col = j.B + (size_t)(col_ok ? col : 0) * j.sbj;
        const float b0 = (j.bias && col_ok) ? j.bias[col] : 0.f;
        f32x4 acc = {b0, b0, b0, b0};
        float rs = 0.f;
        f32x4 sum = acc, err = {0.f, 0.f, 0.f, 0.f};
        float rsum = 0.f, rerr = 0.f;
        for (int c0 = 0; c0 < j.K; c0 += kSarlGemmSpan) {
            const int c1 = c0 + kSarlGemmSpan < j.K ? c0 + kSarlGemmSpan : j.K;
            for (int k0 = c0; k0 < c1; k0 += 16) {
                float a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + 4 * g + i;
                    const bool k_ok = k < j.K;
                    a[i] = (row_ok && k_ok) ? a_row[(size_t)k * j.sak] : 0.f;
                    b[i] = (col_ok && k_ok) ? b_col[(size_t)k * j.sbk] : 0.f;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc = mfma4(a[i], b[i], acc);
                    rs += a[i];
                }
            }
            if (c0 == 0) {              // the only span of every product but a weight gradient over more than kSarlGemmSpan rows
                sum = acc;
                rsum = rs;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    err[i] += two_sum_error(sum[i], acc[i]);
                    sum[i] += acc[i];
                }
                rerr += two_sum_error(rsum, rs);
                rsum += rs;
            }
            acc = f32x4{0.f, 0.f, 0.f, 0.f};
            rs = 0.f;
        }
        if (j.K > kSarlGemmSpan) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sum[i] += err[i];
            rsum += rerr;
        }
        if (col_ok) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 16 * ti + 4 * g + i;
                if (r >= j.I) continue;
                float v = sum[i];
                if (j.relu) v = fmaxf(v, 0.f);
                if (j.mask && !(j.mask[(size_t)r * j.ldmask + col] > 0.f)) v = 0.f;
                j.C[(size_t)r * j.ldc + col] = v;
            }
        }
        if (j.rowsum && tj == 0) {          // wave-uniform: every lane takes part in the butterfly
            const float s = kgroups_sum(rsum);
            if (g == 0 && row_ok) j.rowsum[row] = s;
        }
    }
}

// The element-wise steps between the products sum in float64: they are a few hundred operations per scene, and the softmax's gradient
// is a difference of nearly equal terms (with the default initialisation the attention is uniform to three digits).

// the mean of mlp1's outputs over a scene's humans, written behind every row of the scene: ain [S H][200] = [y | mean]
__global__ void sarl_mean_kernel(float* __restrict__ ain, int S, int H) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)S * 100) return;
    const size_t s = (size_t)(t / 100);
    const int c = (int)(t % 100);
    float* base = ain + s * H * 200 + c;
    double sum = 0.0;
    for (int h = 0; h < H; ++h) sum += (double)base[(size_t)h * 200];
    const float m = (float)(sum / (double)H);
    for (int h = 0; h < H; ++h) base[(size_t)h * 200 + 100] = m;
}

// softmax over a scene's humans (sarl.py:57-63 with an all-ones mask), the weighted sum of the mlp2 outputs and the six self
// features of row 0 in front of it: one 64-thread block per scene, every thread walking the humans in order
__global__ __launch_bounds__(64) void sarl_softmax_joint_kernel(const float* __restrict__ rows, const float* __restrict__ score,
                                                                const float* __restrict__ feat, int H, int D,
                                                                float* __restrict__ att, float* __restrict__ joint) {
    const size_t s = blockIdx.x;
    const int c = threadIdx.x;
    const float* sc = score + s * H;
    float smax = -INFINITY;
    for (int h = 0; h < H; ++h) smax = fmaxf(smax, sc[h]);
    double ssum = 0.0;
    for (int h = 0; h < H; ++h) ssum += exp((double)sc[h] - (double)smax);
    double acc = 0.0;
    for (int h = 0; h < H; ++h) {
        const float w = (float)(exp((double)sc[h] - (double)smax) / ssum);
        if (c == 0) att[s * H + h] = w;
        if (c < 50) acc += (double)w * (double)feat[(s * H + h) * 50 + c];
    }
    if (c < 6) joint[s * 56 + c] = rows[s * H * D + c];
    if (c < 50) joint[s * 56 + 6 + c] = (float)acc;
}

// d feat[h] = w_h d joint[6..], d w_h = <d joint[6..], feat[h]>, d score_h = w_h (d w_h - sum_h' w_h' d w_h' / sum_h' w_h'): the
// stored weights sum to one only up to their rounding, and dividing by their sum keeps the scores' gradients of a scene summing to
// zero, as the shift-invariant softmax has it.  One block per scene.
__global__ __launch_bounds__(64) void sarl_softmax_backward_kernel(const float* __restrict__ att, const float* __restrict__ feat,
                                                                   const float* __restrict__ djoint, int H,
                                                                   float* __restrict__ dfeat, float* __restrict__ dscore) {
    __shared__ double dw[RGL_SARL_MAX_HUMANS];
    const size_t s = blockIdx.x;
    const int c = threadIdx.x;
    const float* dj = djoint + s * 56 + 6;
    for (int h = c; h < H; h += 64) {
        const float* f = feat + (s * H + h) * 50;
        double d = 0.0;
        for (int k = 0; k < 50; ++k) d += (double)dj[k] * (double)f[k];
        dw[h] = d;
    }
    __syncthreads();
    double dot = 0.0, wsum = 0.0;
    for (int h = 0; h < H; ++h) {
        dot += (double)att[s * H + h] * dw[h];
        wsum += (double)att[s * H + h];
    }
    dot /= wsum;
    for (int h = c; h < H; h += 64) dscore[s * H + h] = (float)((double)att[s * H + h] * (dw[h] - dot));
    if (c < 50) {
        const float d = dj[c];
        for (int h = 0; h < H; ++h) dfeat[(s * H + h) * 50 + c] = att[s * H + h] * d;
    }
}

// the gradient of mlp1's pre-activation output: what mlp2 sends back, what the attention sends back to the row itself and -- with the
// global state -- the mean's share (d mean summed over the scene's humans in order, divided by H), masked by mlp1's last ReLU
__global__ void sarl_combine_kernel(const float* __restrict__ dym, const float* __restrict__ dain, const float* __restrict__ y,
                                    int S, int H, int KA, float* __restrict__ dy) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)S * 100) return;
    const size_t s = (size_t)(t / 100);
    const int c = (int)(t % 100);
    double share = 0.0;
    if (KA == 200) {
        for (int h = 0; h < H; ++h) share += (double)dain[(s * H + h) * 200 + 100 + c];
        share /= (double)H;
    }
    for (int h = 0; h < H; ++h) {
        const size_t r = s * H + h;
        const double v = (double)dym[r * 100 + c] + (double)dain[r * KA + c] + share;
        dy[r * 100 + c] = y[r * KA + c] > 0.f ? (float)v : 0.f;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct SarlTrainShape {
    int D, KA;                  // row width; attention input width (200 with the global state)
    int K[kLayers], M[kLayers];
    const float* wt[kLayers];   // k-major [K][M]
    const float* bias[kLayers];
};

inline SarlTrainShape sarl_train_shape(const SarlPlanner& pl) {
    SarlTrainShape sh;
    sh.D = 13 + sarl_map_floats(pl);
    sh.KA = pl.with_global_state ? 200 : 100;
    const RglMlp* ms[4] = {&pl.mlp1, &pl.mlp2, &pl.attention, &pl.mlp3};
    int l = 0;
    for (int m = 0; m < 4; ++m)
        for (int k = 0; k < ms[m]->n_layers; ++k, ++l) {
            sh.K[l] = ms[m]->dims[k];
            sh.M[l] = ms[m]->dims[k + 1];
            sh.wt[l] = ms[m]->weight[k];
            sh.bias[l] = ms[m]->bias[k];
        }
    return sh;
}

// the backward's buffers: floats per (scene, human) row and per scene, in the order sarl_train_buffers hands them out
enum { bH1, bAIN, bA1, bA2, bSC, bM1, bFEAT, bATT, bDFEAT, bDSC, bDM1, bDA2, bDA1, bDAIN, bDYM, bDY, bDH1, kRowBuffers };
enum { bJOINT, bP1, bP2, bP3, bDP3, bDP2, bDP1, bDJOINT, kSceneBuffers };

// [sarl_value_f32's workspace | attention weights of a call that asks for none | the backward's buffers: rb of R = S H rows each,
// sb of S rows each]; over a null base the sizes alone.  false: unsupported
struct SarlTrainScratch {
    size_t value_bytes;
    float* attention;
    float *rb[kRowBuffers], *sb[kSceneBuffers];
    long long bytes;
};

inline bool carve_sarl_train(void* base, const SarlPlanner& pl, int n_scenes, int H, SarlTrainScratch& w) {
    if (n_scenes < 1 || H < 1 || (long long)n_scenes * H > kTrainMaxRows) return false;
    w.value_bytes = sarl_value_workspace_bytes_for(&pl, n_scenes, H);
    if (!w.value_bytes) return false;
    const int KA = pl.with_global_state ? 200 : 100;
    const int row[kRowBuffers] = {150, KA, 100, 100, 1, 100, 50, 1, 50, 1, 100, 100, 100, KA, 100, 100, 150};
    const int scene[kSceneBuffers] = {56, 150, 100, 100, 100, 100, 150, 56};
    const long long S = n_scenes, R = S * H;
    Carver c{(char*)base, (long long)w.value_bytes};
    w.attention = c.take<float>(R * 4);
    for (int i = 0; i < kRowBuffers; ++i) w.rb[i] = c.take<float>(R * row[i] * 4);
    for (int i = 0; i < kSceneBuffers; ++i) w.sb[i] = c.take<float>(S * scene[i] * 4);
    w.bytes = c.off;
    return true;
}

struct SarlGemmLaunch {
    SarlGemmArgs args;
    int n = 0;
    long long tiles = 0;

    SarlGemmJob& add(const float* A, long long sai, long long sak, const float* B, long long sbk, long long sbj, float* C, long long ldc,
                     int I, int J, int K) {
        SarlGemmJob& j = args.job[n++];
        j = SarlGemmJob{};
        j.A = A; j.sai = sai; j.sak = sak;
        j.B = B; j.sbk = sbk; j.sbj = sbj;
        j.C = C; j.ldc = ldc;
        j.I = I; j.J = J; j.K = K;
        const long long t = (long long)((I + 15) / 16) * ((J + 15) / 16);
        tiles = t > tiles ? t : tiles;
        return j;
    }
    // out [rows][ldo] = act(in [rows][ldi] Wt + b)
    void forward(const SarlTrainShape& sh, int l, const float* in, long long ldi, float* out, long long ldo, long long rows, bool relu) {
        SarlGemmJob& j = add(in, ldi, 1, sh.wt[l], sh.M[l], 1, out, ldo, (int)rows, sh.M[l], sh.K[l]);
        j.bias = sh.bias[l];
        j.relu = relu;
    }
    // din [rows][ldi] = (dout [rows][ldo] W) masked by `mask` (the activations the layer read, where a ReLU made them)
    void input_grad(const SarlTrainShape& sh, int l, const float* dout, long long ldo, float* din, long long ldi, long long rows,
                    const float* mask, long long ldmask) {
        SarlGemmJob& j = add(dout, ldo, 1, sh.wt[l], 1, sh.M[l], din, ldi, (int)rows, sh.K[l], sh.M[l]);
        j.mask = mask;
        j.ldmask = ldmask;
    }
    // dW [M][K] = dout^T in, db [M] = the column sums of dout, both over the rows in row order
    void weight_grad(const SarlTrainShape& sh, int l, const float* dout, long long ldo, const float* in, long long ldi, long long rows,
                     const SarlGrads& gr) {
        SarlGemmJob& j = add(dout, 1, ldo, in, ldi, 1, gr.weight[l], sh.K[l], sh.M[l], sh.K[l], (int)rows);
        j.rowsum = gr.bias[l];
    }
    int launch(hipStream_t st) {
        const long long blocks = (tiles + 3) / 4;
        hipLaunchKernelGGL(sarl_gemm_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048), n), dim3(256), 0, st, args);
        RGL_LAUNCH_CHECK();
        return RGL_OK;
    }
};

#define SARL_TRY(expr)            \
    do {                          \
        const int rc__ = (expr);  \
        if (rc__) return rc__;    \
    } while (0)

}  // namespace

extern "C" size_t sarl_train_workspace_bytes(const SarlPlanner* planner, int n_scenes, int H) {
    SarlTrainScratch w;
    if (!planner || validate_sarl(*planner, H) || !carve_sarl_train(nullptr, *planner, n_scenes, H, w)) return 0;
    return (size_t)w.bytes;
}

extern "C" int sarl_value_train_f32(const SarlPlanner* planner, const float* rows, int n_scenes, int H, void* workspace,
                                    size_t workspace_bytes, float* value, float* attention, rgl_stream_t stream) {
    if (!planner || !rows || !workspace || !value) return RGL_ERR_NULL;
    SARL_TRY(validate_sarl(*planner, H));
    SarlTrainScratch w;
    if (!carve_sarl_train(workspace, *planner, n_scenes, H, w)) return RGL_ERR_BAD_SHAPE;
    if (workspace_bytes < (size_t)w.bytes) return RGL_ERR_WORKSPACE;
    if (!attention) attention = w.attention;
    return sarl_value_f32(planner, rows, nullptr, nullptr, nullptr, n_scenes, 1, H, workspace, w.value_bytes, value, attention, stream);
}

extern "C" int sarl_value_backward_f32(const SarlPlanner* planner, const float* rows, const float* grad_value, int n_scenes, int H,
                                       void* workspace, size_t workspace_bytes, const SarlGrads* grads, rgl_stream_t stream) {
    if (!planner || !rows || !grad_value || !workspace || !grads) return RGL_ERR_NULL;
    for (int l = 0; l < kLayers; ++l)
        if (!grads->weight[l] || !grads->bias[l]) return RGL_ERR_NULL;
    SARL_TRY(validate_sarl(*planner, H));
    SarlTrainScratch w;
    if (!carve_sarl_train(workspace, *planner, n_scenes, H, w)) return RGL_ERR_BAD_SHAPE;
    if (workspace_bytes < (size_t)w.bytes) return RGL_ERR_WORKSPACE;
    const SarlTrainShape sh = sarl_train_shape(*planner);
    const long long S = n_scenes, R = S * H;
    const int KA = sh.KA, D = sh.D;
    const bool global = planner->with_global_state != 0;
    hipStream_t st = (hipStream_t)stream;

    float* const* rb = w.rb;
    float* const* sb = w.sb;
    const float* y = rb[bAIN];              // mlp1's outputs: the first 100 columns of the attention input, row stride KA

    // ---- the activations again ----
    { SarlGemmLaunch g; g.forward(sh, 0, rows, D, rb[bH1], 150, R, true); SARL_TRY(g.launch(st)); }
    { SarlGemmLaunch g; g.forward(sh, 1, rb[bH1], 150, rb[bAIN], KA, R, true); SARL_TRY(g.launch(st)); }
    if (global) {
        hipLaunchKernelGGL(sarl_mean_kernel, dim3((unsigned)((S * 100 + 255) / 256)), dim3(256), 0, st, rb[bAIN], (int)S, H);
        RGL_LAUNCH_CHECK();
    }
    {
        SarlGemmLaunch g;
        g.forward(sh, 4, rb[bAIN], KA, rb[bA1], 100, R, true);
        g.forward(sh, 2, y, KA, rb[bM1], 100, R, true);
        SARL_TRY(g.launch(st));
    }
    {
        SarlGemmLaunch g;
        g.forward(sh, 5, rb[bA1], 100, rb[bA2], 100, R, true);
        g.forward(sh, 3, rb[bM1], 100, rb[bFEAT], 50, R, false);
        SARL_TRY(g.launch(st));
    }
    { SarlGemmLaunch g; g.forward(sh, 6, rb[bA2], 100, rb[bSC], 1, R, false); SARL_TRY(g.launch(st)); }
    hipLaunchKernelGGL(sarl_softmax_joint_kernel, dim3((unsigned)S), dim3(64), 0, st, rows, rb[bSC], rb[bFEAT], H, D, rb[bATT], sb[bJOINT]);
    RGL_LAUNCH_CHECK();
    { SarlGemmLaunch g; g.forward(sh, 7, sb[bJOINT], 56, sb[bP1], 150, S, true); SARL_TRY(g.launch(st)); }
    { SarlGemmLaunch g; g.forward(sh, 8, sb[bP1], 150, sb[bP2], 100, S, true); SARL_TRY(g.launch(st)); }
    { SarlGemmLaunch g; g.forward(sh, 9, sb[bP2], 100, sb[bP3], 100, S, true); SARL_TRY(g.launch(st)); }

    // ---- the row pass: pre-activation gradients from the value down ----
    { SarlGemmLaunch g; g.input_grad(sh, 10, grad_value, 1, sb[bDP3], 100, S, sb[bP3], 100); SARL_TRY(g.launch(st)); }
    { SarlGemmLaunch g; g.input_grad(sh, 9, sb[bDP3], 100, sb[bDP2], 100, S, sb[bP2], 100); SARL_TRY(g.launch(st)); }
    { SarlGemmLaunch g; g.input_grad(sh, 8, sb[bDP2], 100, sb[bDP1], 150, S, sb[bP1], 150); SARL_TRY(g.launch(st)); }
    { SarlGemmLaunch g; g.input_grad(sh, 7, sb[bDP1], 150, sb[bDJOINT], 56, S, nullptr, 0); SARL_TRY(g.launch(st)); }
    hipLaunchKernelGGL(sarl_softmax_backward_kernel, dim3((unsigned)S), dim3(64), 0, st, rb[bATT], rb[bFEAT], sb[bDJOINT], H, rb[bDFEAT],
                       rb[bDSC]);
    RGL_LAUNCH_CHECK();
    {
        SarlGemmLaunch g;
        g.input_grad(sh, 3, rb[bDFEAT], 50, rb[bDM1], 100, R, rb[bM1], 100);
        g.input_grad(sh, 6, rb[bDSC], 1, rb[bDA2], 100, R, rb[bA2], 100);
        SARL_TRY(g.launch(st));
    }
    {
        SarlGemmLaunch g;
        g.input_grad(sh, 2, rb[bDM1], 100, rb[bDYM], 100, R, nullptr, 0);
        g.input_grad(sh, 5, rb[bDA2], 100, rb[bDA1], 100, R, rb[bA1], 100);
        SARL_TRY(g.launch(st));
    }
    { SarlGemmLaunch g; g.input_grad(sh, 4, rb[bDA1], 100, rb[bDAIN], KA, R, nullptr, 0); SARL_TRY(g.launch(st)); }
    hipLaunchKernelGGL(sarl_combine_kernel, dim3((unsigned)((S * 100 + 255) / 256)), dim3(256), 0, st, rb[bDYM], rb[bDAIN], y, (int)S, H, KA,
                       rb[bDY]);
    RGL_LAUNCH_CHECK();
    { SarlGemmLaunch g; g.input_grad(sh, 1, rb[bDY], 100, rb[bDH1], 150, R, rb[bH1], 150); SARL_TRY(g.launch(st)); }

    // ---- all weight and bias gradients: one launch ----
    SarlGemmLaunch g;
    g.weight_grad(sh, 0, rb[bDH1], 150, rows, D, R, *grads);
    g.weight_grad(sh, 1, rb[bDY], 100, rb[bH1], 150, R, *grads);
    g.weight_grad(sh, 2, rb[bDM1], 100, y, KA, R, *grads);
    g.weight_grad(sh, 3, rb[bDFEAT], 50, rb[bM1], 100, R, *grads);
    g.weight_grad(sh, 4, rb[bDA1], 100, rb[bAIN], KA, R, *grads);
    g.weight_grad(sh, 5, rb[bDA2], 100, rb[bA1], 100, R, *grads);
    g.weight_grad(sh, 6, rb[bDSC], 1, rb[bA2], 100, R, *grads);
    g.weight_grad(sh, 7, sb[bDP1], 150, sb[bJOINT], 56, S, *grads);
    g.weight_grad(sh, 8, sb[bDP2], 100, sb[bP1], 150, S, *grads);
    g.weight_grad(sh, 9, sb[bDP3], 100, sb[bP2], 100, S, *grads);
    g.weight_grad(sh, 10, grad_value, 1, sb[bP3], 100, S, *grads);
    return g.launch(st);
}
