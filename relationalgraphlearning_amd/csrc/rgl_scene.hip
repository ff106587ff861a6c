// rgl_scene.hip -- state-predictor path of the rollout: scenes with their own crowds (one graph forward per tree node).
// Follows (reference paths): crowd_nav/policy/state_predictor.py:20-39, graph_model.py:99-130.
#include "rgl_scene_body.h"

namespace {

// ------------------------------------------------------------------------------------------------
// state-predictor path: scenes with their own crowds (one graph forward per tree node)
//   row_mlp2_kernel   : batched 2-layer embedding MLP over rows (IN -> 64 -> 32, ReLU after both) as an MFMA chain
//   scene_graph_kernel: one wave per scene: S = (X Wa) X^T, softmax, L x relu(A H W)(+H), motion head 32->64->5
// ------------------------------------------------------------------------------------------------
struct RowMlpArgs {
    const float *w1, *b1, *w2, *b2;   // k-major [IN][64], [64], [64][32], [32]
    const float* rows;                // [M][IN]
    float* out;                       // [M][32]
    int M, n_tiles;
};

// One wave per 16-row tile: IN -> 64 -> 32 with ReLU after both layers (row_mlp2_tile, rgl_scene_body.h).
template <int IN>
__device__ __forceinline__ void row_mlp2_tiles(const RowMlpArgs& a, const float* lds_set, int first, int stride, int lane) {
    const int n = lane & 15, q = lane >> 4;
    for (int tile = first; tile < a.n_tiles; tile += stride) {
        const int row = 16 * tile + n;
        const int rc = row < a.M ? row : a.M - 1;
        f32x4 o[2];
        row_mlp2_tile<IN>(lds_set, a.rows + (size_t)rc * IN, lane, o);
        if (row < a.M) {
            float* dst = a.out + (size_t)row * XD;
            *reinterpret_cast<f32x4*>(dst + 4 * q) = o[0];
            *reinterpret_cast<f32x4*>(dst + 16 + 4 * q) = o[1];
        }
    }
}

// Both embedding MLPs of a level in ONE launch (they are launch-latency sized): workgroups [0, grid_a) take the robot rows
// (INA inputs), the others the human rows (INB inputs).  (9, 5): path M's full / observable states; (6, 7): path G's rotated
// self / human features (gcn.py:34-47).
// `grid_mlp` < gridDim.x: the workgroups past the two MLPs run the level's independent next-robot-state / reward work (rgl_children.h)
// in the same launch -- with many scenes that work does not ride in the scene kernel (see scene_graph_kernel) and was a launch of its
// own between this one and the scene kernel.
template <int INA, int INB>
__global__ __launch_bounds__(kThreads, 2) void row_mlp2_pair_kernel(const RowMlpArgs ra, const RowMlpArgs rb, int grid_a, int grid_mlp,
                                                                    const ChildrenArgs ca) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if ((int)blockIdx.x >= grid_mlp) {
        const long long total = (long long)ca.P * ca.A, stride = (long long)(gridDim.x - grid_mlp) * kThreads;
        const long long first_pair = (long long)(blockIdx.x - grid_mlp) * kThreads + threadIdx.x;
        if (ca.A >= 64 && ca.H <= 64 && !ca.robot64) {
            const float v_max = table_speed_bound(ca);
            for (long long base = first_pair & ~63LL; base < total; base += stride) children_wave(ca, base, total, v_max);
        } else {
            for (long long idx = first_pair; idx < total; idx += stride) children_thread(ca, idx);
        }
        return;
    }
    constexpr int F1 = 0, F2 = F1 + 4 * 1 * 4 * 64, B1 = F2 + 2 * 4 * 4 * 64, B2 = B1 + HID;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool first = (int)blockIdx.x < grid_a;
    const RowMlpArgs& a = first ? ra : rb;
    if (first) fill_frags<INA, HID, kThreads>(lds + F1, a.w1, tid); else fill_frags<INB, HID, kThreads>(lds + F1, a.w1, tid);
    fill_frags<HID, XD, kThreads>(lds + F2, a.w2, tid);
    fill_bias<HID>(lds + B1, a.b1, tid);
    fill_bias<XD>(lds + B2, a.b2, tid);
    __syncthreads();
    const int b = first ? blockIdx.x : blockIdx.x - grid_a, g = first ? grid_a : grid_mlp - grid_a;
    if (first) row_mlp2_tiles<INA>(a, lds, b + g * wave, g * kWaves, lane);       // partial round: one tile per workgroup
    else row_mlp2_tiles<INB>(a, lds, b + g * wave, g * kWaves, lane);
}

// SceneArgs, LevelPrologue and the kernel's body (scene_body): rgl_scene_body.h

// One scene per wave (SPLIT: per NT waves).  CH = true: the level's independent next-robot-state / reward work (float64 VALU) rides
// in this launch on EXTRA workgroups [grid_scene, gridDim.x) (see rgl_scene_body.h for when that pays).
template <int NT, int SK, int WAVES, bool CH, bool SPLIT, bool EMB = false, bool BX = false>
__global__ __launch_bounds__(WAVES * 64, 2) void scene_graph_kernel(const SceneArgs a, const ChildrenArgs ca, int grid_scene) {
    constexpr int kSceneThreads = WAVES * 64;
    constexpr int kSlots = SPLIT ? WAVES / NT : WAVES;      // scenes in flight per workgroup
    if constexpr (CH) {
        if ((int)blockIdx.x >= grid_scene) {
            const long long total = (long long)ca.P * ca.A, stride = (long long)(gridDim.x - grid_scene) * kSceneThreads;
            const long long first = (long long)(blockIdx.x - grid_scene) * kSceneThreads + threadIdx.x;
            if (ca.A >= 64 && ca.H <= 64 && !ca.robot64) {       // whole waves: far-human masks per parent (children_wave)
                const float v_max = table_speed_bound(ca);
                for (long long base = first & ~63LL; base < total; base += stride) children_wave(ca, base, total, v_max);
            } else {
                for (long long idx = first; idx < total; idx += stride) children_thread(ca, idx);
            }
            return;
        }
    }
    extern __shared__ __attribute__((aligned(16))) float lds[];
    scene_body<NT, SK, WAVES, SPLIT, EMB, BX>(a, lds, blockIdx.x, grid_scene, grid_scene * kSlots, a.P);
}

// SceneImageLayout / scene_image_layout (the weight image's layout, LDS region and packed global copy alike): rgl_scene_body.h
struct SceneImageArgs {
    const float* wa;                      // null: identity (gaussian)
    const float* Ws[4];
    const float *wm1, *bm1, *wm2, *bm2;   // null: no motion head (value rows)
    int L;
    SceneImageLayout lo;
};

// the BX image: three-piece bf16 fragments of Wa, W_l, wm1, wm2 (no scales: bf16 has f32's exponent range) + the two bias vectors
__global__ __launch_bounds__(256) void scene_pack_b6_kernel(const SceneImageArgs a, float* img) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const SceneImageLayout& lo = a.lo;
    if (e >= lo.total) return;
    float v = 0.f;
    if (e < lo.off_ws) {
        const int i = e - lo.off_wa;
        if (i < B6Floats<XD, XD>::v) {
            if (a.wa) v = frag_bf3_ld<XD, XD>(a.wa, XD, XD, i);
            else {                                              // gaussian: Wa = I -> hi piece 1 on the diagonal
                const int u = i >> 2, p = i & 3, l = u & 63, rest = u >> 6, pc = rest % 3, ot = rest / 3;
                bf16x2 d;
                for (int k = 0; k < 2; ++k) {
                    const int ee = 2 * p + k, in = 16 * (ee >> 2) + 4 * (l >> 4) + (ee & 3), out = 16 * ot + (l & 15);
                    d[k] = (__bf16)((pc == 0 && in == out) ? 1.f : 0.f);
                }
                v = __builtin_bit_cast(float, d);
            }
        }
    } else if (e < lo.off_wm1) {
        const int i = e - lo.off_ws, l = i / lo.ws_stride, j = i - l * lo.ws_stride;
        if (l < a.L && j < B6Floats<XD, XD>::v) v = frag_bf3_ld<XD, XD>(a.Ws[l], XD, XD, j);
    } else if (e < lo.off_bm1) {
        const int i = e - lo.off_wm1;
        if (a.wm1 && i < B6Floats<XD, HID>::v) v = frag_bf3_ld<XD, HID>(a.wm1, HID, HID, i);
    } else if (e < lo.off_wm2) {
        const int i = e - lo.off_bm1;
        if (a.bm1 && i < HID) v = a.bm1[i];
    } else if (e < lo.off_bm2) {
        const int i = e - lo.off_wm2;
        if (a.wm2 && i < B6Floats<HID, 16>::v) v = frag_bf3_ld<HID, 16>(a.wm2, 5, 5, i);
    } else {
        const int i = e - lo.off_bm2;
        if (a.bm2 && i < 5) v = a.bm2[i];
    }
    img[e] = v;
}

inline RowMlpArgs row_mlp_args(const RglMlp& m, const float* rows, float* out, int M) {
    RowMlpArgs ra;
    ra.w1 = m.weight[0]; ra.b1 = m.bias[0]; ra.w2 = m.weight[1]; ra.b2 = m.bias[1];
    ra.rows = rows; ra.out = out; ra.M = M; ra.n_tiles = (M + 15) / 16;
    return ra;
}

// robot rows [Ma][9] -> [Ma][32] with w_r, human rows [Mb][5] -> [Mb][32] with w_h
// `children` (optional): the level's reward / next-state work on extra workgroups of this launch
inline int launch_row_mlp2_pair(const RglMlp& wr, const float* robot_rows, float* x0_out, int Ma, const RglMlp& wh,
                                const float* human_rows, float* xh_out, int Mb, hipStream_t st, const ChildrenArgs* children = nullptr) {
    const RowMlpArgs ra = row_mlp_args(wr, robot_rows, x0_out, Ma), rb = row_mlp_args(wh, human_rows, xh_out, Mb);
    int grid_a = (ra.n_tiles + kWaves - 1) / kWaves, grid_b = (rb.n_tiles + kWaves - 1) / kWaves;
    if (grid_a > 256) grid_a = 256;
    if (grid_b > 1024) grid_b = 1024;
    ChildrenArgs ca{};
    int grid_c = 0;
    if (children) {
        ca = *children;
        const long long blocks = ((long long)ca.P * ca.A + kThreads - 1) / kThreads;
        grid_c = (int)(blocks < 4096 ? blocks : 4096);
    }
    const int grid_mlp = grid_a + grid_b;
    if (wr.dims[0] == 9)
        hipLaunchKernelGGL((row_mlp2_pair_kernel<9, 5>), dim3(grid_mlp + grid_c), dim3(kThreads), kRowMlpSetFloats * sizeof(float), st, ra,
                           rb, grid_a, grid_mlp, ca);
    else
        hipLaunchKernelGGL((row_mlp2_pair_kernel<6, 7>), dim3(grid_mlp + grid_c), dim3(kThreads), kRowMlpSetFloats * sizeof(float), st, ra,
                           rb, grid_a, grid_mlp, ca);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

// ---- the launch decisions, each made in ONE place: read by the launchers below and by rgl_plan_scene_forward -----------------------
// node tiles of an N-node scene: 1..4 tiles of 16, the eight-tile form beyond 64 nodes
inline int scene_node_tiles(int N) { return N > 64 ? 8 : (N + 15) / 16; }

// Split scenes (NT waves per scene) below this many scenes: env RGL_SCENE_SPLIT_BELOW overrides (0 = never, tests / measurements)
inline int scene_split_below(int nt) {
    const int env = scene_split_below_asked();
    if (env >= 0) return env;
    return nt == 2 ? 3072 : 4096;
}

// few scenes of the shipped shape: the scene kernel embeds its own node tiles (one launch for the level instead of two)
inline bool scene_embeds_inside(const RglGraph& g, int NT0, int P, bool embed_children) {
    return scene_embed_inside_enabled() && !embed_children && g.w_r.dims[0] == 9 && scene_similarity_mode(g) == SIM_SOFTMAX &&
           (NT0 == 1 || NT0 == 2 || NT0 == 4) && P <= 512 &&     // measured: +1.5-3 % up to 512 scenes, -2 % at 1-2 k (sibling scenes repeat their crowd's rows)
           (NT0 == 1 || P < scene_split_below(NT0));       // the split form (see launch_scene)
}

// scene slots the LDS region of a launch holds (fill_scene_args): one per wave, or -- the split form, which launch_scene always
// takes with the embeddings inside -- one per NT waves of its 8 (with the unsplit count a 50-agent scene workgroup held 95 KB instead
// of 76: one per CU, and the launch's reward workgroups, which reserve the same LDS, waited for a scene workgroup to retire)
inline int scene_region_slots(int NT, bool embed_inside) {
    const bool wide_slots = scene_wide_slots();      // measurements
    return (embed_inside && (NT == 2 || NT == 4) && !wide_slots) ? 8 / NT : (NT <= 2 ? 8 : (NT <= 4 ? 4 : 1));
}

// scenes in flight per workgroup of an instantiation, and the most scene workgroups of a launch (one or two per CU by LDS; 4-wave
// workgroups: twice as many)
constexpr int scene_slots(bool split, int waves, int nt) { return split ? waves / nt : waves; }
inline int scene_grid_cap(size_t lds_bytes, int waves) {
    return rgl::kCuCount * rgl::workgroups_per_cu_by_lds(lds_bytes, 2) * (waves == 4 ? 2 : 1);
}

// the level's reward / next-state work rides in the scene kernel's launch below this many scenes (launch_predict_humans)
// cross-over: ~3 k scenes for the f32 scene kernel (round 2), ~1.1 k once its weight products run on the matrix pipe (round 5:
// 2048 roots 0.3022 -> 0.2988 ms, 1024 roots 0.1773 -> 0.1759, 512 roots unchanged); RGL_SCENE_CHILDREN_BELOW overrides (measurements)
inline int scene_children_below(bool bf16x6) {
    const int below_env = scene_children_below_asked();
    return below_env >= 0 ? below_env : (bf16x6 ? 1100 : 3072);
}

// What a launch would be, recorded INSTEAD of launched (rgl_plan_scene_forward): with a ScenePlan the launchers below take every
// branch they take otherwise and stop short of the launch itself.
struct ScenePlan {
    int node_tiles, family, waves, split, embed_inside, bx, slots, grid, grid_cap, children_riding, embed_launch;
    size_t lds_bytes;
};

template <int NT, int SK, int WAVES, bool SPLIT = false, bool EMB = false, bool BX = false>
int launch_scene_k(const SceneArgs& sa, size_t lds_bytes, const ChildrenArgs* children, hipStream_t st, ScenePlan* plan = nullptr) {
    if constexpr (!SPLIT && SK != 3 && (NT == 2 || NT == 4)) {
        if (sa.P < scene_split_below(NT)) return launch_scene_k<NT, SK, 8, true, EMB, BX>(sa, lds_bytes, children, st, plan);
    }
    constexpr int kSlots = scene_slots(SPLIT, WAVES, NT);
    int grid = (sa.P + kSlots - 1) / kSlots;
    const int cap = scene_grid_cap(lds_bytes, WAVES);
    if (grid > cap) grid = cap;
    if (plan) {
        plan->node_tiles = NT; plan->family = SK; plan->waves = WAVES; plan->split = SPLIT; plan->embed_inside = EMB; plan->bx = BX;
        plan->slots = kSlots; plan->grid = grid; plan->grid_cap = cap; plan->children_riding = children != nullptr;
        plan->lds_bytes = lds_bytes;
        return RGL_OK;
    }
    ChildrenArgs ca{};
    int grid_children = 0;
    if (children) {
        ca = *children;
        const long long blocks = ((long long)ca.P * ca.A + WAVES * 64 - 1) / (WAVES * 64);
        grid_children = (int)(blocks < 2048 ? blocks : 2048);
    }
    auto kern = children ? scene_graph_kernel<NT, SK, WAVES, true, SPLIT, EMB, BX> : scene_graph_kernel<NT, SK, WAVES, false, SPLIT, EMB, BX>;
    return rgl::launch_lds(kern,dim3(grid + grid_children), dim3(WAVES * 64), lds_bytes, st, sa, ca, grid);
}

// 64 < N <= 128: eight column tiles, always split over the eight waves of a workgroup (one scene per workgroup pass; the
// unsplit form would hold an 8 x 8 block of adjacency tiles per wave: 256 VGPRs).  The pair-MLP similarity has no split form.
inline int launch_scene_wide(const SceneArgs& sa, size_t lds_bytes, const ChildrenArgs* children, hipStream_t st, ScenePlan* plan = nullptr) {
    if (sa.sim == SIM_SOFTMAX) return launch_scene_k<8, 0, 8, true>(sa, lds_bytes, children, st, plan);
    if (sa.sim == SIM_COSINE || sa.sim == SIM_COSINE_SOFTMAX) return launch_scene_k<8, 2, 8, true>(sa, lds_bytes, children, st, plan);
    if (sa.sim == SIM_CONCAT) return RGL_ERR_BAD_MODE;      // (never asked: scene_kernel_covers ends the pair MLP at 64 nodes)
    return launch_scene_k<8, 1, 8, true>(sa, lds_bytes, children, st, plan);
}

template <int NT, int WAVES>
int launch_scene(const SceneArgs& sa, size_t lds_bytes, const ChildrenArgs* children, hipStream_t st, ScenePlan* plan = nullptr) {
    if constexpr (NT == 2) {
        if (sa.bx)                                       // six-term bf16 weight products (softmax similarity, two node tiles)
            return sa.robot_rows ? launch_scene_k<2, 0, 8, true, true, true>(sa, lds_bytes, children, st, plan)
                                 : launch_scene_k<2, 0, WAVES, false, false, true>(sa, lds_bytes, children, st, plan);
    }
    if constexpr (NT == 1) {
        if (sa.robot_rows) return launch_scene_k<1, 0, 8, false, true>(sa, lds_bytes, children, st, plan);           // embeddings inside
    }
    if constexpr (NT == 2 || NT == 4) {
        if (sa.robot_rows) return launch_scene_k<NT, 0, 8, true, true>(sa, lds_bytes, children, st, plan);          // ... and split scenes
    }
    if (sa.sim == SIM_SOFTMAX) return launch_scene_k<NT, 0, WAVES>(sa, lds_bytes, children, st, plan);
    if (sa.sim == SIM_COSINE || sa.sim == SIM_COSINE_SOFTMAX) return launch_scene_k<NT, 2, WAVES>(sa, lds_bytes, children, st, plan);
    if (sa.sim == SIM_CONCAT) return launch_scene_k<NT, 3, WAVES>(sa, lds_bytes, children, st, plan);
    return launch_scene_k<NT, 1, WAVES>(sa, lds_bytes, children, st, plan);
}

static bool scene_kernel_covers(const RglGraph& g, int N) {
    const bool path_m = mlp_is(g.w_r, 9, HID, XD, true) && mlp_is(g.w_h, 5, HID, XD, true);
    const bool path_g = mlp_is(g.w_r, 6, HID, XD, true) && mlp_is(g.w_h, 7, HID, XD, true);        // gcn.ValueNetwork's inputs
    return fast_path_enabled() && scene_similarity_mode(g) >= 0 && g.x_dim == XD && g.num_layer >= 1 && g.num_layer <= 4 &&
           (path_m || path_g) && N <= 128 && (N <= 64 || scene_similarity_mode(g) != SIM_CONCAT);
}

// SceneArgs of the scene kernel (and of the level prologue); returns the LDS floats.  `slots` > 0: the level prologue -- that many
// scene slots in the workgroup (one per wave) and the row buffer of its cooperative embeddings, as large as `region_floats` LDS floats
// leave room for; 0: the launcher's choice
static int fill_scene_args(SceneArgs& sa, const RglGraph& g, const RglMlp* mh, const float* robot, const float* humans, int crowds_per,
                           int P, int H, float* humans_next, float* rows_out, float* x0_rows, float* xh_rows, bool embed_inside,
                           const float* sp_image, int slots, int region_floats = 0) {
    const int N = H + 1;
    const int NT = scene_node_tiles(N);
    sa.robot_rows = embed_inside ? robot : nullptr;
    sa.human_rows = embed_inside ? humans : nullptr;
    sa.er_w1 = g.w_r.weight[0]; sa.er_b1 = g.w_r.bias[0]; sa.er_w2 = g.w_r.weight[1]; sa.er_b2 = g.w_r.bias[1];
    sa.eh_w1 = g.w_h.weight[0]; sa.eh_b1 = g.w_h.bias[0]; sa.eh_w2 = g.w_h.weight[1]; sa.eh_b2 = g.w_h.bias[1];
    sa.off_er = sa.off_eh = 0;
    // (one node tile: measured slower than the f32 form -- 0.0615 vs 0.0496 ms per configs[1] step: too few MFMAs to pay for the splits)
    const bool split_ok = sp_image && scene_similarity_mode(g) == SIM_SOFTMAX && NT == 2 && g.num_layer <= 4;      // (mh == null: value rows)
    sa.bx = split_ok ? 1 : 0;
    sa.image = sp_image;
    sa.xh_rows = xh_rows; sa.x0_rows = x0_rows; sa.crowds_per = crowds_per;
    sa.wa = bilinear_wa(g);
    sa.sim = scene_similarity_mode(g);
    sa.layerwise = g.layerwise_graph;
    for (int l = 0; l < RGL_MAX_GCN_LAYERS; ++l) sa.Ws[l] = l < g.num_layer ? g.Ws[l] : nullptr;
    sa.L = g.num_layer; sa.skip = g.skip_connection;
    sa.wm1 = mh ? mh->weight[0] : nullptr; sa.bm1 = mh ? mh->bias[0] : nullptr;
    sa.wm2 = mh ? mh->weight[1] : nullptr; sa.bm2 = mh ? mh->bias[1] : nullptr;
    sa.humans_next = humans_next;
    sa.rows_out = rows_out;
    sa.P = P; sa.H = H; sa.N = N;
    int off = 0;
    auto take = [&](int nfl) { int o = off; off += (nfl + 3) & ~3; return o; };
    {   // the weight image: one layout for the LDS region and for its packed global copy
        const SceneImageLayout lo = scene_image_layout(g.num_layer, sa.bx != 0);
        sa.off_wa = lo.off_wa; sa.off_ws = lo.off_ws; sa.off_wm1 = lo.off_wm1; sa.off_bm1 = lo.off_bm1;
        sa.off_wm2 = lo.off_wm2; sa.off_bm2 = lo.off_bm2;
        sa.ws_stride = lo.ws_stride;
        sa.image_floats = lo.total;
        off = lo.total;
    }
    sa.wc1 = sa.bc1 = sa.wc2 = sa.bc2 = nullptr;
    sa.off_wc1 = sa.off_bc1 = sa.off_wc2 = 0;
    if (sa.sim == SIM_CONCAT) {
        sa.wc1 = g.w_a_mlp.weight[0]; sa.bc1 = g.w_a_mlp.bias[0]; sa.wc2 = g.w_a_mlp.weight[1]; sa.bc2 = g.w_a_mlp.bias[1];
        sa.off_wc1 = take(2 * XD * W1LD); sa.off_bc1 = take(HID); sa.off_wc2 = take(HID);
    }
    if (embed_inside) {
        sa.off_er = take(kRowMlpSetFloats);
        sa.off_eh = take(kRowMlpSetFloats);
    }
    sa.wave_stride = 16 * NT * XLD;
    // scene slots of a workgroup: the level prologue's, or the launcher's choice
    const bool prologue = slots > 0;
    if (slots <= 0) slots = scene_region_slots(NT, embed_inside);
    sa.off_wave = take(slots * sa.wave_stride);
    sa.off_rows = sa.chunk_crowds = 0;
    if (prologue) {      // the row buffer, behind everything else (prologue_scene_floats counts it so): as many crowds as the region holds
        const int room = (region_floats - off - kPrologueChunk * XD) / (H * XD);
        sa.chunk_crowds = room < kPrologueChunkCrowds ? room : kPrologueChunkCrowds;        // < 1: the caller refuses the form
        sa.off_rows = take(prologue_row_floats(H, sa.chunk_crowds > 0 ? sa.chunk_crowds : 1));
    }
    return off;
}

// embeddings (one launch) + one-wave-per-scene graph forward; mh != null: motion head -> humans_next; rows_out != null: value rows
// `plan` (rgl_plan_scene_forward): nothing is launched, the form of the launches is recorded
static int run_scene_kernels(const RglGraph& g, const RglMlp* mh, const float* robot, const float* humans, int crowds_per, int P,
                             int H, float* humans_next, float* rows_out, float* x0_rows, float* xh_rows,
                             const ChildrenArgs* ca, hipStream_t stream, const ChildrenArgs* embed_children = nullptr,
                             const float* sp_image = nullptr, ScenePlan* plan = nullptr) {
    const int N = H + 1, n_crowds = P / crowds_per;
    const int NT0 = scene_node_tiles(N);
    const bool embed_inside = scene_embeds_inside(g, NT0, P, embed_children != nullptr);
    if (!embed_inside) {
        if (plan) plan->embed_launch = 1;
        else {
            int rc = launch_row_mlp2_pair(g.w_r, robot, x0_rows, P, g.w_h, humans, xh_rows, n_crowds * H, stream, embed_children);
            if (rc) return rc;
        }
    }
    SceneArgs sa;
    const size_t lds_bytes = fill_scene_args(sa, g, mh, robot, humans, crowds_per, P, H, humans_next, rows_out, x0_rows, xh_rows,
                                             embed_inside, sp_image, 0) * sizeof(float);
    switch (NT0) {
        case 1: return launch_scene<1, 8>(sa, lds_bytes, ca, stream, plan);
        case 2: return launch_scene<2, 8>(sa, lds_bytes, ca, stream, plan);
        case 3: return launch_scene<3, 4>(sa, lds_bytes, ca, stream, plan);
        case 4: return launch_scene<4, 4>(sa, lds_bytes, ca, stream, plan);
        default: return launch_scene_wide(sa, lds_bytes, ca, stream, plan);
    }
}

// The rows of S scenes around run_scene_kernels, one Carver walk: the embeddings x0 [S][32] | xh [S / crowds_per][H][32] | rows [S][64],
// the value rows (with_rows: callers with a value head).  Null base: the size.  The embeddings are ONE take (one launch writes both):
// gcn_predict_f32's forward scratch is the rows' sum rounded up once, which holds one padding in front of `rows`, not two.
struct SceneRows { float *x0, *xh, *rows; size_t bytes; };
SceneRows carve_scene_rows(void* base, long long S, int crowds_per, int H, bool with_rows) {
    Carver c{(char*)base, 0};
    SceneRows w;
    w.x0 = c.take<float>((S + S / crowds_per * H) * XD * sizeof(float));
    w.xh = w.x0 ? w.x0 + S * XD : nullptr;
    w.rows = with_rows ? c.take<float>(S * 64 * sizeof(float)) : nullptr;
    w.bytes = (size_t)c.off;
    return w;
}

}  // namespace

namespace rgl {

// The three-piece bf16 weight image of the state predictor's scene kernel (RGL_CONTRACT_BF16X6): depends on the weights only.
// (graph + optional motion head: the state predictor's form; mh == null: the value-rows form of path G / the module forwards)
size_t scene_image_bytes_for(const RglGraph& g, const RglMlp* mh) {
    if (!scene_kernel_covers(g, 20) || scene_similarity_mode(g) != SIM_SOFTMAX) return 0;
    if (mh && !mlp_is(*mh, XD, HID, 5, false)) return 0;
    return (((size_t)scene_image_layout(g.num_layer, true).total * sizeof(float)) + 255) & ~(size_t)255;
}

size_t scene_image_bytes(const MprlPlanner* pl) {
    if (!pl || pl->linear_state_predictor) return 0;
    if (pl->contraction_dtype != RGL_CONTRACT_BF16X6) return 0;
    return scene_image_bytes_for(pl->predictor_graph, &pl->motion_head);
}

int pack_scene_image(const MprlPlanner* pl, float* image, hipStream_t stream) {
    if (!scene_image_bytes(pl)) return RGL_ERR_BAD_MODE;      // the caller asks scene_image_bytes first
    return pack_scene_image_for(pl->predictor_graph, &pl->motion_head, image, stream);
}

int pack_scene_image_for(const RglGraph& g, const RglMlp* mh, float* image, hipStream_t stream) {
    if (!scene_image_bytes_for(g, mh)) return RGL_ERR_BAD_MODE;      // the caller asks scene_image_bytes_for first
    SceneImageArgs ia;
    ia.wa = bilinear_wa(g);
    for (int l = 0; l < 4; ++l) ia.Ws[l] = l < g.num_layer ? g.Ws[l] : nullptr;
    ia.wm1 = mh ? mh->weight[0] : nullptr; ia.bm1 = mh ? mh->bias[0] : nullptr;
    ia.wm2 = mh ? mh->weight[1] : nullptr; ia.bm2 = mh ? mh->bias[1] : nullptr;
    ia.L = g.num_layer;
    ia.lo = scene_image_layout(g.num_layer, true);
    hipLaunchKernelGGL(scene_pack_b6_kernel, dim3((ia.lo.total + 255) / 256), dim3(256), 0, stream, ia, image);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

// The level prologue of the fused children kernel (rgl_fused_kernel.hip): the state predictor's scenes of the parents a workgroup owns in the
// unsplit BX + EMB form of scene_body (one slot per wave, embeddings inside), and the level's reward / next-state pairs.  false = outside
// that form's envelope: the six-term bf16 scene kernel with two node tiles (softmax similarity, 9-wide robot state, a motion head).
bool level_prologue_args(const MprlPlanner* pl, const ChildrenArgs& ca, float* humans_next, const float* sp_image, LevelPrologue* lp) {
    if (!sp_image || !level_prologue_layout(pl, ca.humans_per, ca.P, ca.H, nullptr, nullptr)) return false;
    lp->scene_floats = fill_scene_args(lp->scene, pl->predictor_graph, &pl->motion_head, ca.robot, ca.humans, ca.humans_per, ca.P, ca.H,
                                       humans_next, nullptr, nullptr, nullptr, true, sp_image, 8, fused_prologue_region_floats());
    if (!lp->scene.bx) return false;
    lp->children = ca;
    return true;
}

// The form check and the LDS layout of level_prologue_args without any array (host only; the planner export rgl_plan_prologue_embedding
// asks it too): true and the scene region's LDS floats / the crowds a chunk's row buffer holds, false = outside the form.
bool level_prologue_layout(const MprlPlanner* pl, int crowds_per, int P, int H, int* scene_floats, int* chunk_crowds) {
    if (pl->linear_state_predictor || pl->contraction_dtype != RGL_CONTRACT_BF16X6) return false;
    const RglGraph& g = pl->predictor_graph;
    const int N = H + 1;
    if (!scene_kernel_covers(g, N) || !mlp_is(pl->motion_head, XD, HID, 5, false) || g.w_r.dims[0] != 9) return false;
    if (scene_similarity_mode(g) != SIM_SOFTMAX || (N + 15) / 16 != 2 || crowds_per < 1 || P % crowds_per != 0) return false;
    SceneArgs sa;
    static const float image_stand_in = 0.f;      // fill_scene_args only asks whether there is an image
    const int fl = fill_scene_args(sa, g, &pl->motion_head, nullptr, nullptr, crowds_per, P, H, nullptr, nullptr, nullptr, nullptr, true,
                                   &image_stand_in, 8, fused_prologue_region_floats());
    if (!sa.bx || sa.chunk_crowds < 1) return false;
    if (scene_floats) *scene_floats = fl;
    if (chunk_crowds) *chunk_crowds = sa.chunk_crowds;
    return true;
}

size_t predict_humans_workspace_bytes(int P, int crowds_per, int H) { return carve_scene_rows(nullptr, P, crowds_per, H, false).bytes; }

// humans_next[s] = motion_head(RGL(robot[s], humans[s / crowds_per]))[1:]  for P scenes (StatePredictor.forward).
int launch_predict_humans(const MprlPlanner* pl, const ChildrenArgs& level, float* humans_next, void* workspace,
                          size_t workspace_bytes, hipStream_t stream, int* children_done, const float* sp_image) {
    const float *robot = level.robot, *humans = level.humans;
    const int crowds_per = level.humans_per, P = level.P, H = level.H;
    *children_done = 0;
    const RglGraph& g = pl->predictor_graph;
    const RglMlp& mh = pl->motion_head;
    const int N = H + 1;
    const bool ok = scene_kernel_covers(g, N) && mlp_is(mh, XD, HID, 5, false) && workspace && P % crowds_per == 0 &&
                    workspace_bytes >= predict_humans_workspace_bytes(P, crowds_per, H);
    if (!ok) {
        // outside the shipped shapes: the tile kernels (rgl_tile_pipeline.hip) where they cover the model, else the general kernel
        if (P % crowds_per == 0) {
            bool taken = false;
            const int rc = launch_tiles_forward(&g, nullptr, &mh, robot, humans, P, crowds_per, H, nullptr, nullptr, humans_next, workspace,
                                                workspace_bytes, stream, &taken);
            if (rc || taken) return rc;
        }
        if (require_mfma_forward()) return RGL_ERR_BAD_MODE;
        return launch_generic_forward(&g, nullptr, &mh, robot, humans, P, crowds_per, H, nullptr, nullptr, nullptr,
                                      humans_next, stream);
    }
    const SceneRows w = carve_scene_rows(workspace, P, crowds_per, H, false);
    // the level's reward / next-state work rides in the scene kernel's launch while the scene workgroups leave LDS free (few scenes),
    // in the embedding launch otherwise: never a launch of its own on this path
    const int children_in_scene_below = scene_children_below(pl->contraction_dtype == RGL_CONTRACT_BF16X6);
    const ChildrenArgs* in_scene = P < children_in_scene_below ? &level : nullptr;
    const ChildrenArgs* in_embed = in_scene ? nullptr : &level;
    const int rc = run_scene_kernels(g, &mh, robot, humans, crowds_per, P, H, humans_next, nullptr, w.x0, w.xh, in_scene, stream,
                                     in_embed, pl->contraction_dtype == RGL_CONTRACT_BF16X6 ? sp_image : nullptr);
    if (rc == RGL_OK) *children_done = 1;
    return rc;
}

// Module forwards (ValueEstimator.forward / StatePredictor.forward on a batch: value_estimator.py:11-20, state_predictor.py:20-39)
// through the same kernels: embeddings + one wave per scene; values via the value-rows mode + robot_head_kernel.
// workspace: carve_scene_rows, the value rows for a value head only.
static bool scene_forward_form(const RglGraph& g, const RglMlp* vh, const RglMlp* mh, int S, int crowds_per, int H) {
    const bool has_v = vh && vh->n_layers > 0, has_m = mh && mh->n_layers > 0;
    if (!(has_v || has_m) || crowds_per < 1 || S % crowds_per != 0) return false;
    if (!scene_kernel_covers(g, H + 1)) return false;
    if (has_v && head_variant(*vh) < 0) return false;
    if (has_m && !mlp_is(*mh, XD, HID, 5, false)) return false;
    return true;
}

size_t scene_forward_workspace_bytes(const RglGraph* g, const RglMlp* vh, const RglMlp* mh, int S, int crowds_per, int H) {
    if (!g || !scene_forward_form(*g, vh, mh, S, crowds_per, H)) return 0;
    return carve_scene_rows(nullptr, S, crowds_per, H, vh && vh->n_layers > 0).bytes;
}

bool scene_forward_covers(const RglGraph* g, const RglMlp* vh, const RglMlp* mh, int S, int crowds_per, int H, size_t workspace_bytes) {
    const size_t need = scene_forward_workspace_bytes(g, vh, mh, S, crowds_per, H);
    return need && workspace_bytes >= need;
}

int launch_scene_forward(const RglGraph* g, const RglMlp* vh, const RglMlp* mh, const float* robot, const float* humans, int S,
                         int crowds_per, int H, float* value_out, float* humans_next, void* workspace, size_t workspace_bytes,
                         hipStream_t stream, const float* value_rows_image) {
    if (!workspace || !scene_forward_covers(g, vh, mh, S, crowds_per, H, workspace_bytes)) return RGL_ERR_BAD_MODE;
    const bool has_v = vh && vh->n_layers > 0, has_m = mh && mh->n_layers > 0;
    const SceneRows w = carve_scene_rows(workspace, S, crowds_per, H, has_v);
    if (has_m) {
        int rc = run_scene_kernels(*g, mh, robot, humans, crowds_per, S, H, humans_next, nullptr, w.x0, w.xh, nullptr, stream);
        if (rc) return rc;
    }
    if (has_v) {
        int rc = run_scene_kernels(*g, nullptr, robot, humans, crowds_per, S, H, nullptr, w.rows, w.x0, w.xh, nullptr, stream, nullptr,
                                   value_rows_image);
        if (rc) return rc;
        return launch_head_rows(g, vh, w.rows, S, value_out, stream);
    }
    return RGL_OK;
}

// Value of the children through the one-wave-per-scene kernel: every child's graph in full (no crowd sharing), any of the
// similarity functions it implements, layerwise graphs, 1..4 layers -- the MFMA path of everything the shared-crowd kernels do
// not cover (cosine / cosine_softmax scale the columns by child-dependent norms; layerwise graphs rebuild the adjacency from
// every H_l).  Its region: carve_scene_rows of the P A children, the A of a parent sharing its crowd's rows.
size_t scene_children_workspace_bytes(int P, int A, int H) { return carve_scene_rows(nullptr, (long long)P * A, A, H, true).bytes; }

bool scene_children_covers(const MprlPlanner* pl, int H) {
    return scene_kernel_covers(pl->value_graph, H + 1) && head_variant(pl->value_head) >= 0;
}

int launch_scene_children(const MprlPlanner* pl, const ChildrenCall& c, void* region, size_t region_bytes) {
    const RglGraph& g = pl->value_graph;
    const int P = c.P, A = c.A, H = c.H;
    const SceneRows w = carve_scene_rows(region, (long long)P * A, A, H, true);
    if (!scene_children_covers(pl, H) || !region || region_bytes < w.bytes) return RGL_ERR_BAD_MODE;
    int rc = run_scene_kernels(g, nullptr, c.child_robot, c.humans_next, A, P * A, H, nullptr, w.rows, w.x0, w.xh, nullptr, c.stream);
    if (rc) return rc;
    return launch_head_rows(&g, &pl->value_head, w.rows, P * A, c.child_value, c.stream);
}

}  // namespace rgl

// What rgl_graph_forward_f32 (values / next humans with a workspace), launch_predict_humans, launch_scene_children and path G's value
// rows do once they reach run_scene_kernels: the same functions, with a ScenePlan in place of the launches.
extern "C" int rgl_plan_scene_forward(const RglGraph* graph, int motion_head, int n_scenes, int scenes_per_crowd, int H,
                                      int image_at_hand, int reward_offered, RglSceneForwardPlan* plan) {
    if (!graph || !plan) return RGL_ERR_NULL;
    if (n_scenes < 1 || scenes_per_crowd < 1 || H < 1 || H + 1 > RGL_MAX_NODES || n_scenes % scenes_per_crowd != 0) return RGL_ERR_BAD_SHAPE;
    *plan = RglSceneForwardPlan{};
    const RglGraph& g = *graph;
    const int N = H + 1;
    if (!scene_kernel_covers(g, N)) return RGL_OK;
    // stand-ins: the launchers ask only WHETHER there are rows to embed, an image, a motion head, reward work (nothing is read)
    static const float rows_stand_in = 0.f;
    static const RglMlp head_stand_in{};
    static const ChildrenArgs reward_stand_in{};
    const bool b6 = image_at_hand != 0;
    const ChildrenArgs* in_scene = reward_offered && n_scenes < scene_children_below(b6) ? &reward_stand_in : nullptr;
    const ChildrenArgs* in_embed = reward_offered && !in_scene ? &reward_stand_in : nullptr;
    ScenePlan sp{};
    const int rc = run_scene_kernels(g, motion_head ? &head_stand_in : nullptr, &rows_stand_in, &rows_stand_in, scenes_per_crowd, n_scenes, H,
                                     nullptr, nullptr, nullptr, nullptr, in_scene, nullptr, in_embed, b6 ? &rows_stand_in : nullptr, &sp);
    if (rc) return RGL_OK;                  // (concatenation beyond 64 nodes never gets here: scene_kernel_covers)
    plan->covered = 1;
    plan->node_tiles = sp.node_tiles; plan->family = sp.family; plan->waves = sp.waves; plan->split = sp.split;
    plan->embed_inside = sp.embed_inside; plan->bx = sp.bx; plan->slots = sp.slots; plan->grid = sp.grid; plan->grid_cap = sp.grid_cap;
    const int steps = scene_last_steps(N, sp.node_tiles, sp.family);
    plan->last_steps = steps > 0 ? steps : 0;
    plan->children_riding = sp.children_riding; plan->embed_launch = sp.embed_launch;
    plan->lds_bytes = sp.lds_bytes;
    return RGL_OK;
}
