// rgl_scene_body.h -- the state predictor's scene graph forward (one scene per wave, or NT waves per scene) as a device function over
// a range of scenes and an LDS base: the body of scene_graph_kernel (rgl_scene.hip) and of the level prologue of
// children_fused_kernel (rgl_fused_kernel.hip), which run the same code on the same inputs and so write the same bits.
// Follows (reference paths): crowd_nav/policy/state_predictor.py:20-39, graph_model.py:99-130.
#pragma once
#include "rgl_children.h"
#include "rgl_mlp_chain.h"

using rgl::LevelPrologue;      // rgl_search_args.h
using rgl::SceneArgs;

namespace {

constexpr int M2LD = 20;   // LDS row stride of the [64][5 -> 16] motion output layer (4*M2LD % 32 == 16)

// The level prologue embeds the rows of the parents a workgroup owns in chunks (scene_body's WGE form): at most kPrologueChunk parents
// (ONE w_r tile of robot rows) that use at most `max_crowds` distinct crowds -- kPrologueChunkCrowds, or fewer where a predictor of
// three or four layers leaves less LDS behind its image (fill_scene_args).  16 sibling-sharing parents (crowds_per >= 2) span at
// most 9 crowds; at the root level (crowds_per = 1) the crowd bound cuts a chunk to 12 parents -- 16 crowds of 19 humans would be
// 41 KB of rows, and 32 592 B lie free behind the scene region of a two-layer predictor (rgl_fused_kernel.hip proves the fit).
constexpr int kPrologueChunk = 16, kPrologueChunkCrowds = 12;
// parents [c0, prologue_chunk_end) form the chunk that starts at c0: its crowds c0 / crowds_per .. (end - 1) / crowds_per
__host__ __device__ inline int prologue_chunk_end(int c0, int end, int crowds_per, int max_crowds) {
    int c1 = c0 + kPrologueChunk;
    const int by_crowds = (c0 / crowds_per + max_crowds) * crowds_per;      // the first parent of one crowd too many
    if (by_crowds < c1) c1 = by_crowds;
    return c1 < end ? c1 : end;
}
constexpr int prologue_row_floats(int H, int max_crowds) { return (max_crowds * H + kPrologueChunk) * XD; }

// ---- weight image of the scene kernel: one layout for the LDS region and (BX) for its packed global copy ---------------------------
struct SceneImageLayout { int off_wa, off_ws, off_wm1, off_bm1, off_wm2, off_bm2, total, ws_stride; };
// bx: the matrices as three-piece bf16 fragments (layer_mfma_b6: 6 bytes per weight) instead of k-major f32 rows
constexpr SceneImageLayout scene_image_layout(int L, bool bx = false) {
    SceneImageLayout o{};
    int off = 0;
    auto take = [&](int nfl) { int r = off; off += (nfl + 3) & ~3; return r; };      // (a constexpr lambda: C++17)
    o.ws_stride = bx ? B6Floats<XD, XD>::v : XD * WLD;
    o.off_wa = take(bx ? B6Floats<XD, XD>::v : XD * WLD);
    o.off_ws = take(L * o.ws_stride);
    o.off_wm1 = take(bx ? B6Floats<XD, HID>::v : XD * W1LD);
    o.off_bm1 = take(HID);
    o.off_wm2 = take(bx ? B6Floats<HID, 16>::v : HID * M2LD);
    o.off_bm2 = take(16);
    o.total = off;
    return o;
}

// k steps of A H over the LAST node tile that reach a valid node (PERM in scene_body): ceil(valid / 4) of its four; all four for the
// concatenation family (SK 3: no node permutation); <= 0 where the eight-tile form's last tile is padding only (N <= 112)
__host__ __device__ constexpr int scene_last_steps(int N, int NT, int SK) { return SK != 3 ? (N - 16 * (NT - 1) + 3) >> 2 : 4; }

constexpr int kRowMlpSetFloats = 4 * 1 * 4 * 64 + 2 * 4 * 4 * 64 + HID + XD;
// LDS floats of the level prologue's scene region for an L-layer predictor and crowds of H humans (17..20 nodes): the BX image, the
// two embedding sets, 8 wave slots of two node tiles, the row buffer -- what fill_scene_args lays out (level_prologue_args checks it)
constexpr int prologue_scene_floats(int L, int H) {
    return scene_image_layout(L, true).total + 2 * kRowMlpSetFloats + 8 * 32 * XLD + prologue_row_floats(H, kPrologueChunkCrowds);
}

// Phase marks of the level prologue (-DRGL_PHASE_TIMING, tools/phase_timing.py prologue): per-wave s_memtime deltas of 0 = image and
// fragment loads up to the first barrier, 1 = embeddings (and the fill of the wave's node rows), 2 = scene graph, 3 = reward and
// next-state pairs, 4 = waits at the chunk barriers and the closing barrier.  A mark costs ~400 cycles.
#ifdef RGL_PHASE_TIMING
struct ProPhases { unsigned long long acc[5] = {0, 0, 0, 0, 0}, t0 = 0; };
#define PRO_PHASE_START(pp) do { if (pp) (pp)->t0 = __builtin_amdgcn_s_memtime(); } while (0)
#define PRO_PHASE_MARK(pp, idx)                                            \
    do {                                                                   \
        if (pp) {                                                          \
            const unsigned long long now__ = __builtin_amdgcn_s_memtime(); \
            (pp)->acc[idx] += now__ - (pp)->t0;                            \
            (pp)->t0 = now__;                                              \
        }                                                                  \
    } while (0)
#define PRO_PHASE_FLUSH(pp)                                                \
    do {                                                                   \
        if ((threadIdx.x & 63) == 0)                                       \
            for (int i__ = 0; i__ < 5; ++i__) atomicAdd(&g_phase_cycles[10 + i__], (pp)->acc[i__]); \
    } while (0)
#else
struct ProPhases {};
#define PRO_PHASE_START(pp) do { } while (0)
#define PRO_PHASE_MARK(pp, idx) do { } while (0)
#define PRO_PHASE_FLUSH(pp) do { (void)(pp); } while (0)
#endif

// One 16-row tile of a two-layer embedding MLP (IN -> 64 -> 32, ReLU after both; fragment set `lds_set`: fill_frags / frag_store
// layout) as an MFMA chain: lane (n, q) feeds the features of row `src` and gets outputs 4 q .. 4 q + 3 and 16 + 4 q .. of that row.
// Every output column depends on its own input column and the weights only: where a row sits in which tile does not alter its bits.
template <int IN>
__device__ __forceinline__ void row_mlp2_tile(const float* lds_set, const float* src, int lane, f32x4 (&o)[2]) {
    constexpr int F1 = 0, F2 = F1 + 4 * 1 * 4 * 64, B1 = F2 + 2 * 4 * 4 * 64, B2 = B1 + HID;
    const int q = lane >> 4;
    f32x4 in[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int feat = tile_feature<IN>(0, q, r);
        in[0][r] = feat < IN ? src[feat] : 0.f;
    }
    f32x4 h[4];
    layer_mfma<IN, HID, true>(lds_set + F1, in, h, lane, lds_set + B1);
    relu_tiles<HID>(h);
    layer_mfma<HID, XD, true>(lds_set + F2, h, o, lane, lds_set + B2);
    relu_tiles<XD>(o);
}

// N <= 32: 8 waves share one 30 KB weight image, two workgroups per CU = 4 waves per SIMD (round 1 ran 4-wave workgroups, 2 waves
// per SIMD: a scene is one serial chain of ~290 MFMAs with a softmax in the middle, and two waves did not cover its latencies).
// Larger crowds (3-4 column tiles: 200+ VGPRs, 9 KB of node features per wave) keep 4-wave workgroups, two per CU.

// One scene per wave.  CH = true: the level's independent next-robot-state / reward work (float64 VALU) rides in this launch on
// EXTRA workgroups [grid_scene, gridDim.x).  That pays while the scene workgroups leave LDS free (few scenes: the two halves
// overlap and a launch is saved); with many scenes the extra workgroups -- which reserve the same dynamic LDS -- only start when
// a scene workgroup retires, and the second code path costs the kernel a third of its occupancy in registers: the launcher then
// uses CH = false and the caller launches mprl_children_kernel (measured cross-over ~3 k scenes; an in-wave variant, lanes =
// actions with scalar crowd loads, was tried and was never better).
// SK: 0 = softmax of S (embedded_gaussian / gaussian), 1 = plain weights over their row sum (squared / equal_attention /
// diagonal), 2 = cosine family (cosine / cosine_softmax; graph_model.py:70-79), 3 = concatenation (pair MLP, :80-85)
// SPLIT: the NT column tiles of a scene go to NT waves (WAVES / NT scenes per workgroup pass, node features shared in LDS,
// workgroup barriers where a phase needs every row): a scene is one serial chain of ~70 MFMAs per column tile with a softmax in
// the middle, and with few scenes (the upper tree levels, dense crowds: 256-512 scenes of 50 agents on 256 CUs) nothing else hides
// that chain.  With thousands of scenes the unsplit form -- no barriers, the same MFMA count -- is as fast or faster.
// EMB: the wave computes the embeddings of its node tiles itself (w_r on the robot row, w_h on the human rows: the MFMA chains of
// row_mlp2_tiles) instead of reading rows a separate launch prepared -- with few scenes that launch is ~5 us of latency for ~1 us
// of work (and a round trip through HBM); sibling scenes repeat their crowd's human embeddings, which only matters when the
// kernel is throughput-bound (many scenes: the launcher keeps the two-launch form there).
// BX (RGL_CONTRACT_BF16X6, softmax similarity): the WEIGHT products as six bf16 MFMA terms over three-piece operands (layer_mfma_b6).
// WGE (with EMB; the level prologue): the WORKGROUP embeds the rows of its scenes, a chunk of them at a time (prologue_chunk_end),
// into the LDS row buffer at off_rows -- the human rows of the chunk's distinct crowds once per crowd, packed densely into 16-row
// tiles across crowd boundaries, and the chunk's robot rows as one w_r tile, the tiles dealt over the waves (row_mlp2_tile: the
// chain of row_mlp2_tiles) -- and behind a barrier every wave fills its slot from that buffer as the rows-from-global form does
// from x0_rows / xh_rows.  Against EMB alone: sibling scenes no longer repeat their crowd's rows and no tile is mostly padding
// (configs[2], 16 parents of 8 crowds per workgroup: 11 tile passes instead of 48).
// Scenes first, first + slot_step, ... (see the loop below) up to `end`, on the 64 * WAVES threads of the workgroup; `lds`: the base
// of the region the SceneArgs offsets point into (its image is loaded here, behind a workgroup barrier).
template <int NT, int SK, int WAVES, bool SPLIT, bool EMB = false, bool BX = false, bool WGE = false>
__device__ __forceinline__ void scene_body(const SceneArgs& a, float* lds, int first, int slot_step, int pass_step, int end,
                                           ProPhases* pp = nullptr) {
    static_assert(!BX || SK == 0, "six-term bf16 products: softmax similarity");
    static_assert(!WGE || (EMB && !SPLIT), "workgroup-cooperative embeddings: the embedding sets in LDS, one scene per wave");
    static_assert(!SPLIT || (SK != 3 && NT > 1 && WAVES % NT == 0), "split scenes: whole scenes per workgroup, no pair-MLP similarity");
    constexpr int kSceneThreads = WAVES * 64;
    constexpr int NCT = SPLIT ? 1 : NT;                     // column tiles of a scene this wave owns
    const int sim = SK == 0 ? (int)SIM_SOFTMAX : a.sim;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    const int N = a.N, H = a.H;
    const float* wa = lds + a.off_wa;       // [32][WLD]
    const float* ws = lds + a.off_ws;       // [L][32][WLD]
    const float* wm1 = lds + a.off_wm1;     // [32][W1LD]
    const float* bm1 = lds + a.off_bm1;     // [64]
    const float* wm2 = lds + a.off_wm2;     // [64][M2LD], columns >= 5 zero
    const float* bm2 = lds + a.off_bm2;     // [16], entries >= 5 zero
    const int slot = __builtin_amdgcn_readfirstlane(SPLIT ? wave / NT : wave);
    const int ctb = SPLIT ? __builtin_amdgcn_readfirstlane(wave % NT) : 0;      // my first (SPLIT: only) column tile
    float* Hs = lds + a.off_wave + slot * a.wave_stride;   // [16*NT][XLD] node features of the slot's current scene
    // EMB: the fragment sets of the two embedding MLPs.  Their loads go out together with the weight image's (f32 image: before its
    // stores), so that the whole prologue is ONE L2 round trip instead of one per fill (round 4)
    constexpr int kEmbThreads = EMB ? kSceneThreads : 64;
    FragRegs<9, HID, kEmbThreads> er1;
    FragRegs<HID, XD, kEmbThreads> er2, eh2;
    FragRegs<5, HID, kEmbThreads> eh1;
    float ebias[4] = {0.f, 0.f, 0.f, 0.f};
    auto emb_loads = [&]() {
        if constexpr (EMB) {
            frag_load(er1, a.er_w1, tid);
            frag_load(er2, a.er_w2, tid);
            frag_load(eh1, a.eh_w1, tid);
            frag_load(eh2, a.eh_w2, tid);
            ebias[0] = bias_load<HID>(a.er_b1, tid);
            ebias[1] = bias_load<XD>(a.er_b2, tid);
            ebias[2] = bias_load<HID>(a.eh_b1, tid);
            ebias[3] = bias_load<XD>(a.eh_b2, tid);
        }
    };
    if constexpr (BX) {
        // three-piece bf16 image, packed once per parameter state (or per search) in exactly this layout: b128 copies, every
        // load of a thread in flight at once.  (Converting the matrices here -- two L2 round trips per fragment element -- cost 10 us per launch.)
        // (round 6: LDS-direct loads, every chunk of a wave in flight at once.  The b128 copy loop this replaces compiled to load -> wait
        // -> store per iteration: 19 dependent L2 round trips, ~2.5 us of every launch.)
        constexpr int kChunk = 256;                                            // floats per wave and instruction
        const int n_chunks = (a.image_floats + kChunk - 1) / kChunk;
        for (int c = wave; c < n_chunks; c += WAVES) {
            const int fl = c * kChunk + lane * 4;
            if (fl < a.image_floats)                                           // the last chunk is partial (image_floats % 4 == 0)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.image + fl),
                                                 (__attribute__((address_space(3))) void*)(lds + c * kChunk), 16, 0, 0);
        }
        wait_vmcnt0();                                                         // my chunks have landed (the barrier below: everyone's)
    } else
    {   // weight image in two phases -- every global load of the thread first, then the LDS stores -- so that the whole
        // 30 KB image costs ONE L2 round trip (filling matrix by matrix cost one per matrix: ~9 us of a ~35 us launch)
        float* w = lds;
        constexpr int NT_ = kSceneThreads;
        constexpr int KQ = XD * XD / NT_, KM1 = XD * HID / NT_, KM2 = HID * 16 / NT_;
        float vq[5][KQ];                                       // wa + up to 4 layer matrices
        float vm1[KM1], vm2[KM2], vb;
        const int Lc = a.L < 4 ? a.L : 4;
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const int i = tid + k * NT_;
            vq[0][k] = a.wa ? a.wa[i] : ((i / XD) == (i % XD) ? 1.f : 0.f);      // gaussian: Wa = I
#pragma unroll
            for (int l = 0; l < 4; ++l) vq[1 + l][k] = l < Lc ? a.Ws[l][i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < KM1; ++k) vm1[k] = a.wm1 ? a.wm1[tid + k * NT_] : 0.f;        // value mode: no motion head
#pragma unroll
        for (int k = 0; k < KM2; ++k) {
            const int i = tid + k * NT_, r = i / 16, c = i - r * 16;
            vm2[k] = a.wm2 ? a.wm2[r * 5 + (c < 5 ? c : 0)] : 0.f;
        }
        vb = !a.bm1 ? 0.f : (tid < HID ? a.bm1[tid] : (tid < HID + 5 ? a.bm2[tid - HID] : 0.f));
        emb_loads();
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const int i = tid + k * NT_, r = i / XD, c = i - r * XD;
            w[a.off_wa + r * WLD + c] = vq[0][k];
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (l < Lc) w[a.off_ws + (l * XD + r) * WLD + c] = vq[1 + l][k];
        }
#pragma unroll
        for (int k = 0; k < KM1; ++k) {
            const int i = tid + k * NT_, r = i / HID, c = i - r * HID;
            w[a.off_wm1 + r * W1LD + c] = vm1[k];
        }
#pragma unroll
        for (int k = 0; k < KM2; ++k) {
            const int i = tid + k * NT_, r = i / 16, c = i - r * 16;
            w[a.off_wm2 + r * M2LD + c] = c < 5 ? vm2[k] : 0.f;
        }
        if (tid < HID) w[a.off_bm1 + tid] = vb;
        else if (tid < HID + 16) w[a.off_bm2 + tid - HID] = tid < HID + 5 ? vb : 0.f;
        if (SK == 3) {
            fill_matrix<2 * XD, 2 * XD, HID, W1LD, kSceneThreads>(w + a.off_wc1, a.wc1, tid);
            for (int i = tid; i < HID; i += kSceneThreads) { w[a.off_bc1 + i] = a.bc1[i]; w[a.off_wc2 + i] = a.wc2[i]; }
        }
    }
    if constexpr (EMB) {
        float* w = lds;
        constexpr int F1 = 0, F2 = F1 + 4 * 1 * 4 * 64, B1 = F2 + 2 * 4 * 4 * 64, B2 = B1 + HID;
        if constexpr (BX) emb_loads();
        frag_store(er1, w + a.off_er + F1, tid);
        frag_store(er2, w + a.off_er + F2, tid);
        bias_store<HID>(ebias[0], w + a.off_er + B1, tid);
        bias_store<XD>(ebias[1], w + a.off_er + B2, tid);
        frag_store(eh1, w + a.off_eh + F1, tid);
        frag_store(eh2, w + a.off_eh + F2, tid);
        bias_store<HID>(ebias[2], w + a.off_eh + B1, tid);
        bias_store<XD>(ebias[3], w + a.off_eh + B2, tid);
    }
    __syncthreads();
    PRO_PHASE_MARK(pp, 0);
    // WGE: chunks [c0, c1) of the scenes first .. end - 1 (slot_step 1: the workgroup's own parents); otherwise one pass over all
    if (WGE && first >= end) return;                       // (workgroup-uniform; a workgroup of the prologue owns at least one parent)
    int c0 = first;
    do {
    const int c1 = WGE ? prologue_chunk_end(c0, end, a.crowds_per, a.chunk_crowds) : end;
    const int cr0 = WGE ? c0 / a.crowds_per : 0;            // the chunk's first crowd
    const int robot_rows0 = WGE ? a.off_rows + a.chunk_crowds * H * XD : 0;      // the robot rows' place in the row buffer
    if constexpr (WGE) {
        if (c0 != first) {
            __syncthreads();                               // every wave has filled its slot from the previous chunk's rows
            PRO_PHASE_MARK(pp, 4);
        }
        const int hrows = ((c1 - 1) / a.crowds_per - cr0 + 1) * H, htiles = (hrows + 15) >> 4;
        for (int t = wave; t <= htiles; t += WAVES) {      // human tiles 0 .. htiles - 1, then the robot tile
            f32x4 o[2];
            int dst;
            bool valid;
            if (t < htiles) {
                const int row = 16 * t + n;
                valid = row < hrows;
                row_mlp2_tile<5>(lds + a.off_eh, a.human_rows + ((size_t)cr0 * H + (valid ? row : hrows - 1)) * 5, lane, o);
                dst = a.off_rows + row * XD;
            } else {
                valid = n < c1 - c0;
                row_mlp2_tile<9>(lds + a.off_er, a.robot_rows + (size_t)(valid ? c0 + n : c1 - 1) * 9, lane, o);
                dst = robot_rows0 + n * XD;
            }
            if (valid) {
                *reinterpret_cast<f32x4*>(&lds[dst + 4 * q]) = o[0];
                *reinterpret_cast<f32x4*>(&lds[dst + 16 + 4 * q]) = o[1];
            }
        }
        PRO_PHASE_MARK(pp, 1);
        __syncthreads();                                   // the chunk's rows are in place
        PRO_PHASE_MARK(pp, 4);
    }
    // scene of slot k in pass i: c0 + slot_step * k + i * pass_step, below c1.  SPLIT: the loop is uniform over the workgroup
    // (barriers inside); a slot past the end recomputes the last scene and writes nothing.
    for (int it = c0 + (SPLIT ? 0 : slot_step * slot); it < c1; it += pass_step) {
        const int sc_raw = SPLIT ? it + slot_step * slot : it;
        const bool active = sc_raw < c1;
        const int sc = active ? sc_raw : c1 - 1;
        // node features of this scene: row 0 = robot, rows 1..H = its crowd, rows >= N zero
        if constexpr (EMB && !WGE) {
            constexpr int F1 = 0, F2 = F1 + 4 * 1 * 4 * 64, B1 = F2 + 2 * 4 * 4 * 64, B2 = B1 + HID;
            const float* er = lds + a.off_er;
            const float* eh = lds + a.off_eh;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int node = 16 * (ct + ctb) + n;
                const bool human = node >= 1 && node < N;
                const float* hsrc = a.human_rows + ((size_t)(sc / a.crowds_per) * H + (human ? node - 1 : 0)) * 5;
                f32x4 in[1];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int feat = tile_feature<5>(0, q, r);
                    in[0][r] = (human && feat < 5) ? hsrc[feat] : 0.f;
                }
                f32x4 hh[4], oh[2];
                layer_mfma<5, HID, true>(eh + F1, in, hh, lane, eh + B1);
                relu_tiles<HID>(hh);
                layer_mfma<HID, XD, true>(eh + F2, hh, oh, lane, eh + B2);
                relu_tiles<XD>(oh);
                if (ct + ctb == 0) {                              // the tile that holds the robot: its row through w_r
                    const float* rsrc = a.robot_rows + (size_t)sc * 9;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int feat = tile_feature<9>(0, q, r);
                        in[0][r] = (n == 0 && feat < 9) ? rsrc[feat] : 0.f;
                    }
                    f32x4 orr[2];
                    layer_mfma<9, HID, true>(er + F1, in, hh, lane, er + B1);
                    relu_tiles<HID>(hh);
                    layer_mfma<HID, XD, true>(er + F2, hh, orr, lane, er + B2);
                    relu_tiles<XD>(orr);
                    if (n == 0) { oh[0] = orr[0]; oh[1] = orr[1]; }
                }
#pragma unroll
                for (int ot = 0; ot < 2; ++ot)
                    *reinterpret_cast<f32x4*>(&Hs[node * XLD + 16 * ot + 4 * q]) = node < N ? oh[ot] : zero4();
            }
            __builtin_amdgcn_wave_barrier();
        } else if constexpr (WGE) {
        const int xr = robot_rows0 + (sc - c0) * XD;            // base indices into the row buffer
        const int xh = a.off_rows + (sc / a.crowds_per - cr0) * H * XD;
        for (int idx = lane; idx < 16 * NCT * (XD / 4); idx += 64) {
            const int row = (idx >> 3) + 16 * ctb, c4 = (idx & 7) * 4;
            f32x4 val = zero4();
            if (row == 0) val = *reinterpret_cast<const f32x4*>(&lds[xr + c4]);
            else if (row < N) val = *reinterpret_cast<const f32x4*>(&lds[xh + (row - 1) * XD + c4]);
            *reinterpret_cast<f32x4*>(&Hs[row * XLD + c4]) = val;
        }
        __builtin_amdgcn_wave_barrier();
        } else {
        const float* xr = a.x0_rows + (size_t)sc * XD;
        const float* xh = a.xh_rows + (size_t)(sc / a.crowds_per) * H * XD;
        for (int idx = lane; idx < 16 * NCT * (XD / 4); idx += 64) {
            const int row = (idx >> 3) + 16 * ctb, c4 = (idx & 7) * 4;
            f32x4 val = zero4();
            if (row == 0) val = *reinterpret_cast<const f32x4*>(xr + c4);
            else if (row < N) val = *reinterpret_cast<const f32x4*>(xh + (size_t)(row - 1) * XD + c4);
            *reinterpret_cast<f32x4*>(&Hs[row * XLD + c4]) = val;
        }
        }
        PRO_PHASE_MARK(pp, 1);
        if (SPLIT) __syncthreads();
        // adjacency of the node features currently in Hs, transposed and in B-operand order: pr[ct][jt][r] = A[i][j] for
        // column i = 16 ct + n, j = 16 jt + 4 q + r.  Once per scene, or once per layer for layerwise graphs.
        // Node order inside the LAST 16-node tile (PERM: every similarity but concatenation): D row 4q + r of an S^T tile holds node
        // 16 jt + 4 r + q instead of 16 jt + 4 q + r, so that as the k index of A*H the valid nodes of a partial tile sit in its first
        // ceil(valid / 4) k steps and the steps over padding nodes are skipped (N = 20: 5 of 8 steps per layer, N = 5: 2 of 4).
        constexpr bool PERM = SK != 3;
        auto jnode = [&](int jt, int r) { return 16 * jt + ((PERM && jt == NT - 1) ? 4 * r + q : 4 * q + r); };
        const int last_steps = scene_last_steps(N, NT, SK);
        f32x4 pr[NT][NT];
        auto adjacency = [&]() {
            if constexpr (SK == 3) {
                // concatenation: A_ij = relu(w2 . relu(W1a x_i + W1b x_j + b1) + b2).  P^T = W1a^T X^T and Q^T = W1b^T X^T by MFMA
                // (lane (n, q) of column tile ct holds hidden units 16 ht + 4 q + r of node 16 ct + n); the pair sum over the 64
                // hidden units: Q_j of the same q-group arrives as a DPP row_newbcast operand, the four q-groups add up at the end.
                const float* wc1 = lds + a.off_wc1;      // [64][W1LD]: rows 0..31 act on x_i, rows 32..63 on x_j
                const float* bc1 = lds + a.off_bc1;
                const float* wc2 = lds + a.off_wc2;
                const float bc2 = a.bc2[0];
                f32x4 pt[NT][4], qt[NT][4];
#pragma unroll
                for (int ct = 0; ct < NT; ++ct) {
#pragma unroll
                    for (int ht = 0; ht < 4; ++ht) {
                        pt[ct][ht] = *reinterpret_cast<const f32x4*>(&bc1[16 * ht + 4 * q]);      // P carries b1
                        qt[ct][ht] = zero4();
                    }
#pragma unroll
                    for (int ft = 0; ft < 2; ++ft) {
                        load_fence();
                        const f32x4 xb = *reinterpret_cast<const f32x4*>(&Hs[(16 * ct + n) * XLD + 16 * ft + 4 * q]);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int ht = 0; ht < 4; ++ht) {
                                pt[ct][ht] = mfma4(wc1[(16 * ft + 4 * q + r) * W1LD + 16 * ht + n], xb[r], pt[ct][ht]);
                                qt[ct][ht] = mfma4(wc1[(XD + 16 * ft + 4 * q + r) * W1LD + 16 * ht + n], xb[r], qt[ct][ht]);
                            }
                    }
                }
                f32x4 w2h[4];
#pragma unroll
                for (int ht = 0; ht < 4; ++ht) w2h[ht] = *reinterpret_cast<const f32x4*>(&wc2[16 * ht + 4 * q]);
#pragma unroll
                for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                    for (int jt = 0; jt < NT; ++jt) {
                        f32x4 res = zero4();
                        static_for<0, 16>([&](auto jc) {
                            constexpr int jl = decltype(jc)::value;
                            float acc = 0.f;
#pragma unroll
                            for (int ht = 0; ht < 4; ++ht)
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    acc = fmaf(fmaxf(dpp_rowbcast_add<jl>(qt[jt][ht][r], pt[ct][ht][r]), 0.f), w2h[ht][r], acc);
                            acc = fmaxf(kgroups_sum(acc) + bc2, 0.f);
                            const int j = 16 * jt + jl;
                            if (j >= N || 16 * ct + n >= N) acc = 0.f;
                            if ((jl >> 2) == q) res[jl & 3] = acc;
                        });
                        pr[ct][jt] = res;
                    }
                return;
            }
            // G^T = Wa^T X^T   (per column tile: [g = 16gt+4q+r][col n])
            f32x4 gt_[NT][2];
            {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                if constexpr (BX) {
                    load_fence();
                    f32x4 xin[2];
#pragma unroll
                    for (int ft = 0; ft < 2; ++ft)
                        xin[ft] = *reinterpret_cast<const f32x4*>(&Hs[(16 * (ct + ctb) + n) * XLD + 16 * ft + 4 * q]);
                    layer_mfma_b6<XD, XD, false>(wa, xin, gt_[ct], lane);
                    continue;
                }
                gt_[ct][0] = zero4();
                gt_[ct][1] = zero4();
                load_fence();
#pragma unroll
                for (int ft = 0; ft < 2; ++ft) {
                    const f32x4 xb = *reinterpret_cast<const f32x4*>(&Hs[(16 * (ct + ctb) + n) * XLD + 16 * ft + 4 * q]);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int g = 0; g < 2; ++g)
                            gt_[ct][g] = mfma4(wa[(16 * ft + 4 * q + r) * WLD + 16 * g + n], xb[r], gt_[ct][g]);
                }
            }
            // S^T[j][col] = X[j] . G[col]
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int jt = 0; jt < NT; ++jt) {
                    load_fence();
                    f32x4 sacc = zero4();
#pragma unroll
                    for (int ft = 0; ft < 2; ++ft) {
                        const int jrow = (PERM && jt == NT - 1) ? 4 * (n & 3) + (n >> 2) : n;       // D row m <-> node perm(m), see jnode
                        const f32x4 xa = *reinterpret_cast<const f32x4*>(&Hs[(16 * jt + jrow) * XLD + 16 * ft + 4 * q]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) sacc = mfma4(xa[r], gt_[ct][ft][r], sacc);
                    }
                    pr[ct][jt] = sacc;
                }
            }
            if (SK == 2) {
                // cosine family (graph_model.py:70-79): C_ij = S_ij / (m_i m_j), m_i = |S_i,:|_2 (rows of S itself).  Row norm of
                // column i: over my registers and the four q-groups; m_j of the other index goes through the padding column
                // 32 of the node-feature rows (XLD = 36).  Padded nodes get 1/m = 0: their rows and columns stay exactly 0.
                load_fence();
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    float z = 0.f;
#pragma unroll
                    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) z = fmaf(pr[ct][jt][r], pr[ct][jt][r], z);
                    z = kgroups_sum(z);
                    const float im = (16 * (ct + ctb) + n < N && z > 0.f) ? 1.f / sqrtf(z) : 0.f;
                    if (q == 0) Hs[(16 * (ct + ctb) + n) * XLD + 32] = im;
#pragma unroll
                    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) pr[ct][jt][r] *= im;
                }
                if (SPLIT) __syncthreads(); else __builtin_amdgcn_wave_barrier();      // every column's 1/m is in place
                load_fence();
#pragma unroll
                for (int jt = 0; jt < NT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float imj = Hs[jnode(jt, r) * XLD + 32];
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct) pr[ct][jt][r] *= imj;
                    }
                if (sim == SIM_COSINE) return;                   // the cosine matrix itself is the adjacency (not normalised)
            }
            // row normalisation: softmax over j (kept in B-operand order), or the plain weights / their row sums
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                float mx = -INFINITY;
#pragma unroll
                for (int jt = 0; jt < NT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = jnode(jt, r);
                        float v = pr[ct][jt][r];
                        if (SK == 1) v = plain_weight(sim, v, 16 * (ct + ctb) + n, j);
                        if (j >= N) v = SK == 1 ? 0.f : -INFINITY;
                        mx = fmaxf(mx, v);
                        pr[ct][jt][r] = v;
                    }
                mx = kgroups_max(mx);
                float sum = 0.f;
#pragma unroll
                for (int jt = 0; jt < NT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (SK != 1) pr[ct][jt][r] = __expf(pr[ct][jt][r] - mx);
                        sum += pr[ct][jt][r];
                    }
                sum = kgroups_sum(sum);
                const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
                for (int jt = 0; jt < NT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pr[ct][jt][r] *= inv;
            }
        };
        if (!a.layerwise) adjacency();
        // layers: H <- relu((A H) W_l) (+ H); every column tile's A*H is taken before any row is overwritten
        for (int l = 0; l < a.L; ++l) {
            if (a.layerwise) adjacency();
            const bool last = (l == a.L - 1);
            const bool rows_only = last && a.rows_out != nullptr;     // value rows: only (A H)[robot] of the last layer is needed
            f32x4 acc[NT][2];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                acc[ct][0] = zero4();
                acc[ct][1] = zero4();
            }
            {
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) {
                load_fence();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (PERM && jt == NT - 1 && r >= last_steps) continue;      // k steps over padding nodes only
                    const float a0 = Hs[jnode(jt, r) * XLD + n];
                    const float a1 = Hs[jnode(jt, r) * XLD + 16 + n];
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        if (rows_only && ct + ctb > 0) continue;
                        acc[ct][0] = mfma4(a0, pr[ct][jt][r], acc[ct][0]);
                        acc[ct][1] = mfma4(a1, pr[ct][jt][r], acc[ct][1]);
                    }
                }
            }
            }
            if (SPLIT) __syncthreads();      // every wave of the scene has taken its A*H: rows may be overwritten
            if (rows_only) {
                // hand-off row of stage 2 (robot_head_kernel): [ (A H_{L-1})[robot] | H_{L-1}[robot] ]; column 0 of tile 0 = robot
                if (active && ctb == 0) {
                    float* out = a.rows_out + (size_t)sc * 64;
                    if (n == 0) {
                        *reinterpret_cast<f32x4*>(out + 4 * q) = acc[0][0];
                        *reinterpret_cast<f32x4*>(out + 16 + 4 * q) = acc[0][1];
                    }
                    if (lane < 8) *reinterpret_cast<f32x4*>(out + 32 + 4 * lane) = *reinterpret_cast<const f32x4*>(&Hs[4 * lane]);
                }
                break;
            }
            const float* wl = ws + l * a.ws_stride;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                load_fence();
                f32x4 o[2] = {zero4(), zero4()};
                if constexpr (BX) {
                    layer_mfma_b6<XD, XD, false>(wl, acc[ct], o, lane);
                } else {
#pragma unroll
                for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int ot = 0; ot < 2; ++ot)
                            o[ot] = mfma4(wl[(16 * ft + 4 * q + r) * WLD + 16 * ot + n], acc[ct][ft][r], o[ot]);
                }
#pragma unroll
                for (int ot = 0; ot < 2; ++ot) {
                    const f32x4 sk = *reinterpret_cast<const f32x4*>(&Hs[(16 * (ct + ctb) + n) * XLD + 16 * ot + 4 * q]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float hv = fmaxf(o[ot][r], 0.f);
                        if (a.skip) hv += sk[r];
                        o[ot][r] = 16 * (ct + ctb) + n < N ? hv : 0.f;          // padded node rows stay exactly zero (a softmax row of a
                    }                                                   // padded node is uniform, not zero; layerwise graphs re-read H)
                    if (!last) *reinterpret_cast<f32x4*>(&Hs[(16 * (ct + ctb) + n) * XLD + 16 * ot + 4 * q]) = o[ot];
                }
                if (last) {
                    // motion head on this tile's columns, straight from registers: 32 -> 64 (ReLU) -> 5
                    f32x4 hm[4] = {zero4(), zero4(), zero4(), zero4()};
                    f32x4 om = zero4();
                    if constexpr (BX) {
                        layer_mfma_b6<XD, HID, true>(wm1, o, hm, lane, bm1);
#pragma unroll
                        for (int ht = 0; ht < 4; ++ht)
#pragma unroll
                            for (int r = 0; r < 4; ++r) hm[ht][r] = fmaxf(hm[ht][r], 0.f);
                        f32x4 om1[1];
                        layer_mfma_b6<HID, 16, false>(wm2, hm, om1, lane);
                        om = om1[0];
                    } else {
#pragma unroll
                    for (int ot = 0; ot < 2; ++ot) {
                        load_fence();
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int ht = 0; ht < 4; ++ht)
                                hm[ht] = mfma4(wm1[(16 * ot + 4 * q + r) * W1LD + 16 * ht + n], o[ot][r], hm[ht]);
                    }
#pragma unroll
                    for (int ht = 0; ht < 4; ++ht) {
                        load_fence();
                        const f32x4 bb = *reinterpret_cast<const f32x4*>(&bm1[16 * ht + 4 * q]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float hv = fmaxf(hm[ht][r] + bb[r], 0.f);
                            om = mfma4(wm2[(16 * ht + 4 * q + r) * M2LD + n], hv, om);
                        }
                    }
                    }
                    const int node = 16 * (ct + ctb) + n;
                    if (active && node >= 1 && node < N) {
                        float* dst = a.humans_next + ((size_t)sc * H + (node - 1)) * 5;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int oidx = 4 * q + r;
                            if (oidx < 5) dst[oidx] = om[r] + bm2[oidx];
                        }
                    }
                }
            }
            if (SPLIT) __syncthreads(); else __builtin_amdgcn_wave_barrier();      // the next layer / adjacency reads the rows written above
        }
        if (SPLIT) __syncthreads();      // the slot's rows are free for the next scene
        PRO_PHASE_MARK(pp, 2);
    }
    c0 = c1;
    } while (WGE && c0 < end);
}

}  // namespace
