// rgl_fused_kernel.hip -- "value of the sibling children" for the shipped shape (L = 2, N <= 32, value head 32-100-100-1) as ONE
// kernel over a stream of 16-child tiles.
//
// Follows (reference paths): crowd_nav/policy/graph_model.py:99-130 (RGL.forward), value_estimator.py:11-20,
// model_predictive_rl.py:245-250 (the per-action loop whose iterations run side by side here).
//
// Algebra: the rank-1 (shared-crowd) form of rgl_rank1.hip -- siblings share every human row of X and of S except the
// robot column, so a human row i of child c is (alpha_i UW_i + beta_i (x0_c W1)) / Z_i with crowd-only UW, msh, Zsh.
// What changes is the organisation (round 2):
//   * children_fused_kernel: every wave owns one 16-child tile from the robot embedding to the VALUE: embedding,
//     robot row/column of S, softmax scalars, the VALU row pass, the robot row, the last GCN layer on the robot row and the
//     value head all run on registers and a 5-6.5 KB wave-private LDS scratch.  No workgroup barrier after the weight image
//     is built, no [P*A][64] fp32 hand-off through HBM, no second launch.  Round 3: every workgroup OWNS a contiguous block
//     of parents; their work items (groups of tiles of one parent, plan_items) are dealt over the workgroup's 8 waves in
//     snake passes, heaviest first, so the four SIMDs of a CU carry the same load.  Because all 81 values of a parent are
//     produced inside one workgroup, the search's bookkeeping for that parent -- one-step values, top-w clipping, gather of the
//     next level's robot rows, and at the deepest level the whole back-up chain and the root decision (rgl_tail.h) -- runs in
//     the TAIL of this kernel behind a workgroup barrier: mprl_select / mprl_backup / mprl_root are no launches of their own.
//   * row pass (softmax similarity, N <= 20) in the MFMA D layout with packed fp32 math: 4 instructions per 2 elements.
//   * the crowd-only quantities of a parent (Xh, G = Xh Wa, UW, msh, Zsh: 208 MFMAs, ~9 % of a parent's work) are computed
//     by the wave that owns the work item, at the item's start, straight into the registers the tiles read them from
//     (the MFMA D layout of the crowd chain IS the A-operand layout of the robot row / column products; the two
//     transposed views go through the wave's own scratch).  Nothing crowd-sized crosses HBM: the kernel reads the child
//     robot rows and the parent's human rows and writes the values.  (Until the end of round 2 a crowd_block_kernel
//     produced 7.8-16.6 KB blocks per parent in global memory: one more launch and 5-10x the algorithmic HBM bytes.)
//   * a parent's partial last tile (A % 16 children; the single `stop` action of the 81-action table) runs everything but
//     the head and leaves its rows in a small buffer; the workgroup scores the rows of ITS partial tiles at the end of the
//     kernel, tile-packed over parents (16 `stop` children = one head tile), so the head never multiplies 15 columns of
//     padding and the whole path is one launch.
// This unit: the kernel and the dispatch from a plan to its instantiation.  Which launches take the kernel and how their tiles are
// cut is rgl_fused.hip's (host only), the weight image rgl_fused_image.hip's; rgl_fused.h is what the three share.
#include "rgl_fused.h"
#include "rgl_scene_body.h"
#include "rgl_tail.h"

using namespace rgl::fused;

namespace {

// h = relu(t W_last)(+hprev), value head 32 -> D1 -> D2 -> D3 -> 1 for the 16 children of a tile (lane (n, q): child n, D-layout
// registers); returns the value of child n in every lane of its column (without the last bias)
template <class LO, int D1, int D2, int D3, bool SKIP, bool BX = false>
__device__ __forceinline__ float head_chain(const float* lds, const f32x4 (&tin)[2], const f32x4 (&hp)[2], int lane) {
    const int q = lane >> 4;
    f32x4 h[2];
    if constexpr (BX) layer_mfma_b6<XD, XD, false>(lds + LO::f_last, tin, h, lane);
    else layer_mfma<XD, XD, false>(lds + LO::f_last, tin, h, lane);
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float x = relu1(h[ot][r]);
            if (SKIP) x += hp[ot][r];
            h[ot][r] = x;
        }
    f32x4 a1[Tiles<D1>::v];
    if constexpr (BX && D1 == 32) layer_mfma_bx1<XD, 32, true>(lds + LO::f1, h, a1, lane, lds + LO::b1);
    else layer_mfma<XD, D1, true>(lds + LO::f1, h, a1, lane, lds + LO::b1);
    relu_tiles<D1>(a1);
    f32x4 a2[Tiles<D2>::v];
    if constexpr (BX) layer_mfma_bx1<D1, D2, true>(lds + LO::f2, a1, a2, lane, lds + LO::b2);
    else layer_mfma<D1, D2, true>(lds + LO::f2, a1, a2, lane, lds + LO::b2);
    relu_tiles<D2>(a2);
    f32x4 a3[Tiles<D3>::v];
    if constexpr (BX) layer_mfma_bx<D2, D3, true>(lds + LO::f3, a2, a3, lane, lds + LO::b3);
    else layer_mfma<D2, D3, true>(lds + LO::f3, a2, a3, lane, lds + LO::b3);
    relu_tiles<D3>(a3);
    float v = 0.f;
#pragma unroll
    for (int ot = 0; ot < Tiles<D3>::v; ++ot) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(&lds[LO::w4 + 16 * ot + 4 * q]);
#pragma unroll
        for (int r = 0; r < 4; ++r) v = fmaf(a3[ot][r], w[r], v);
    }
    return kgroups_sum(v);
}

// BX: one 16 x 16 block of A B^T over a K = 32 chunk whose BOTH operands are three-piece register operands (split3_pair of two
// D-layout tiles: the crowd's S = G Xh^T and U = E Xh, the tile's robot row / column of S) -- the six terms of layer_mfma_b6, small
// ones first
__device__ __forceinline__ f32x4 b6_block(const Split3& a, const Split3& b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l, b.h, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.m, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.l, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.h, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.m, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, acc, 0, 0, 0);
}

// scale of the PK row pass (children_fused_kernel): its ReLU sits in the clamp bit of v_pk_fma_f32 (rgl_mfma.h), which clamps to [0, 1]
constexpr float kRowScale = 0x1p-110f, kRowUnscale = 0x1p110f;

// HR >= N: human rows of UW held in registers (padded rows contribute exactly 0); SOFT: softmax row normalisation
// BX: the D2 x D3 head matrix's first 64 input features as six bf16 terms on the matrix pipe (layer_mfma_bx; RGL_CONTRACT_BF16X6)
// PRO: the level prologue (RGL_LEVEL_PROLOGUE): the workgroup first runs the state predictor and the reward / next-state pairs of the
// parents it owns -- the humans_next rows and child robot rows its items read, the rewards its tail reads -- so that a tree level is
// ONE launch (instead of embeddings + rewards, scenes, children)
template <int HR, int NT, bool SKIP, bool SOFT, int D1, int D2, int D3, bool BX = false, bool PRO = false>
__global__ __launch_bounds__(kFusedWaves * 64) void children_fused_kernel(const FusedArgs a, const PrologueArgs<PRO> pa) {
    const int sim = SOFT ? (int)SIM_SOFTMAX : a.sim;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using LO = FusedLds<D1, D2, D3, BX>;
    constexpr int NP = 16 * NT;
    constexpr int nthreads = kFusedWaves * 64;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    constexpr bool PK = fused_packed_rows(HR, SOFT);    // row pass in the D layout with packed fp32 math
    // 16 < N <= 20 (the shipped crowd): the second node tile holds four valid nodes.  Its rows of the robot row / column of S come
    // from v_mfma_f32_4x4x1_16B_f32 (rgl_mlp_chain.h: 12 clocks instead of 32 per k step) and land, after a reduce-scatter over
    // the k-groups, as node 16 + q in register 0 of lane (n, q): the tile's node order is 16 + 4 r + q, registers 1..3 are
    // padding -- their exps, table entries and k steps of p Xh are not computed at all.
    constexpr bool T1P = PK && NT == 2 && HR <= 20;
    constexpr int HRL = HR < NP ? HR : NP;              // rows of UW the row pass visits (rows >= N are zero)
    constexpr int SLDK = HRL + 2;
    const int N = a.N, A = a.A, SLD = PK ? SLDK : a.SLD;
    const float NEG_INF = -INFINITY;
    const float* wr1 = lds + LO::wr1;   // [12][W1LD], rows 9..11 zero (BX: [9][72], see FusedLds)
    const float* br1 = lds + LO::br1;
    const float* wr2 = lds + LO::wr2;   // [HID][WLD]
    const float* br2 = lds + LO::br2;
    const float* wa = lds + LO::wa;     // [XD][WLD]
    const float* w1 = lds + LO::w1;     // [XD][WLD]
    float* WS = lds + LO::scratch + wave * fused_scratch_floats(HR, NT, SOFT);
    float* UWs = WS;                                                    // PK: [HRL][32] UW rows of the item's parent
    float* AB = PK ? WS + HRL * 32 : WS;                                // [16][SLD][2]: per child and row (a, b) / (r, b), p folded in
    float* Y0 = AB + 2 * 16 * SLD;                                      // !PK: [16][XLD]: x0 W1, then t_c without the robot-row term
    const float hb4 = a.hb4[0];

    // Work items of the parents this workgroup owns, dealt over its 8 waves:
    //   item (j, p), group-major (all first groups, then all second ...): G consecutive full tiles of parent p; the LAST (short)
    //   group of a parent starts with its partial tile (A % 16 children: everything but the head, rows -> rows_left; scored at the
    //   end of the kernel, tile-packed over the workgroup's parents) -- or, with few parents per workgroup (inline_partial), the
    //   partial tile is one more ordinary tile with its own head.
    // The crowd quantities of a parent are computed once per item, and the NEXT item's loads (robot rows, crowd state rows) are
    // issued before the head of the current item's last tile: no item starts waiting on HBM.
    const int G = a.tiles_per_item;
    const int p_first = blockIdx.x * a.parents_per_wg;          // my workgroup's parents: p_first .. p_first + k_b - 1
    const int k_b = a.P - p_first < a.parents_per_wg ? a.P - p_first : a.parents_per_wg;
    const int n_items = k_b * a.items_per_parent;
    const int n_pass = (n_items + kFusedWaves - 1) / kFusedWaves;
    // pass k deals the workgroup's items 8 k .. 8 k + 7 over its waves, odd passes in reverse ("snake"): with the heavy items
    // first in the order, the waves that got a heavy item in one pass get a light one (or none) in the next; waves w and w + 4
    // share a SIMD
    auto item_at = [&](int k) { return k * kFusedWaves + ((k & 1) ? kFusedWaves - 1 - wave : wave); };
    const int n_tiles_inl = a.n_full + (a.inline_partial ? 1 : 0);      // tiles that run their own head
    float rin[3], hin[NT][2];
    // BX: w_h's second matrix [64][32] as the A-operand elements my lane feeds to its 32 MFMAs of every crowd computation --
    // fragment (ht, r, ot): row 16 ht + 4 q + r, column 16 ot + n -- held in registers for the whole kernel (see FusedLds::bh2)
    float wh2r[BX ? 32 : 1];
    auto wh2_loads = [&]() {
        if constexpr (BX) {
#pragma unroll
            for (int ht = 0; ht < 4; ++ht)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ot = 0; ot < 2; ++ot) wh2r[(ht * 4 + r) * 2 + ot] = a.wh2[(16 * ht + 4 * q + r) * XD + 16 * ot + n];
        }
    };
    if (!PRO) wh2_loads();
    f32x4 gq[NT][2], xq[NT][2], ms[NT], zs[NT], xt[NT][2], uw4[HRL / 4];
    float xt1p[2] = {0.f, 0.f}, ms1 = 0.f, zs1 = 1.f;      // T1P: Xh^T[f][node 16 + q], msh / Zsh of node 16 + q
    constexpr int NTS = T1P ? 1 : NT;                        // node tiles of the tile's robot row / column of S on the 16 x 16 MFMA
    // BXS: those products as six terms, their A operands (rows of G, Xh) held as pieces, split once per item -- where one node tile
    // takes them (+8 VGPRs); two (N > 20, or a plain similarity with N > 16) would add 16 to kernels that spill already
    constexpr bool BXS = BX && NTS == 1;
    Split3 gpc[BXS ? NTS : 1], xpc[BXS ? NTS : 1];
    // item wi = (order position o, local parent), o-major; group j = (o + rot) % items_per_parent covers the full tiles j G ..; the
    // LAST group (the short one) also carries the parent's partial tile, which it runs first.  Tile sequence ts .. t1-1, where
    // t < t0 means "the partial tile".
    auto item_tiles = [&](int wi, int& p, int& t0, int& ts, int& t1) {
        const int o = wi / k_b;
        p = p_first + (wi - o * k_b);
        int j = o + a.rot;
        if (j >= a.items_per_parent) j -= a.items_per_parent;
        t0 = j * G;
        t1 = t0 + G < n_tiles_inl ? t0 + G : n_tiles_inl;
        ts = (j == a.items_per_parent - 1 && a.rem && !a.inline_partial) ? t0 - 1 : t0;
    };
    auto robot_rows = [&](int p, int t) {                          // rows of child 16 t + n of parent p -> rin
        const int c0 = 16 * t + n;
        const float* rr = a.child_robot + ((size_t)p * A + (c0 < A ? c0 : A - 1)) * 9;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int k = 4 * s + q;
            rin[s] = k < 9 ? rr[k] : 0.f;
        }
    };
    auto human_rows = [&](int p) {                                 // state rows of the parent's crowd (node 16 pct + n) -> hin
#pragma unroll
        for (int pct = 0; pct < NT; ++pct) {
            const int node = 16 * pct + n;
            const bool ok = node >= 1 && node < N;
            const float* hsrc = a.humans + ((size_t)p * a.H + (ok ? node - 1 : 0)) * 5;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int k = 4 * s + q;
                hin[pct][s] = (ok && k < 5) ? hsrc[k] : 0.f;
            }
        }
    };
    auto item_loads = [&](int wi) {                                // first robot rows + crowd state rows of item wi
        int p, t0, ts, t1;
        item_tiles(wi, p, t0, ts, t1);
        robot_rows(p, ts < t0 ? a.n_full : ts);
        human_rows(p);
    };
    // Crowd-only quantities of the item's parent, from hin, into the registers the tiles read (row 0 = robot slot and rows >= N
    // are zero rows / contribute nothing).  The MFMA D layout of the chain (lane (n, q): node 16 pct + n, features 16 ot + 4 q + r)
    // is the A-operand layout of the S products; Xh^T and the feature-major UW go through the wave's scratch (free between items).
    auto crowd_compute = [&]() {
        const float* wh1 = lds + LO::wh1;   // [8][W1LD], rows 5..7 zero (BX: [5][72])
        const float* bh1 = lds + LO::bh1;
        const float* wh2 = lds + LO::wh2;   // [HID][WLD]
        const float* bh2 = lds + LO::bh2;
        float* Xs = WS;                     // [NP][XLD]: Xh, later UW
        float* msz = WS + NP * XLD;         // [2][NP]: msh | Zsh
        // part 1: Xh = w_h(humans), G = Xh Wa   (transposed MFMA chain, 16 nodes per pass)
#pragma unroll
        for (int pct = 0; pct < NT; ++pct) {
            const int node = 16 * pct + n;
            const bool node_ok = node >= 1 && node < N;
            f32x4 hacc[4] = {zero4(), zero4(), zero4(), zero4()};
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int k = 4 * s + q;
#pragma unroll
                for (int ht = 0; ht < 4; ++ht) hacc[ht] = mfma4(wh1[(k < LO::WH1ROWS ? k : LO::WH1ROWS - 1) * LO::WH1LD + 16 * ht + n], hin[pct][s], hacc[ht]);
            }
#pragma unroll
            for (int ht = 0; ht < 4; ++ht) {
                const f32x4 bb = *reinterpret_cast<const f32x4*>(&bh1[16 * ht + 4 * q]);
#pragma unroll
                for (int r = 0; r < 4; ++r) hacc[ht][r] = relu1(hacc[ht][r] + bb[r]);
            }
            f32x4 xa[2] = {zero4(), zero4()};
            {
#pragma unroll
            for (int ht = 0; ht < 4; ++ht) {
                load_fence();
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ot = 0; ot < 2; ++ot)
                        xa[ot] = mfma4(BX ? wh2r[BX ? (ht * 4 + r) * 2 + ot : 0] : wh2[(16 * ht + 4 * q + r) * WLD + 16 * ot + n], hacc[ht][r], xa[ot]);
            }
            load_fence();
#pragma unroll
            for (int ot = 0; ot < 2; ++ot) {
                const f32x4 bb = *reinterpret_cast<const f32x4*>(&bh2[16 * ot + 4 * q]);
#pragma unroll
                for (int r = 0; r < 4; ++r) xa[ot][r] = node_ok ? relu1(xa[ot][r] + bb[r]) : 0.f;   // robot slot / padding rows: 0
                *reinterpret_cast<f32x4*>(&Xs[node * XLD + 16 * ot + 4 * q]) = xa[ot];
                xq[pct][ot] = xa[ot];
            }
            f32x4 pg[2] = {zero4(), zero4()};
            if constexpr (BX) layer_mfma_b6<XD, XD, false>(wa, xa, pg, lane);
            else {
#pragma unroll
            for (int ot = 0; ot < 2; ++ot) {
                load_fence();
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int gt = 0; gt < 2; ++gt)
                        pg[gt] = mfma4(wa[(16 * ot + 4 * q + r) * WLD + 16 * gt + n], xa[ot][r], pg[gt]);
            }
            load_fence();
            }
            gq[pct][0] = pg[0];
            gq[pct][1] = pg[1];
            }
        }
        __builtin_amdgcn_wave_barrier();
        load_fence();
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                for (int r = 0; r < 4; ++r)      // Xh^T for p Xh and U; T1P: only k step 0 of tile 1 is read by the tiles (node 16 + q)
                    xt[nt][ot][r] = Xs[(16 * nt + 4 * q + r) * XLD + 16 * ot + n];
        if constexpr (T1P) {
#pragma unroll
            for (int ot = 0; ot < 2; ++ot) xt1p[ot] = Xs[(16 + q) * XLD + 16 * ot + n];
        }
        load_fence();
        __builtin_amdgcn_wave_barrier();
        
        // part 2 (every Xh row is in registers now): S_ij = G_i . Xh_j over humans j, msh / E / Zsh, U = E Xh, UW = U W1
        // BX: S and U as six-term products; Xh and Xh^T are split once per item (one K = 32 chunk each: the 32 features of a node
        // tile, the <= 32 nodes of a feature tile)
        Split3 xqs[BX ? NT : 1], xts[BX ? 2 : 1];
        if constexpr (BX) {
            static_assert(NT <= 2, "Xh^T: one chunk over the nodes");
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) xqs[jt] = split3_pair(xq[jt][0], xq[jt][1]);
            if constexpr (BXS) xpc[0] = xqs[0];
#pragma unroll
            for (int ft = 0; ft < 2; ++ft) xts[ft] = split3_pair(xt[0][ft], NT > 1 ? xt[NT > 1 ? 1 : 0][ft] : zero4());
        }
#pragma unroll
        for (int pct = 0; pct < NT; ++pct) {
            const int node = 16 * pct + n;
            const bool node_ok = node >= 1 && node < N;
            f32x4 e[NT];
            float mx = NEG_INF;
            Split3 gs;
            if constexpr (BX) {
                gs = split3_pair(gq[pct][0], gq[pct][1]);
                if (BXS && pct == 0) gpc[0] = gs;
            }
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) {
                f32x4 sacc = zero4();
                if constexpr (BX) sacc = b6_block(xqs[jt], gs, sacc);
                else {
#pragma unroll
                for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sacc = mfma4(xq[jt][ft][r], gq[pct][ft][r], sacc);      // [j = 16jt+4q+r][i = my node]
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * jt + 4 * q + r;
                    if (sim != SIM_SOFTMAX) sacc[r] = plain_weight(sim, sacc[r], node, j);
                    if (j < 1 || j >= N) sacc[r] = sim == SIM_SOFTMAX ? NEG_INF : 0.f;
                    mx = fmaxf(mx, sacc[r]);
                }
                e[jt] = sacc;
            }
            mx = kgroups_max(mx);
            if (!node_ok || sim != SIM_SOFTMAX) mx = 0.f;
            float z = 0.f;
#pragma unroll
            for (int jt = 0; jt < NT; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (sim == SIM_SOFTMAX) e[jt][r] = __expf(e[jt][r] - mx);
                    if (!node_ok) e[jt][r] = 0.f;
                    z += e[jt][r];
                }
            z = kgroups_sum(z);
            if (q == 0) {
                msz[node] = mx;
                msz[NP + node] = node_ok ? z : 1.f;
            }
            f32x4 u[2] = {zero4(), zero4()};
            f32x4 uw[2] = {zero4(), zero4()};
            {
            if constexpr (BX) {
                const Split3 es = split3_pair(e[0], NT > 1 ? e[NT > 1 ? 1 : 0] : zero4());
                u[0] = b6_block(xts[0], es, u[0]);
                u[1] = b6_block(xts[1], es, u[1]);
            } else {
#pragma unroll
            for (int jt = 0; jt < NT; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    u[0] = mfma4(xt[jt][0][r], e[jt][r], u[0]);                               // U^T[f][i] = sum_j Xh[j][f] E[i][j]
                    u[1] = mfma4(xt[jt][1][r], e[jt][r], u[1]);
                }
            }
            if constexpr (BX) layer_mfma_b6<XD, XD, false>(w1, u, uw, lane);
            else {
#pragma unroll
            for (int ft = 0; ft < 2; ++ft) {
                load_fence();
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ot = 0; ot < 2; ++ot)
                        uw[ot] = mfma4(w1[(16 * ft + 4 * q + r) * WLD + 16 * ot + n], u[ft][r], uw[ot]);
            }
            load_fence();
            }
            }
            if constexpr (PK) {                                                              // UW rows over the (consumed) Xh rows
                if (node < HRL) {
                    *reinterpret_cast<f32x4*>(&UWs[node * 32 + 4 * q]) = uw[0];
                    *reinterpret_cast<f32x4*>(&UWs[node * 32 + 16 + 4 * q]) = uw[1];
                }
            } else {
                *reinterpret_cast<f32x4*>(&Xs[node * XLD + 4 * q]) = uw[0];
                *reinterpret_cast<f32x4*>(&Xs[node * XLD + 16 + 4 * q]) = uw[1];
            }
        }
        __builtin_amdgcn_wave_barrier();
        load_fence();
#pragma unroll
        for (int nt = 0; nt < (T1P ? 1 : NT); ++nt) {
            ms[nt] = *reinterpret_cast<const f32x4*>(&msz[16 * nt + 4 * q]);
            zs[nt] = *reinterpret_cast<const f32x4*>(&msz[NP + 16 * nt + 4 * q]);
        }
        if constexpr (T1P) {
            ms1 = msz[16 + q];
            zs1 = msz[NP + 16 + q];
            // rows 16..19 of G and Xh as A operands of the 4 x 4 x 1 blocks: A row = lane % 4 (rows 20..31 were zero padding)
#pragma unroll
            for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gq[1][ot][r] = quad0_bcast(gq[1][ot][r]);
                    xq[1][ot][r] = quad0_bcast(xq[1][ot][r]);
                }
        }
        if constexpr (!PK) {
#pragma unroll
            for (int i4 = 0; i4 < HRL / 4; ++i4)
#pragma unroll
                for (int k = 0; k < 4; ++k) uw4[i4][k] = Xs[(4 * i4 + k) * XLD + (lane & 31)];  // lane = feature holds its nodes
        }
        load_fence();
        __builtin_amdgcn_wave_barrier();      // the tiles' AB / Y0 writes stay behind these reads
    };
    // Weight image -> LDS with LDS-direct loads (global_load_lds_dwordx4: a wave moves 1 KB per instruction, no registers in
    // between), in TWO parts (round 4): everything the crowd quantities and a tile need before its head -- the embedding and graph
    // matrices, the per-feature vectors: [0, f_last), a third of the image -- is waited for here; the value head's fragments (the
    // other two thirds) keep streaming in under the first item's crowd computation and its first tile's embedding / row pass, and
    // every wave waits for them once, in front of its first head (await_image: its own loads via vmcnt, the other waves' via an
    // LDS counter).  Until round 4 the whole image was staged through registers before anything else ran: ~4 us of every launch.
    static_assert(LO::scratch % 4 == 0 && LO::f_last % 4 == 0, "b128 granules");
    constexpr int kChunk = 256;                                            // floats per wave and instruction
    constexpr int kChunksA = (LO::f_last + kChunk - 1) / kChunk, kChunksAll = (LO::scratch + kChunk - 1) / kChunk;
    static_assert(LO::scratch == FusedImage<BX>::scratch, "fused_lds_floats is written for the shipped head's image");
    int* image_arrivals = reinterpret_cast<int*>(lds + fused_lds_floats(HR, NT, SOFT, BX) - kArrivalFloats);
    // ... and in the same granule, for the tile-packed head pass (RGL_FUSED_HEAD_EARLY, below): the rows the partial tiles have
    // handed off so far, and the packed tiles taken so far
    int* rows_arrivals = image_arrivals + 1;
    int* packed_taken = image_arrivals + 2;
    static_assert(kArrivalFloats >= 3, "three counters");
    auto image_chunk = [&](int c) {
        const int fl = c * kChunk + lane * 4;
        if (fl < LO::scratch)                                              // the last chunk is partial
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.image + fl),
                                             (__attribute__((address_space(3))) void*)(lds + c * kChunk), 16, 0, 0);
    };
    if constexpr (PRO) {
        // LDS during the prologue: the image's first part [0, f_last) -- requested here, it lands under the scene image's loads and
        // is waited for with them -- and behind its last chunk the scene region (predictor image, embedding sets, 8 wave slots:
        // 97 KB), which the rest of the image and the wave scratches overwrite behind the barrier below
        // The embeddings are the workgroup's (scene_body's WGE form): the rows of the owned parents' distinct crowds and their robot
        // rows, a chunk of 16 parents at a time, into a row buffer behind the wave slots.
        static_assert(kPrologueSceneBase<LO> == kChunksA * kChunk, "the scene region starts behind the first part's chunks");
        static_assert(kPrologueSceneBase<LO> + prologue_scene_floats(2, 19) <= fused_lds_floats(HR, NT, SOFT, BX),
                      "a two-layer predictor's scene region with the row buffer of a full chunk (12 crowds of 19 humans, 16 robot rows) fits the kernel's LDS");
        ProPhases pro_phases;
        ProPhases* const pp = &pro_phases;
        PRO_PHASE_START(pp);
        for (int c = wave; c < kChunksA; c += kFusedWaves) image_chunk(c);
#ifdef RGL_PROLOGUE_EMB_PER_WAVE      // measurements (the timing build's "before" column): every wave embeds its own scene's rows
        constexpr bool kWge = false;
#else
        constexpr bool kWge = true;
#endif
        scene_body<2, 0, kFusedWaves, false, true, true, kWge>(pa.scene, lds + kPrologueSceneBase<LO>, p_first, 1, kFusedWaves,
                                                               p_first + k_b, pp);
        const ChildrenArgs& ca = pa.children;
        const long long pair0 = (long long)p_first * ca.A, pair_end = (long long)(p_first + k_b) * ca.A;
        if (ca.A >= 64 && ca.H <= 64 && !ca.robot64) {       // as the stand-alone launches: whole waves, far-human masks per parent
            const float v_max = table_speed_bound(ca);
            for (long long base = pair0 + 64 * wave; base < pair_end; base += 64 * kFusedWaves) children_wave(ca, base, pair_end, v_max);
        } else {
            for (long long idx = pair0 + tid; idx < pair_end; idx += nthreads) children_thread(ca, idx);
        }
        PRO_PHASE_MARK(pp, 3);
        __syncthreads();                 // my parents' humans_next, child robot rows and rewards are written; the scene region is free
        PRO_PHASE_MARK(pp, 4);
        PRO_PHASE_FLUSH(pp);
        wh2_loads();
    }
    // (the first item's state rows are requested BEFORE the image: the wait in front of the barrier covers them, and no later
    // wait for them can hold the wave until the head fragments have landed as well -- vmcnt counts in order)
    if (wave < n_items) item_loads(item_at(0));
    if (tid == 0) *image_arrivals = *rows_arrivals = *packed_taken = 0;
    bool image_complete = false;                                           // wave-uniform
    if (a.image_sync) {                                                    // RGL_FUSED_IMAGE_SYNC=1 (measurements): the round-3 copy
        copy_image<LO::scratch, nthreads>(lds, a.image, tid);
        __syncthreads();
        image_complete = true;
    } else {
    if (!PRO) for (int c = wave; c < kChunksA; c += kFusedWaves) image_chunk(c);          // (PRO: loaded in the prologue)
    wait_vmcnt0();
    __syncthreads();
    for (int c = kChunksA + wave; c < kChunksAll; c += kFusedWaves) image_chunk(c);
    }
    auto await_image = [&]() {
        if (image_complete) return;
        wait_vmcnt0();                                                     // my share of the head fragments has landed
        asm volatile("" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(image_arrivals, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (__hip_atomic_load(image_arrivals, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < kFusedWaves) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
        image_complete = true;
    };
    if (wave >= 4) {
        for (int i = 0; i < a.phase_delay; ++i) __builtin_amdgcn_s_sleep(8);
        if (a.prio & 1) __builtin_amdgcn_s_setprio(1);
    }
    PHASE_START();
    for (int pass = 0; pass < n_pass; ++pass) {
        const int wi = item_at(pass);
        if (wi >= n_items) break;                          // only the last pass is short
        const int wi_next = pass + 1 < n_pass ? item_at(pass + 1) : n_items;
        PHASE_MARK(0);
        int p, t0, ts, t1;
        item_tiles(wi, p, t0, ts, t1);
        load_fence();
        crowd_compute();
        PHASE_MARK(1);

      for (int ti = ts; ti < t1; ++ti) {
        const int t = ti < t0 ? a.n_full : ti;             // the first group of a parent starts with the partial tile
        const bool full = t < a.n_full;
        const int c = 16 * t + n;                          // my child (column of the MFMA tiles)
        const int n_valid = full ? 16 : a.rem;

        // ---------------- embedding: x0 = w_r(robot'), y = x0 W1, g0 = x0 Wa (transposed MFMA chain) ----------------
        f32x4 xacc[2] = {zero4(), zero4()}, gacc[2] = {zero4(), zero4()}, yacc[2] = {zero4(), zero4()};
        float s00 = 0.f;
        Split3 sx;                                         // BX: pieces of x0 (the products with Wa, W1 and the robot column of S)
        {
            f32x4 hacc[4] = {zero4(), zero4(), zero4(), zero4()};
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int k = 4 * s + q;
#pragma unroll
                for (int ht = 0; ht < 4; ++ht) hacc[ht] = mfma4(wr1[(k < LO::WR1ROWS ? k : LO::WR1ROWS - 1) * LO::WR1LD + 16 * ht + n], rin[s], hacc[ht]);
            }
            if (ti + 1 < t1) robot_rows(p, ti + 1);      // robot rows of my next tile: in flight under this tile's work
#pragma unroll
            for (int ht = 0; ht < 4; ++ht) {
                const f32x4 bb = *reinterpret_cast<const f32x4*>(&br1[16 * ht + 4 * q]);
#pragma unroll
                for (int r = 0; r < 4; ++r) hacc[ht][r] = relu1(hacc[ht][r] + bb[r]);
            }
            if constexpr (BX) {
                // round 6: the tile chain's weight products -- hidden -> x0 (64 x 32), x0 Wa, x0 W1 -- as six bf16 terms over three-piece
                // operands too (fragments in the image where the f32 matrices were; x0 is split once for both products)
                layer_mfma_b6<HID, XD, true>(wr2, hacc, xacc, lane, br2);
#pragma unroll
                for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                    for (int r = 0; r < 4; ++r) xacc[ot][r] = relu1(xacc[ot][r]);
                sx = split3_pair(xacc[0], xacc[1]);
                layer_mfma_b6_pre<XD, false>(wa, sx, gacc, lane);
                layer_mfma_b6_pre<XD, false>(w1, sx, yacc, lane);
            } else {
#pragma unroll
            for (int ht = 0; ht < 4; ++ht) {
                load_fence();
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ot = 0; ot < 2; ++ot)
                        xacc[ot] = mfma4(wr2[(16 * ht + 4 * q + r) * WLD + 16 * ot + n], hacc[ht][r], xacc[ot]);
            }
            load_fence();
#pragma unroll
            for (int ot = 0; ot < 2; ++ot) {
                const f32x4 bb = *reinterpret_cast<const f32x4*>(&br2[16 * ot + 4 * q]);
#pragma unroll
                for (int r = 0; r < 4; ++r) xacc[ot][r] = relu1(xacc[ot][r] + bb[r]);
            }
#pragma unroll
            for (int ot = 0; ot < 2; ++ot) {
                load_fence();
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int gt = 0; gt < 2; ++gt) {
                        gacc[gt] = mfma4(wa[(16 * ot + 4 * q + r) * WLD + 16 * gt + n], xacc[ot][r], gacc[gt]);
                        yacc[gt] = mfma4(w1[(16 * ot + 4 * q + r) * WLD + 16 * gt + n], xacc[ot][r], yacc[gt]);
                    }
            }
            load_fence();
            }
            if constexpr (!PK) {
                *reinterpret_cast<f32x4*>(&Y0[n * XLD + 4 * q]) = yacc[0];
                *reinterpret_cast<f32x4*>(&Y0[n * XLD + 16 + 4 * q]) = yacc[1];
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) s00 = fmaf(gacc[tt][r], xacc[tt][r], s00);
            s00 = kgroups_sum(s00);
        }

        PHASE_MARK(2);
        // ---------------- robot row / column of S, p = softmax(robot row), p Xh, the (a, b) table ---------------------
        // all in the MFMA D layout: lane (n, q) = child 16 t + n, registers = nodes 16 nt + 4 q + r
        f32x4 t0h[2] = {zero4(), zero4()};        // (p_c Xh)^T of my 16 children
        float p00;                                // A_c[0][0]
        {
            f32x4 s0t[NT], sct[NT];
            float mx0 = NEG_INF;
            float sc1 = NEG_INF, p1 = NEG_INF;           // T1P: S_c[16 + q][0], then S_c[0][16 + q] -> p of node 16 + q
            if constexpr (T1P) {
                f32x4 psc[2] = {zero4(), zero4()}, ps0[2] = {zero4(), zero4()};
#pragma unroll
                for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        psc[r & 1] = mfma4x4(gq[1][ot][r], xacc[ot][r], psc[r & 1]);
                        ps0[r & 1] = mfma4x4(xq[1][ot][r], gacc[ot][r], ps0[r & 1]);
                    }
                sc1 = kgroups_reduce_scatter(psc[0] + psc[1]);
                p1 = kgroups_reduce_scatter(ps0[0] + ps0[1]);
                if (16 + q >= N) { sc1 = NEG_INF; p1 = NEG_INF; }
                mx0 = p1;
            }
            Split3 sg;                                   // BX: pieces of g0 = x0 Wa
            if constexpr (BXS) sg = split3_pair(gacc[0], gacc[1]);
#pragma unroll
            for (int nt = 0; nt < NTS; ++nt) {
                f32x4 sc = zero4(), s0 = zero4();
                if constexpr (BXS) {
                    sc = b6_block(gpc[0], sx, sc);
                    s0 = b6_block(xpc[0], sg, s0);
                } else {
#pragma unroll
                for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        sc = mfma4(gq[nt][ot][r], xacc[ot][r], sc);
                        s0 = mfma4(xq[nt][ot][r], gacc[ot][r], s0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int nd = 16 * nt + 4 * q + r;
                    if (nd == 0) { sc[r] = s00; s0[r] = s00; }
                    if (sim != SIM_SOFTMAX) s0[r] = plain_weight(sim, s0[r], 0, nd);
                    if (!T1P && nd >= N) { sc[r] = NEG_INF; s0[r] = sim == SIM_SOFTMAX ? NEG_INF : 0.f; }   // T1P: nd <= 15 < N here
                    mx0 = fmaxf(mx0, s0[r]);
                }
                s0t[nt] = s0;
                sct[nt] = sc;
            }
            mx0 = kgroups_max(mx0);
            float z0 = 0.f;
            if constexpr (T1P) {
                p1 = __expf(p1 - mx0);
                z0 = p1;
            }
#pragma unroll
            for (int nt = 0; nt < (T1P ? 1 : NT); ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (sim == SIM_SOFTMAX) s0t[nt][r] = __expf(s0t[nt][r] - mx0);
                    z0 += s0t[nt][r];
                }
            const float iz0 = __builtin_amdgcn_rcpf(kgroups_sum(z0));
            if constexpr (T1P) p1 *= iz0;
#pragma unroll
            for (int nt = 0; nt < (T1P ? 1 : NT); ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) s0t[nt][r] *= iz0;                       // p = A_c[0][:] (0 beyond row N-1)
            p00 = kgroups_sum(q == 0 ? s0t[0][0] : 0.f);
            // (p_c Xh)^T[f][c] = sum_j Xh^T[f][j] p_c[j]: the D registers of the robot-row product are already the B operand
            {
#pragma unroll
            for (int nt = 0; nt < (T1P ? 1 : NT); ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    t0h[0] = mfma4(xt[nt][0][r], s0t[nt][r], t0h[0]);
                    t0h[1] = mfma4(xt[nt][1][r], s0t[nt][r], t0h[1]);
                }
            if constexpr (T1P) {                                 // nodes 16..19: ONE k step (k slot q = node 16 + q)
                t0h[0] = mfma4(xt1p[0], p1, t0h[0]);
                t0h[1] = mfma4(xt1p[1], p1, t0h[1]);
            }
            }
            if constexpr (PK) {
                // human row i of child c: relu((alpha UW_i + beta y_c) / Z) weighted by p_i = b_i relu(r_i UW_i + y_c) with
                // r_i = alpha / beta = exp(msh_i - S_i0), b_i = p_i beta / Z = p_i / (r_i Zsh_i + 1); r is capped at e^60 (beyond,
                // beta y is below fp32 resolution of the row and b r = p / Zsh is exact)
#pragma unroll
                for (int nt = 0; nt < (T1P ? 1 : NT); ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int nd = 16 * nt + 4 * q + r;
                        const float rr = __expf(fminf(ms[nt][r] - sct[nt][r], 60.f));
                        const float bb = s0t[nt][r] * __builtin_amdgcn_rcpf(fmaf(rr, zs[nt][r], 1.f));
                        // T1P: rows 1..15 are humans whatever N is (N > 16) and lie inside the table: no guards, no exec masks
                        const bool rh = T1P ? nd >= 1 : (nd >= 1 && nd < N);
                        if (T1P || nd < HRL) *reinterpret_cast<f32x2*>(&AB[(n * SLDK + nd) * 2]) = f32x2{rh ? rr * kRowScale : 0.f, rh ? bb : 0.f};
                    }
                if constexpr (T1P) {                             // node 16 + q (HRL == 20: rows 16..19 of the table)
                    const int nd = 16 + q;
                    const float rr = __expf(fminf(ms1 - sc1, 60.f));
                    const float bb = p1 * __builtin_amdgcn_rcpf(fmaf(rr, zs1, 1.f));
                    const bool rh = nd < N;
                    *reinterpret_cast<f32x2*>(&AB[(n * SLDK + nd) * 2]) = f32x2{rh ? rr * kRowScale : 0.f, rh ? bb : 0.f};      // nd <= 19 < HRL = 20
                }
            } else {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int nd = 16 * nt + 4 * q + r;
                        const float pv = s0t[nt][r];
                        float al, be;
                        if (sim == SIM_SOFTMAX) {
                            const float m = fmaxf(ms[nt][r], sct[nt][r]);
                            al = __expf(ms[nt][r] - m);
                            be = __expf(sct[nt][r] - m);
                        } else {
                            al = 1.f;
                            be = plain_weight(sim, sct[nt][r], nd, 0);        // diagonal: nd >= 1 here, so 0
                        }
                        const float piz = pv * __builtin_amdgcn_rcpf(fmaf(al, zs[nt][r], be));
                        const bool rh = nd >= 1 && nd < N;
                        *reinterpret_cast<f32x2*>(&AB[(n * SLD + nd) * 2]) = f32x2{rh ? al * piz : 0.f, rh ? be * piz : 0.f};
                    }
            }
        }
        __builtin_amdgcn_wave_barrier();
        load_fence();
        PHASE_MARK_ALT(!full, 3);      // (the partial tile's crowd stage -- this phase and the row pass -- has counter 15)

        // ---------------- row pass over my 16 children -------------------------------------------------------------------
        f32x4 tp4[2] = {zero4(), zero4()};           // PK: t_c without the robot-row / skip terms, D layout (child n, features)
        if constexpr (PK) {
            // D layout throughout: lane (n, q) = child n, features 4q..4q+3 and 16+4q..: y and the result stay in registers, the
            // child's (r_i, b_i) come as broadcast b128 reads (two nodes each), UW_i as two broadcast b128 reads; per node and feature
            // pair: v_pk_fma (r UW + y) with the ReLU in its clamp bit, v_pk_fma (acc += b relu) -- 2 instructions per 2 elements
            // (round 3: 4, with two integer-max relus; the lane = feature form spends 8: DPP broadcasts cannot feed packed operands).
            // The clamp is to [0, 1], so the pass runs on 2^-110 of its values: r (in the table) and y carry the factor, every
            // product and sum is the exact 2^-110 multiple of the unscaled one -- power-of-two scalings commute with rounding -- as
            // long as r UW + y stays below 2^110 = 1.3e33 (r <= e^60 = 1.1e26: UW up to 1e7) and terms below 2^-39 are not missed;
            // the sum is scaled back once per tile.
            f32x2 acc[4] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};
            const f32x2 y2[4] = {f32x2{yacc[0][0], yacc[0][1]} * kRowScale, f32x2{yacc[0][2], yacc[0][3]} * kRowScale,
                                 f32x2{yacc[1][0], yacc[1][1]} * kRowScale, f32x2{yacc[1][2], yacc[1][3]} * kRowScale};
            const float* abrow = AB + n * SLDK * 2;
            // software pipeline by node pair: the loads of pair j + 1 are issued before the arithmetic of pair j; the register
            // fence after it keeps hipcc from stacking all 48 b128 loads (192 VGPRs) in front of the arithmetic
            f32x4 ab[2], ua[2][2], ub[2][2];                          // [buffer][node of the pair]
            auto load_pair = [&](int j2, int buf) {
                ab[buf] = *reinterpret_cast<const f32x4*>(&abrow[4 * j2]);              // (r, b) of nodes 2 j2, 2 j2 + 1
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int i = 2 * j2 + e;
                    ua[buf][e] = *reinterpret_cast<const f32x4*>(&UWs[i * 32 + 4 * q]);
                    ub[buf][e] = *reinterpret_cast<const f32x4*>(&UWs[i * 32 + 16 + 4 * q]);
                }
            };
            load_pair(0, 0);
            static_for<0, HRL / 2>([&](auto jc) {
                constexpr int j2 = decltype(jc)::value, buf = j2 & 1;
                if constexpr (j2 + 1 < HRL / 2) load_pair(j2 + 1, buf ^ 1);
                static_for<0, 2>([&](auto ec) {
                    constexpr int e = decltype(ec)::value, i = 2 * j2 + e;
                    if constexpr (i >= 1) {                                             // node 0 is the robot slot
                        const f32x2 rb = f32x2{ab[buf][2 * e], ab[buf][2 * e + 1]};       // (2^-110 r_i, b_i): one register pair
                        const f32x2 u2[4] = {f32x2{ua[buf][e][0], ua[buf][e][1]}, f32x2{ua[buf][e][2], ua[buf][e][3]},
                                             f32x2{ub[buf][e][0], ub[buf][e][1]}, f32x2{ub[buf][e][2], ub[buf][e][3]}};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            acc[k] = pk_fma_hi(rb, pk_fma_lo_clamp(rb, u2[k], y2[k]), acc[k]);
                        }
                    }
                });
                asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]) :: "memory");
            });
            tp4[0] = f32x4{acc[0][0], acc[0][1], acc[1][0], acc[1][1]} * kRowUnscale;
            tp4[1] = f32x4{acc[2][0], acc[2][1], acc[3][0], acc[3][1]} * kRowUnscale;
        } else {
            const int hh = lane >> 5, f = lane & 31;
            constexpr int HRV = HR < 16 * NT ? HR : 16 * NT;      // the table holds 16*NT rows per child
            const int n_pairs = (n_valid + 1) >> 1;
            for (int pair = 0; pair < n_pairs; ++pair) {
                const int lc = 2 * pair + hh;                                      // child within the tile
                const float* sc_mine = AB + (lc * SLD + (lane & 15)) * 2;
                f32x2 ab[NT];
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) ab[tt] = *reinterpret_cast<const f32x2*>(&sc_mine[32 * tt]);
                const float yv = Y0[lc * XLD + f];
                float rp[4] = {0.f, 0.f, 0.f, 0.f};
                static_for<0, (HRV + 2) / 4>([&](auto gc) {
                    constexpr int i0 = 1 + 4 * decltype(gc)::value;
                    float tv[4];
                    static_for<0, 4>([&](auto kc) {
                        constexpr int ii = i0 + decltype(kc)::value;
                        if constexpr (ii < HRV) tv[ii - i0] = dpp_rowbcast_mul<(ii & 15)>(ab[ii >> 4][1], yv);
                    });
                    static_for<0, 4>([&](auto kc) {
                        constexpr int ii = i0 + decltype(kc)::value;
                        if constexpr (ii < HRV) tv[ii - i0] = dpp_rowbcast_fmac<(ii & 15)>(ab[ii >> 4][0], uw4[ii >> 2][ii & 3], tv[ii - i0]);
                    });
                    static_for<0, 4>([&](auto kc) {
                        constexpr int ii = i0 + decltype(kc)::value;
                        if constexpr (ii < HRV) rp[ii - i0] += relu1(tv[ii - i0]);
                    });
                });
                Y0[lc * XLD + f] = (rp[0] + rp[1]) + (rp[2] + rp[3]);             // t_c without the robot-row / skip terms
            }
        }
        __builtin_amdgcn_wave_barrier();
        load_fence();
        PHASE_MARK_ALT(!full, 4);

        // ---------------- robot row: H1_0 = relu(T_0 W1)(+x0), t_c += p00 * H1_0 ---------------------------------------
        f32x4 tin[2], hp[2];
        {
            f32x4 o[2] = {zero4(), zero4()};
            if constexpr (BX) {
                f32x4 tb[2];
#pragma unroll
                for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                    for (int r = 0; r < 4; ++r) tb[ft][r] = fmaf(p00, xacc[ft][r], t0h[ft][r]);      // T_0 = p_c Xh + p_c[0] x0_c
                layer_mfma_b6<XD, XD, false>(w1, tb, o, lane);
            } else {
#pragma unroll
            for (int ft = 0; ft < 2; ++ft) {
                load_fence();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float tb = fmaf(p00, xacc[ft][r], t0h[ft][r]);      // T_0 = p_c Xh + p_c[0] x0_c
#pragma unroll
                    for (int ot = 0; ot < 2; ++ot)
                        o[ot] = mfma4(w1[(16 * ft + 4 * q + r) * WLD + 16 * ot + n], tb, o[ot]);
                }
            }
            load_fence();
            }
#pragma unroll
            for (int ot = 0; ot < 2; ++ot) {
                const f32x4 tp = PK ? tp4[ot] : *reinterpret_cast<const f32x4*>(&Y0[n * XLD + 16 * ot + 4 * q]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float hv = relu1(o[ot][r]);
                    if (SKIP) hv += xacc[ot][r];
                    hp[ot][r] = hv;
                    tin[ot][r] = fmaf(p00, hv, SKIP ? tp[r] + t0h[ot][r] : tp[r]);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();      // the next tile's Y0 / AB writes stay behind this tile's reads
        PHASE_MARK(5);
        if (ti + 1 == t1 && wi_next < n_items) item_loads(wi_next);     // next item's loads fly under this tile's head

        if (!full && !a.inline_partial) {
            // partial last tile: leave the rows [t_c | H1_0] for the tile-packed head pass
            if (n < a.rem) {
                float* out = a.rows_left + ((size_t)p * a.rem + n) * 64;
#pragma unroll
                for (int ot = 0; ot < 2; ++ot) {
                    *reinterpret_cast<f32x4*>(out + 16 * ot + 4 * q) = tin[ot];
                    *reinterpret_cast<f32x4*>(out + 32 + 16 * ot + 4 * q) = hp[ot];
                }
            }
            if (a.head_early) {                                    // my rows have landed: one count per row, released to the workgroup
                wait_vmcnt0();
                asm volatile("" ::: "memory");
                if (lane == 0) __hip_atomic_fetch_add(rows_arrivals, a.rem, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            continue;
        }

        // ---------------- last GCN layer on the robot row + value head: one register-resident MFMA chain -------------------
        await_image();
        if (a.prio & 2) __builtin_amdgcn_s_setprio(2);
        const float v = head_chain<LO, D1, D2, D3, SKIP, BX>(lds, tin, hp, lane);
        if (a.prio & 2) { if ((a.prio & 1) && wave >= 4) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
        if (q == 0 && c < A) a.value[(size_t)p * A + c] = v + hb4;
        PHASE_MARK(6);
      }
    }
    await_image();                       // waves without a head of their own (no items, partial tiles only)
    if (a.rem && !a.inline_partial) {
        // Rows of this workgroup's partial tiles (its own parents, all written by waves of THIS workgroup): scored here,
        // tile-packed over parents -- 16 parents' `stop` children fill one head tile exactly, so the head never multiplies
        // padding columns and the path needs no second launch.
        // Who scores them (RGL_FUSED_HEAD_EARLY): the waves that run out of items FIRST take the packed tiles, one at a time, while
        // the others still work -- a partial tile is the first tile of its item, so the rows are there long before (rows_arrivals
        // says when: no barrier).  Measured, the waves of a workgroup wait 21 k / 26 k cycles on average for its slowest (launches
        // of 2048 / 4096 parents), and the pass -- 11 k cycles on ONE wave behind a barrier, the form RGL_FUSED_HEAD_EARLY=0 keeps:
        // straight-line code that runs once per launch and is fetched as it goes, on rows that cross the barrier before their
        // loads can start -- fits into that wait (profiles/stop_child_ab.txt).  The values do not depend on the wave that
        // computes them.
        const int n_rows = k_b * a.rem;
        const bool early = a.head_early != 0;
        auto take_tile = [&]() {
            int tt = 0;
            if (lane == 0) tt = __hip_atomic_fetch_add(packed_taken, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return __builtin_amdgcn_readfirstlane(tt);
        };
        PHASE_MARK(0);
        if (!early) __syncthreads();
        PHASE_MARK(0);
        for (int tt = early ? take_tile() : wave; 16 * tt < n_rows; tt = early ? take_tile() : tt + kFusedWaves) {
            if (early) {
                while (__hip_atomic_load(rows_arrivals, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < n_rows) __builtin_amdgcn_s_sleep(1);
                asm volatile("" ::: "memory");
            }
            const int i = 16 * tt + n;
            const bool valid = i < n_rows;
            const int lp = valid ? i / a.rem : 0, k = valid ? i - lp * a.rem : 0;
            const int p = p_first + lp;
            const float* row = a.rows_left + ((size_t)p * a.rem + k) * 64;
            f32x4 tin[2], hp[2];
#pragma unroll
            for (int ot = 0; ot < 2; ++ot) {
                tin[ot] = valid ? *reinterpret_cast<const f32x4*>(row + 16 * ot + 4 * q) : zero4();
                hp[ot] = valid ? *reinterpret_cast<const f32x4*>(row + 32 + 16 * ot + 4 * q) : zero4();
            }
            const float v = head_chain<LO, D1, D2, D3, SKIP, BX>(lds, tin, hp, lane);
            if (valid && q == 0) a.value[(size_t)p * A + 16 * a.n_full + k] = v + hb4;
        }
    }
    if (a.tail.enabled) {
        // The search's bookkeeping for the parents this workgroup owns (rgl_tail.h): every value of theirs was written by a wave
        // of this workgroup, so a workgroup barrier is all the synchronisation there is.  One wave per parent selects; at the
        // deepest level the workgroup owns the parents of whole roots and walks the back-up chain up to the root decision.
        PHASE_MARK(7);                   // the tile-packed pass: what its waves spend on it (the others: nothing)
        __syncthreads();
        PHASE_MARK(0);                   // ... and with the loop top, what a wave waits at the barriers behind its items
        static_assert(fused_scratch_floats(HR, NT, SOFT) >= kTailLdsInts, "the wave's scratch holds the select step's tables");
        int* kl = reinterpret_cast<int*>(WS);                    // the wave's scratch is free now
        for (int lp = wave; lp < k_b; lp += kFusedWaves) tail_select(a.tail, p_first + lp, kl);
        if (a.tail.chain) {
            const int W = a.tail.W, lvl = a.tail.level;
            int per_deep = 1;
            for (int l = 0; l < lvl; ++l) per_deep *= W;        // parents of one root at this (the deepest) level
            const int r_first = p_first / per_deep, n_roots = k_b / per_deep;
            int per_l = per_deep;
            for (int l = lvl - 1; l >= 1; --l) {
                per_l /= W;
                __syncthreads();                                 // level l + 1's back-up values are in place
                for (int i = tid; i < n_roots * per_l; i += nthreads) tail_backup(a.tail, l, r_first * per_l + i);
            }
            __syncthreads();
            for (int base = 0; base < n_roots * kRootLanes; base += nthreads) {
                const int i = base + tid, bl = i / kRootLanes;
                tail_root(a.tail, r_first + bl, i % kRootLanes, bl < n_roots);
            }
        }
    }
    PHASE_FLUSH();
}

template <int HR, int NT, bool SKIP, bool SOFT, bool BX = false, bool PRO = false>
int launch_fused_ts(const FusedPlan& pl, hipStream_t st) {
    // a form whose LDS exceeds a CU has no kernel: plan_fused refuses such a plan by the same function (rgl_fused.h lists the forms)
    if constexpr (!fused_form_fits(HR, NT, SOFT, BX)) return RGL_ERR_BAD_MODE;
    else {
    auto kern = children_fused_kernel<HR, NT, SKIP, SOFT, 32, 100, 100, BX, PRO>;
    // pl.lds_bytes is this form's fused_lds_floats (plan_fused): launch_lds raises the kernel's attribute for every compiled form
    static_assert(fused_lds_floats(HR, NT, SOFT, BX) * sizeof(float) > rgl::kLdsBytesWithoutAttribute, "the weight image alone is larger");
    PrologueArgs<PRO> pa{};
    if constexpr (PRO) {
        pa.scene = pl.pro->scene;
        pa.children = pl.pro->children;
    }
    // persistent, one 8-wave workgroup per CU (LDS-bound)
    return rgl::launch_lds(kern, dim3(pl.grid), dim3(kFusedWaves * 64), pl.lds_bytes, st, pl.a, pa);
    }
}

template <int HR, int NT, bool SKIP>
int launch_fused_t(const FusedPlan& pl, hipStream_t st) {
    if (pl.bx) return pl.a.sim == SIM_SOFTMAX ? launch_fused_ts<HR, NT, SKIP, true, true>(pl, st)
                                              : launch_fused_ts<HR, NT, SKIP, false, true>(pl, st);
    return pl.a.sim == SIM_SOFTMAX ? launch_fused_ts<HR, NT, SKIP, true>(pl, st) : launch_fused_ts<HR, NT, SKIP, false>(pl, st);
}

}  // namespace

int rgl::fused::launch_fused(const FusedPlan& pl, bool skip, hipStream_t st) {
    if (pl.pro)          // the only instantiations with the prologue (prologue_form)
        return skip ? launch_fused_ts<kPrologueHR, kPrologueNT, true, true, true, true>(pl, st)
                    : launch_fused_ts<kPrologueHR, kPrologueNT, false, true, true, true>(pl, st);
    switch (pl.hr) {
        case 8: return skip ? launch_fused_t<8, 1, true>(pl, st) : launch_fused_t<8, 1, false>(pl, st);
        case 20: return pl.nt == 1 ? (skip ? launch_fused_t<20, 1, true>(pl, st) : launch_fused_t<20, 1, false>(pl, st))
                                   : (skip ? launch_fused_t<20, 2, true>(pl, st) : launch_fused_t<20, 2, false>(pl, st));
        default: return skip ? launch_fused_t<32, 2, true>(pl, st) : launch_fused_t<32, 2, false>(pl, st);
    }
}

#ifdef RGL_PHASE_TIMING
extern "C" int rgl_debug_read_fused_phase_cycles(unsigned long long* out16, int reset) {
    return rgl::read_phase_cycles(HIP_SYMBOL(g_phase_cycles), out16, reset);
}
#endif
