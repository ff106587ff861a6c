// rgl_graph_kernel.h -- the tile pipeline's persistent graph kernel (rgl_tile_pipeline.hip, steps 2 and 4) and its launcher.  Included
// by the family units only (rgl_graph_plain.hip, rgl_graph_cos.hip, rgl_graph_lw.hip: each instantiates launch_graph_family for its
// COS / LW pair and nothing else) and, for GraphLds, by the planner (rgl_graph.hip), which instantiates no kernel.
#pragma once
#include "rgl_tile_mm.h"
#include "rgl_tiles.h"

using namespace rgl::tiles;

namespace {

// ------------------------------------------------------------------------------------------------
// the graph block: one workgroup per scene
// ------------------------------------------------------------------------------------------------
// sum / max over the 16 lanes of a DPP row, every lane gets it
__device__ __forceinline__ float dpp_f(float x, int ctrl) {
    switch (ctrl) {
        case 0: return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xf, 0xf, true));     // quad_perm [1,0,3,2]
        case 1: return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x4E, 0xf, 0xf, true));     // quad_perm [2,3,0,1]
        case 2: return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x141, 0xf, 0xf, true));    // row_half_mirror
        default: return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x140, 0xf, 0xf, true));   // row_mirror
    }
}
__device__ __forceinline__ float row16_sum(float x) {
#pragma unroll
    for (int c = 0; c < 4; ++c) x += dpp_f(x, c);
    return x;
}
__device__ __forceinline__ float row16_maxf(float x) {
#pragma unroll
    for (int c = 0; c < 4; ++c) x = fmaxf(x, dpp_f(x, c));
    return x;
}

// LDS of a workgroup: weights  Wa | W_0 .. W_{L-1}  ([X][FLD] each, FLD = X + 2: row-indexed A-operand reads hit 32 distinct banks),
// then the scene's   X, dH, dZ, dT, T_0 .. T_{L-1}, H_1 .. H_{L-1}   ([NP][FLD], NP = N rounded up to 4: the padding rows stay zero,
// so node-indexed k loops need no guards)   and   A, dA   ([NP][ALD]).  A forward-only launch has no dH, dZ, dA.
template <int NT, int XT>
struct GraphLds {
    static constexpr int XW = XT * 16, FLD = XW + 2, ALD = NT * 16 + 2;
    static __host__ __device__ constexpr int scene_floats(int N, int L, bool bwd, bool lw = false) {     // lw: an adjacency per layer
        const int NP = (N + 3) & ~3;
        return ((bwd ? 4 : 2) + L + (L - 1)) * NP * FLD + ((lw ? L : 1) + (bwd ? 1 : 0)) * NP * ALD;
    }
    static __host__ __device__ constexpr int weight_floats(int L) { return (1 + L) * XW * FLD; }
};

// A scene is a chain of ~20 small products (8 MFMAs per 16 x 16 tile each), every one needing the whole result of the one before:
// a wave per scene spends its time in LDS round trips.  So the 2 NT waves of a workgroup share ONE scene: each product's output tiles
// are dealt to the waves -- an [N][X] result has NT x XT tiles (X = 16 XT features: 32 shipped, 64 supported), a 1 x XT/2 block per
// wave; [N][N] results NT x NT; the [X][X] weight gradients XT x XT over four waves -- with a workgroup barrier between phases, and
// several workgroups per CU overlap each other's barriers.  The weight gradients stay in the accumulators of the waves that own
// their tiles over all scenes of the workgroup (one slab per workgroup).
// COS: the build with the cosine family's passes (norm 4 / 5).  A build of its own, so that the shipped similarity functions keep
// the register allocation they had without them (the passes cost the L = 2 backward 36 more bytes of scratch per lane otherwise).
// LW (round 6): layerwise graphs (graph_model.py:118-122) -- the adjacency is recomputed from every layer's input, A_l =
// softmax(H_l Wa H_l^T): L adjacency buffers in LDS, and the backward pass goes through the similarity block inside the layer loop
// (dA_l, the softmax, dG_l = dS_l H_l, dH_l += dS_l^T G_l + dG_l Wa^T, dWa += H_l^T dG_l) before it forms the next layer's dZ.
// The softmax normalisations (embedded_gaussian, gaussian) and the squared one; equal_attention / diagonal adjacencies are
// constants, so their layerwise graphs ARE the one-adjacency form; the cosine family and the pair-MLP similarity of a layerwise
// graph stay on the per-scene kernel.
// (two workgroups per CU at least for the layerwise form: its backward carries the similarity block's accumulators through the
// layer loop and spills 50-88 registers under the four-workgroup budget of the one-adjacency form)
template <int NT, int XT, int L, bool BWD, bool COS, bool LW = false>
__global__ __launch_bounds__(NT * 128, LW ? 2 : ((NT == 2 && XT == 2) ? 4 : (NT == 1 ? 3 : 2))) void graph_kernel(const GraphArgs a) {
    static_assert(!(LW && COS), "layerwise graphs: the softmax and squared normalisations only");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using Lds = GraphLds<NT, XT>;
    constexpr int XW = Lds::XW, FLD = Lds::FLD, ALD = Lds::ALD;
    constexpr int W = 2 * NT;                        // waves
    constexpr int XTW = XT / 2;                      // column tiles of an [N][X] result per wave
    constexpr int NTW = NT >= 2 ? NT / 2 : 1;        // column tiles of an [N][N] result per wave
    constexpr int GM = XT / 2, GN = W >= 4 ? XT / 2 : XT;        // this wave's block of an [X][X] result, in tiles
    constexpr int PF = XW / 8;                       // elements per thread of a scene's [NP][X] rows (NP X / 64 W <= X / 8)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, kq = lane >> 4;
    const int N = a.N, NP = (N + 3) & ~3, NK = NP >> 2, last = NP - 1;
    const bool embedded = a.w_a != nullptr;
    float* Wa = lds;
    float* Wl = lds + XW * FLD;
    for (int idx = threadIdx.x; idx < XW * XW; idx += W * 64) {
        const int k = idx / XW, c = idx % XW;
        Wa[k * FLD + c] = embedded ? a.w_a[idx] : 0.f;
#pragma unroll
        for (int l = 0; l < L; ++l) Wl[l * XW * FLD + k * FLD + c] = a.Ws[l][idx];
    }
    float* base = lds + Lds::weight_floats(L);
    const int U = NP * FLD;
    float* X = base;
    float* dT = X + U;                 // G = X Wa lives here in the forward sweep
    float* T = dT + U;                 // [L]
    float* Hs = T + L * U;             // [L - 1]: H_1 ..
    float* A = Hs + (L - 1) * U;       // LW: A_0 .. A_{L-1}
    float* dA = A + (LW ? L : 1) * NP * ALD;          // backward only from here
    float* dH = dA + NP * ALD;
    float* dZ = dH + U;
    auto Hl = [&](int l) { return l == 0 ? X : Hs + (l - 1) * U; };
    // this wave's block of an [N][X] result, of an [N][N] result, of an [X][X] result
    const int fm = (wave >> 1) * 16, fn = (wave & 1) * XTW * 16;
    const int am = fm, an = (wave & 1) * NTW * 16;
    const bool a_on = (wave & 1) * NTW < NT;
    const int gm = (W >= 4 ? (wave >> 1) : wave) * GM * 16, gn = W >= 4 ? (wave & 1) * GN * 16 : 0;
    const bool g_on = W >= 4 ? wave < 4 : true;
    const int frow = fm + 4 * kq;      // element r of this lane in a tile of its [N][X] block: row frow + r, column fn + 16 nt + l16

    f32x4 gWa[GM][GN], gW[L][GM][GN];
    clear<GM, GN>(gWa);
#pragma unroll
    for (int l = 0; l < L; ++l) clear<GM, GN>(gW[l]);
    // X (and the upstream gradient) of a scene are fetched into registers one scene ahead
    float xp[PF], dp[PF];
    auto prefetch = [&](int s) {
        const bool ok = s < a.S;
        const int sc = ok ? s : 0;
        const float* xr = a.Xr + (size_t)sc * a.xr_stride;
        const float* xh = a.Xh + (size_t)(sc / a.spc) * a.xh_stride - XW;       // row i >= 1 at xh + i * XW
        const float* dg = BWD ? a.dHL + (size_t)sc * N * XW : nullptr;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int idx = threadIdx.x + u * W * 64;
            xp[u] = (ok && idx < N * XW) ? (idx < XW ? xr[idx] : xh[idx]) : 0.f;
            if constexpr (BWD) dp[u] = (ok && idx < N * XW) ? dg[idx] : 0.f;
        }
    };
    prefetch(blockIdx.x);
    __syncthreads();

    for (int s = blockIdx.x; s < a.S; s += gridDim.x) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {      // rows N .. NP-1 zero
            const int idx = threadIdx.x + u * W * 64;
            if (idx < NP * XW) {
                X[(idx / XW) * FLD + idx % XW] = xp[u];
                if constexpr (BWD) dH[(idx / XW) * FLD + idx % XW] = dp[u];
            }
        }
        prefetch(s + gridDim.x);
        __syncthreads();
        float* G = dT;
        // out[row][fn ..] of this wave's [N][X] block = v, zero in the padding rows
        auto put = [&](float* out, const f32x4 (&acc)[1][XTW]) {
#pragma unroll
            for (int nt = 0; nt < XTW; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (frow + r < NP) out[(frow + r) * FLD + fn + nt * 16 + l16] = frow + r < N ? acc[0][nt][r] : 0.f;
        };
        auto make_G = [&](const float* Hin) {          // G = H Wa of the rows the similarity is taken over (X; LW: H_l)
            f32x4 acc[1][XTW];
            clear<1, XTW>(acc);
            mm<1, XTW, 8>(acc, XW / 4, [&](int i, int k) { return Hin[min(fm + i, last) * FLD + k]; },
                          [&](int k, int j) { return Wa[k * FLD + fn + j]; });
            put(G, acc);
        };
        const int norm = a.norm;
        // A_l of a layerwise graph: S = (H_l Wa) H_l^T (gaussian, squared: H_l H_l^T), its row normalisation; ends with a barrier
        auto make_A_lw = [&](const float* Hc, float* Al) {
            if (embedded) {
                make_G(Hc);
                __syncthreads();
            }
            const float* GXl = embedded ? G : Hc;
            if (a_on) {
                f32x4 acc[1][NTW];
                clear<1, NTW>(acc);
                mm<1, NTW, 8>(acc, XW / 4, [&](int i, int k) { return GXl[min(am + i, last) * FLD + k]; },
                              [&](int k, int j) { return Hc[min(an + j, last) * FLD + k]; });
                each<1, NTW>(acc, [&](int i, int j, float v, int, int, int) {
                    const int row = am + i, col = an + j;
                    if (row < NP) Al[row * ALD + col] = (row < N && col < N) ? v : 0.f;
                });
            }
            __syncthreads();
            for (int row = wave * 4 + kq; norm == 1 && row < N; row += W * 4) {       // squared: as in the one-adjacency form below
                float* r = Al + row * ALD;
                float sv[NT], w[NT], sum = 0.f;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    sv[j] = l16 + 16 * j < N ? r[l16 + 16 * j] : 0.f;
                    w[j] = sv[j] * sv[j];
                    sum += w[j];
                }
                sum = row16_sum(sum);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (l16 + 16 * j < N) r[l16 + 16 * j] = copysignf(w[j] / sum, sv[j]);
                if (l16 == 0) r[NT * 16] = sum;
            }
            for (int row = wave * 4 + kq; norm == 0 && row < N; row += W * 4) {
                float* r = Al + row * ALD;
                float v[NT], mx = -3.4e38f;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    v[j] = l16 + 16 * j < N ? r[l16 + 16 * j] : -3.4e38f;
                    mx = fmaxf(mx, v[j]);
                }
                mx = row16_maxf(mx);
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    v[j] = l16 + 16 * j < N ? expf(v[j] - mx) : 0.f;
                    sum += v[j];
                }
                sum = row16_sum(sum);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (l16 + 16 * j < N) r[l16 + 16 * j] = v[j] / sum;
            }
            __syncthreads();
        };
        const bool cosine = COS && norm >= 4;
        const bool from_s = norm <= 1 || cosine;        // the adjacency is a function of S (it is a constant otherwise)
        // squared similarity: A is kept SIGNED in LDS -- sign(S_ij) |A_ij| -- and the row's Z_i = sum_j S_ij^2 in the row's padding
        // column, so that the backward pass gets S_ij = sign sqrt(|A_ij| Z_i) back without a buffer of its own; every consumer of
        // A reads it through aval()
        auto aval = [&](float x) { return norm == 1 ? fabsf(x) : x; };
        if (embedded && !LW) {
            make_G(X);
            __syncthreads();
        }
        const float* GX = embedded ? G : X;
        if (!from_s) {
            const float c = norm == 2 ? 1.f / (float)N : 0.f;
            for (int idx = threadIdx.x; idx < NP * ALD; idx += W * 64) {
                const int row = idx / ALD, col = idx - row * ALD;
                A[idx] = (row < N && col < N) ? (norm == 2 ? c : (row == col ? 1.f : 0.f)) : 0.f;
            }
        }
        if (a_on && from_s && !LW) {   // S = G X^T   (graph_model.py:64-69)
            f32x4 acc[1][NTW];
            clear<1, NTW>(acc);
            mm<1, NTW, 8>(acc, XW / 4, [&](int i, int k) { return GX[min(am + i, last) * FLD + k]; },
                          [&](int k, int j) { return X[min(an + j, last) * FLD + k]; });
            each<1, NTW>(acc, [&](int i, int j, float v, int, int, int) {
                const int row = am + i, col = an + j;
                if (row < NP) A[row * ALD + col] = (row < N && col < N) ? v : 0.f;
            });
        }
        __syncthreads();
        // squared (graph_model.py:86-89): w = S^2 over its row sum
        for (int row = wave * 4 + kq; norm == 1 && row < N; row += W * 4) {
            float* r = A + row * ALD;
            float sv[NT], w[NT], sum = 0.f;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                sv[j] = l16 + 16 * j < N ? r[l16 + 16 * j] : 0.f;
                w[j] = sv[j] * sv[j];
                sum += w[j];
            }
            sum = row16_sum(sum);
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (l16 + 16 * j < N) r[l16 + 16 * j] = copysignf(w[j] / sum, sv[j]);
            if (l16 == 0) r[NT * 16] = sum;
        }
        // cosine family (graph_model.py:70-79): the norms of S's ROWS first (kept in the rows' padding column, like the squared sums:
        // the backward pass needs them again), then C_ij = S_ij / (m_i m_j) and, cosine_softmax, its row softmax in the same pass
        if constexpr (COS) {
        for (int row = wave * 4 + kq; cosine && row < N; row += W * 4) {
            float* r = A + row * ALD;
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float v = l16 + 16 * j < N ? r[l16 + 16 * j] : 0.f;
                sum = fmaf(v, v, sum);
            }
            sum = row16_sum(sum);
            if (l16 == 0) r[NT * 16] = sqrtf(sum);
        }
        if (cosine) __syncthreads();
        for (int row = wave * 4 + kq; cosine && row < N; row += W * 4) {
            float* r = A + row * ALD;
            const float mi = r[NT * 16];
            float v[NT], mx = -3.4e38f;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = l16 + 16 * j;
                v[j] = col < N ? r[col] / (mi * A[col * ALD + NT * 16]) : -3.4e38f;
                mx = fmaxf(mx, v[j]);
            }
            if (norm == 5) {
                mx = row16_maxf(mx);
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    v[j] = l16 + 16 * j < N ? expf(v[j] - mx) : 0.f;
                    sum += v[j];
                }
                sum = row16_sum(sum);
#pragma unroll
                for (int j = 0; j < NT; ++j) v[j] /= sum;
            }
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (l16 + 16 * j < N) r[l16 + 16 * j] = v[j];
        }
        }
        // row softmax: 16 lanes per row, four rows per wave and pass
        for (int row = wave * 4 + kq; !LW && norm == 0 && row < N; row += W * 4) {
            float* r = A + row * ALD;
            float v[NT], mx = -3.4e38f;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                v[j] = l16 + 16 * j < N ? r[l16 + 16 * j] : -3.4e38f;
                mx = fmaxf(mx, v[j]);
            }
            mx = row16_maxf(mx);
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                v[j] = l16 + 16 * j < N ? expf(v[j] - mx) : 0.f;
                sum += v[j];
            }
            sum = row16_sum(sum);
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (l16 + 16 * j < N) r[l16 + 16 * j] = v[j] / sum;
        }
        __syncthreads();
        unsigned mask[L];
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const float* Hc = Hl(l);
            float* Tl = T + l * U;
            const float* Al = LW ? A + l * NP * ALD : A;
            if constexpr (LW) make_A_lw(Hc, A + l * NP * ALD);
            {   // T_l = A H_l
                f32x4 acc[1][XTW];
                clear<1, XTW>(acc);
                mm<1, XTW, 8>(acc, NK, [&](int i, int k) { return aval(Al[min(fm + i, last) * ALD + k]); },
                              [&](int k, int j) { return Hc[k * FLD + fn + j]; });
                put(Tl, acc);
            }
            __syncthreads();
            {   // H_{l+1} = relu(T_l W_l) (+ H_l)
                f32x4 acc[1][XTW];
                clear<1, XTW>(acc);
                const float* Wc = Wl + l * XW * FLD;
                mm<1, XTW, 8>(acc, XW / 4, [&](int i, int k) { return Tl[min(fm + i, last) * FLD + k]; },
                              [&](int k, int j) { return Wc[k * FLD + fn + j]; });
                unsigned bits = 0;
                const bool keep = l + 1 < L;                    // the next layer's input
                float* Hn = keep ? Hs + l * U : nullptr;
                float* out = (!BWD && !keep) ? (a.hl_row0 ? a.HL + (size_t)s * XW : a.HL + (size_t)s * N * XW) : nullptr;
#pragma unroll
                for (int nt = 0; nt < XTW; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = frow + r, col = fn + nt * 16 + l16;
                        const float v = acc[0][nt][r];
                        if (v > 0.f) bits |= 1u << (nt * 4 + r);
                        if (row < NP) {
                            const float h = row < N ? fmaxf(v, 0.f) + (a.skip ? Hc[row * FLD + col] : 0.f) : 0.f;
                            if (keep) Hn[row * FLD + col] = h;
                            else if (out && row < (a.hl_row0 ? 1 : N)) out[row * XW + col] = h;
                            // the top layer's dZ = dH_L where its ReLU is open, straight from here
                            if constexpr (BWD)
                                if (!keep) dZ[row * FLD + col] = (v > 0.f && row < N) ? dH[row * FLD + col] : 0.f;
                        }
                    }
                mask[l] = bits;
            }
            __syncthreads();
        }
        if constexpr (BWD) {
            f32x4 dAacc[1][NTW];
            clear<1, NTW>(dAacc);
#pragma unroll
            for (int l = L - 1; l >= 0; --l) {
                const float* Hc = Hl(l);
                const float* Tl = T + l * U;
                const float* Wc = Wl + l * XW * FLD;
                const float* Al = LW ? A + l * NP * ALD : A;
                // dW_l += T_l^T dZ
                if (g_on)
                    mm<GM, GN, 8>(gW[l], NK, [&](int mi, int k) { return Tl[k * FLD + gm + mi]; },
                                  [&](int k, int j) { return dZ[k * FLD + gn + j]; });
                {   // dT = dZ W_l^T
                    f32x4 acc[1][XTW];
                    clear<1, XTW>(acc);
                    mm<1, XTW, 8>(acc, XW / 4, [&](int i, int k) { return dZ[min(fm + i, last) * FLD + k]; },
                                  [&](int k, int j) { return Wc[(fn + j) * FLD + k]; });
                    put(dT, acc);
                }
                __syncthreads();
                // dA += dT H_l^T
                if (a_on)
                    mm<1, NTW, 8>(dAacc, XW / 4, [&](int i, int k) { return dT[min(am + i, last) * FLD + k]; },
                                  [&](int k, int j) { return Hc[min(an + j, last) * FLD + k]; });
                {   // dH_l = A^T dT (+ dH_{l+1} through the skip connection); the next layer's dZ right away
                    f32x4 acc[1][XTW];
                    clear<1, XTW>(acc);
                    mm<1, XTW, 8>(acc, NK, [&](int mi, int k) { return aval(Al[k * ALD + fm + mi]); },
                                  [&](int k, int j) { return dT[k * FLD + fn + j]; });
#pragma unroll
                    for (int nt = 0; nt < XTW; ++nt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = frow + r, col = fn + nt * 16 + l16;
                            if (row < N) {
                                const float d = acc[0][nt][r] + (a.skip ? dH[row * FLD + col] : 0.f);
                                dH[row * FLD + col] = d;
                                // (LW: dH_l is not complete yet -- the similarity block of this layer adds to it below)
                                if (!LW && l > 0) dZ[row * FLD + col] = ((mask[l > 0 ? l - 1 : 0] >> (nt * 4 + r)) & 1u) ? d : 0.f;
                            }
                        }
                }
                __syncthreads();
                if constexpr (LW) {
                    // ---- through A_l = softmax(S_l), S_l = G_l H_l^T, G_l = H_l Wa (gaussian: G_l = H_l)
                    if (a_on)
                        each<1, NTW>(dAacc, [&](int i, int j, float v, int, int, int) {
                            const int row = am + i, col = an + j;
                            if (row < NP) dA[row * ALD + col] = (row < N && col < N) ? v : 0.f;
                        });
                    clear<1, NTW>(dAacc);
                    if (embedded) make_G(Hc);            // into dT's buffer: its readers (dA_l, dH_l) are behind the barrier above
                    __syncthreads();
                    for (int row = wave * 4 + kq; norm == 1 && row < N; row += W * 4) {     // squared: dS = 2 S (dA - sum dA A) / Z
                        float* d = dA + row * ALD;
                        const float* p = Al + row * ALD;
                        const float zi = p[NT * 16];
                        float dv[NT], pv[NT], dot = 0.f;
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
                            const bool ok = l16 + 16 * j < N;
                            dv[j] = ok ? d[l16 + 16 * j] : 0.f;
                            pv[j] = ok ? p[l16 + 16 * j] : 0.f;
                            dot = fmaf(dv[j], fabsf(pv[j]), dot);
                        }
                        dot = row16_sum(dot);
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            if (l16 + 16 * j < N) d[l16 + 16 * j] = 2.f * copysignf(sqrtf(fabsf(pv[j]) / zi), pv[j]) * (dv[j] - dot);
                    }
                    for (int row = wave * 4 + kq; norm == 0 && row < N; row += W * 4) {       // softmax: dS_ij = A_ij (dA_ij - sum_k dA_ik A_ik)
                        float* d = dA + row * ALD;
                        const float* p = Al + row * ALD;
                        float dv[NT], pv[NT], dot = 0.f;
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
                            const bool ok = l16 + 16 * j < N;
                            dv[j] = ok ? d[l16 + 16 * j] : 0.f;
                            pv[j] = ok ? p[l16 + 16 * j] : 0.f;
                            dot = fmaf(dv[j], pv[j], dot);
                        }
                        dot = row16_sum(dot);
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            if (l16 + 16 * j < N) d[l16 + 16 * j] = pv[j] * (dv[j] - dot);
                    }
                    __syncthreads();
                    const float* GXl = embedded ? G : Hc;
                    float* dGl = dZ;                      // dZ_l is spent: dW_l and dT have read it
                    f32x4 dxl[1][XTW];
                    {
                        f32x4 acc[1][XTW];
                        clear<1, XTW>(acc);
                        mm<1, XTW, 8>(acc, NK, [&](int i, int k) { return dA[min(fm + i, last) * ALD + k]; },
                                      [&](int k, int j) { return Hc[k * FLD + fn + j]; });
                        put(dGl, acc);
                        clear<1, XTW>(dxl);
                        mm<1, XTW, 8>(dxl, NK, [&](int mi, int k) { return dA[k * ALD + fm + mi]; },
                                      [&](int k, int j) { return GXl[k * FLD + fn + j]; });
                        if (!embedded) {
#pragma unroll
                            for (int nt = 0; nt < XTW; ++nt)
#pragma unroll
                                for (int r = 0; r < 4; ++r) dxl[0][nt][r] += acc[0][nt][r];
                        }
                    }
                    __syncthreads();
                    if (embedded) {
                        if (g_on)
                            mm<GM, GN, 8>(gWa, NK, [&](int mi, int k) { return Hc[k * FLD + gm + mi]; },
                                          [&](int k, int j) { return dGl[k * FLD + gn + j]; });
                        mm<1, XTW, 8>(dxl, XW / 4, [&](int i, int k) { return dGl[min(fm + i, last) * FLD + k]; },
                                      [&](int k, int j) { return Wa[(fn + j) * FLD + k]; });
                    }
                    __syncthreads();                      // every read of dG_l (in dZ's buffer) is done
#pragma unroll
                    for (int nt = 0; nt < XTW; ++nt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = frow + r, col = fn + nt * 16 + l16;
                            if (row < NP) {
                                const float d = row < N ? dH[row * FLD + col] + dxl[0][nt][r] : 0.f;
                                if (row < N) dH[row * FLD + col] = d;
                                if (l > 0) dZ[row * FLD + col] = ((mask[l > 0 ? l - 1 : 0] >> (nt * 4 + r)) & 1u) ? d : 0.f;
                            }
                        }
                    __syncthreads();
                }
            }
            f32x4 dx[1][XTW];
            clear<1, XTW>(dx);
            if constexpr (!LW) {
            // through the row softmax: dS_ij = A_ij (dA_ij - sum_k dA_ik A_ik)
            if (a_on)
                each<1, NTW>(dAacc, [&](int i, int j, float v, int, int, int) {
                    const int row = am + i, col = an + j;
                    if (row < NP) dA[row * ALD + col] = (row < N && col < N && from_s) ? v : 0.f;      // constant adjacency: dS = 0
                });
            if (embedded) make_G(X);           // dT's buffer is free again
            __syncthreads();
            // through the squared normalisation: dS_ij = 2 S_ij (dA_ij - sum_k dA_ik A_ik) / Z_i, S_ij = sign sqrt(|A_ij| Z_i)
            for (int row = wave * 4 + kq; norm == 1 && row < N; row += W * 4) {
                float* d = dA + row * ALD;
                const float* p = A + row * ALD;
                const float zi = p[NT * 16];
                float dv[NT], pv[NT], dot = 0.f;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const bool ok = l16 + 16 * j < N;
                    dv[j] = ok ? d[l16 + 16 * j] : 0.f;
                    pv[j] = ok ? p[l16 + 16 * j] : 0.f;
                    dot = fmaf(dv[j], fabsf(pv[j]), dot);
                }
                dot = row16_sum(dot);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (l16 + 16 * j < N) d[l16 + 16 * j] = 2.f * copysignf(sqrtf(fabsf(pv[j]) / zi), pv[j]) * (dv[j] - dot);
            }
            for (int row = wave * 4 + kq; (norm == 0 || (COS && norm == 5)) && row < N; row += W * 4) {
                float* d = dA + row * ALD;
                const float* p = A + row * ALD;
                float dv[NT], pv[NT], dot = 0.f;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const bool ok = l16 + 16 * j < N;
                    dv[j] = ok ? d[l16 + 16 * j] : 0.f;
                    pv[j] = ok ? p[l16 + 16 * j] : 0.f;
                    dot = fmaf(dv[j], pv[j], dot);
                }
                dot = row16_sum(dot);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (l16 + 16 * j < N) d[l16 + 16 * j] = pv[j] * (dv[j] - dot);
            }
            if constexpr (COS) if (cosine) {
                // through C_ij = S_ij / (m_i m_j), m_i = sqrt(sum_k S_ik^2):
                //   dS_ij = dC_ij / (m_i m_j) - (r_i + c_i) S_ij / m_i^2,   r_i = sum_j dC_ij C_ij,  c_i = sum_j dC_ji C_ji
                // (m_i enters row i AND column i of C).  S is recomputed into A's buffer -- nothing reads the adjacency after the
                // layer loop -- next to the norms the forward sweep left in the padding column; dA holds dC.
                __syncthreads();
                if (a_on) {
                    f32x4 acc[1][NTW];
                    clear<1, NTW>(acc);
                    mm<1, NTW, 8>(acc, XW / 4, [&](int i, int k) { return X[min(am + i, last) * FLD + k]; },
                                  [&](int k, int j) { return X[min(an + j, last) * FLD + k]; });
                    each<1, NTW>(acc, [&](int i, int j, float v, int, int, int) {
                        const int row = am + i, col = an + j;
                        if (row < NP) A[row * ALD + col] = (row < N && col < N) ? v : 0.f;
                    });
                }
                __syncthreads();
                for (int row = wave * 4 + kq; row < N; row += W * 4) {          // r_i + c_i -> dA's padding column
                    const float mi = A[row * ALD + NT * 16];
                    float e = 0.f;
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const int col = l16 + 16 * j;
                        if (col < N) {
                            const float inv = 1.f / (mi * A[col * ALD + NT * 16]);
                            e = fmaf(dA[row * ALD + col], A[row * ALD + col] * inv, e);
                            e = fmaf(dA[col * ALD + row], A[col * ALD + row] * inv, e);
                        }
                    }
                    e = row16_sum(e);
                    if (l16 == 0) dA[row * ALD + NT * 16] = e;
                }
                __syncthreads();
                for (int row = wave * 4 + kq; row < N; row += W * 4) {
                    float* d = dA + row * ALD;
                    const float mi = A[row * ALD + NT * 16], back = d[NT * 16] / (mi * mi);
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const int col = l16 + 16 * j;
                        if (col < N) d[col] = d[col] / (mi * A[col * ALD + NT * 16]) - back * A[row * ALD + col];
                    }
                }
            }
            __syncthreads();
            // S = G X^T:  dG = dS X ;  dX += dS^T G        G = X Wa:  dWa += X^T dG ;  dX += dG Wa^T     (gaussian: G = X, dX += dG)
            float* dG = dZ;
            {
                f32x4 acc[1][XTW];
                clear<1, XTW>(acc);
                mm<1, XTW, 8>(acc, NK, [&](int i, int k) { return dA[min(fm + i, last) * ALD + k]; },
                              [&](int k, int j) { return X[k * FLD + fn + j]; });
                put(dG, acc);
                clear<1, XTW>(dx);
                mm<1, XTW, 8>(dx, NK, [&](int mi, int k) { return dA[k * ALD + fm + mi]; },
                              [&](int k, int j) { return GX[k * FLD + fn + j]; });
                if (!embedded) {
#pragma unroll
                    for (int nt = 0; nt < XTW; ++nt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) dx[0][nt][r] += acc[0][nt][r];
                }
            }
            __syncthreads();
            if (embedded) {
                if (g_on)
                    mm<GM, GN, 8>(gWa, NK, [&](int mi, int k) { return X[k * FLD + gm + mi]; },
                                  [&](int k, int j) { return dG[k * FLD + gn + j]; });
                mm<1, XTW, 8>(dx, XW / 4, [&](int i, int k) { return dG[min(fm + i, last) * FLD + k]; },
                              [&](int k, int j) { return Wa[(fn + j) * FLD + k]; });
            }
            }
            float* dxr = a.dXr + (size_t)s * a.xr_stride;
            float* dxh = a.dXh + (size_t)s * a.xh_stride - XW;
#pragma unroll
            for (int nt = 0; nt < XTW; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = frow + r, col = fn + nt * 16 + l16;
                    if (row < N) (row == 0 ? dxr : dxh + (size_t)row * XW)[col] = dx[0][nt][r] + dH[row * FLD + col];
                }
            __syncthreads();
        }
    }
    if constexpr (BWD) {
        if (g_on) {
            float* slab = a.slabs + (size_t)blockIdx.x * ((embedded ? 1 : 0) + L) * XW * XW;
            if (embedded) {
                each<GM, GN>(gWa, [&](int i, int j, float v, int, int, int) { slab[(gm + i) * XW + gn + j] = v; });
                slab += XW * XW;
            }
#pragma unroll
            for (int l = 0; l < L; ++l)
                each<GM, GN>(gW[l], [&](int i, int j, float v, int, int, int) { slab[l * XW * XW + (gm + i) * XW + gn + j] = v; });
        }
    }
}

template <int NT, int XT, int L, bool BWD, bool COS, bool LW = false>
int launch_graph_kernel(const GraphArgs& ga, size_t lds, int grid, hipStream_t st) {
    auto kern = graph_kernel<NT, XT, L, BWD, COS, LW>;
    return rgl::launch_lds(kern, dim3(grid), dim3(NT * 128), lds, st, ga);
}

// graph_kernel<4, 4, 3, true, ..> is never launched: 64 features in three layers with the backward's buffers need more than the LDS
// of a CU already at the smallest N that takes four node tiles (plan_graph answers an empty plan), so it is not compiled either
static_assert((size_t)(GraphLds<4, 4>::weight_floats(3) + GraphLds<4, 4>::scene_floats(33, 3, true, false)) * sizeof(float) >
                  (size_t)rgl::kLdsBytesPerCu,
              "graph_kernel<4, 4, 3, true, ..>: launch_graph_nxl assumes that no scene of N > 32 fits the LDS of a CU");
template <int NT, int XT, int L, bool COS, bool LW>
int launch_graph_nxl(const GraphArgs& ga, bool bwd, size_t lds, int grid, hipStream_t st) {
    // the two forms that are not compiled are never asked for (tiles_cover, plan_graph): an error if they are
    if constexpr (LW && !(XT == 2 && NT <= 2)) {  // layerwise graphs: the softmax / squared normalisations, up to 32 nodes of 32 features (tiles_cover)
        return RGL_ERR_BAD_MODE;
    } else if constexpr (NT == 4 && XT == 4 && L == 3) {
        return bwd ? RGL_ERR_LDS : launch_graph_kernel<NT, XT, L, false, COS, LW>(ga, lds, grid, st);
    } else {
        return bwd ? launch_graph_kernel<NT, XT, L, true, COS, LW>(ga, lds, grid, st)
                   : launch_graph_kernel<NT, XT, L, false, COS, LW>(ga, lds, grid, st);
    }
}
template <int NT, int XT, bool COS, bool LW>
int launch_graph_nx(const GraphArgs& ga, int L, bool bwd, size_t lds, int grid, hipStream_t st) {
    switch (L) {
        case 1: return launch_graph_nxl<NT, XT, 1, COS, LW>(ga, bwd, lds, grid, st);
        case 2: return launch_graph_nxl<NT, XT, 2, COS, LW>(ga, bwd, lds, grid, st);
        default: return launch_graph_nxl<NT, XT, 3, COS, LW>(ga, bwd, lds, grid, st);
    }
}
// every instantiation of one family (GraphForm::family: COS / LW), by node tiles, feature tiles, layers and direction
template <bool COS, bool LW>
int launch_graph_family(const GraphArgs& ga, const GraphForm& f, int L, bool bwd, size_t lds, int grid, hipStream_t st) {
    switch (f.nt * 10 + f.xt) {
        case 12: return launch_graph_nx<1, 2, COS, LW>(ga, L, bwd, lds, grid, st);
        case 22: return launch_graph_nx<2, 2, COS, LW>(ga, L, bwd, lds, grid, st);
        case 42: return launch_graph_nx<4, 2, COS, LW>(ga, L, bwd, lds, grid, st);
        case 14: return launch_graph_nx<1, 4, COS, LW>(ga, L, bwd, lds, grid, st);
        case 24: return launch_graph_nx<2, 4, COS, LW>(ga, L, bwd, lds, grid, st);
        default: return launch_graph_nx<4, 4, COS, LW>(ga, L, bwd, lds, grid, st);
    }
}

}  // namespace
