// rgl_fused_image.hip -- the packed weight image of the fused children kernel (rgl_fused_kernel.hip; FusedLds, rgl_mlp_chain.h): the
// packing kernel, and the ABI calls with which a caller of fixed weights packs it once.
#include "rgl_fused.h"

using namespace rgl::fused;

namespace {

// Both weight images in global memory, in exactly the LDS layouts the kernels use: built ONCE per tree search (or per
// stand-alone call) by a grid of threads, then every workgroup of every level copies its image with b128 loads that are all in
// flight at once.  (Building the 97 KB image inside each persistent workgroup cost ~10 us of dependent L2 round trips per
// launch -- most of a small-batch launch.)
// One thread per image float (inverse map: which array, which element): every source load of the grid is in flight at once --
// one L2 round trip for both images instead of one per array (the array-by-array version took 7 us).
constexpr int kPackThreads = 256;

// element `idx` of the A-fragment image of W (k-major [IN][OUT]); same map as fill_frags
template <int IN, int OUT>
__device__ __forceinline__ float frag_element(const float* __restrict__ W, int idx) {
    constexpr int IT = Tiles<IN>::v;
    const int l = idx & 63, fr = idx >> 6;
    const int r = fr & 3, it = (fr >> 2) % IT, ot = (fr >> 2) / IT;
    const int in = tile_feature<IN>(it, l >> 4, r), out = frag_out_feature<OUT>(ot, l);
    return (in < IN && out < OUT) ? W[in * OUT + out] : 0.f;
}
template <int OUT>
__device__ __forceinline__ float bias_element(const float* __restrict__ b, int idx) {
    const int feat = tile_feature<OUT>(idx >> 4, (idx >> 2) & 3, idx & 3);
    return feat < OUT ? b[feat] : 0.f;
}
// element `e` of a [ROWS_PAD][LD] image of a k-major [ROWS][COLS] matrix (padding rows / columns: 0)
template <int ROWS, int COLS, int LD>
__device__ __forceinline__ float matrix_element(const float* __restrict__ W, int e) {
    const int r = e / LD, c = e - r * LD;
    return (r < ROWS && c < COLS) ? W[r * COLS + c] : 0.f;
}

// one float of the BX f3 region (BxLayout): a pair of bf16 pieces of the matrix-pipe fragments, or an f32 fragment element
template <int IN, int OUT>
__device__ __forceinline__ float bx_element(const float* __restrict__ W, int idx) {
    using BL = BxLayout<IN, OUT>;
    if (idx >= BL::p4) {                                           // partial tile, compact: row (q, lane % 4), k step = it * 4 + r
        using PC = P4Compact<BL::KP>;
        const int j = idx - BL::p4, row = j / PC::KPAD, ks = j - row * PC::KPAD;
        return ks < BL::KP ? frag_element<IN, OUT>(W, (BL::OTF * BL::IT * 4 + ks) * 64 + 16 * (row >> 2) + (row & 3)) : 0.f;
    }
    if (idx >= BL::f32) {
        const int j = idx - BL::f32, l = j & 63, slot = j >> 6;                          // slot: k steps of the output tiles, in order
        int ot, kf, it0;
        if (slot < BL::OT3 * BL::KF3) { ot = slot / BL::KF3; kf = slot - ot * BL::KF3; it0 = BL::ITB + 2; }
        else { const int s2 = slot - BL::OT3 * BL::KF3; ot = BL::OT3 + s2 / BL::KF; kf = s2 % BL::KF; it0 = BL::ITB; }
        return frag_element<IN, OUT>(W, ((ot * BL::IT + it0) * 4 + kf) * 64 + l);
    }
    int c, ot, pc, l, p;
    if (idx >= BL::b16c) {                                                               // third chunk: [ot < OT3][piece][lane]
        const int u = (idx - BL::b16c) >> 2, rest = u >> 6;
        p = idx & 3; l = u & 63; pc = rest % 3; ot = rest / 3; c = BL::NCB;
    } else {
        const int u = idx >> 2, rest = u >> 6;
        p = idx & 3; l = u & 63; pc = rest % 3; c = (rest / 3) % BL::NCB; ot = rest / 3 / BL::NCB;
    }
    const int q = l >> 4, out = frag_out_feature<OUT>(ot, l);
    bf16x2 v;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = 2 * p + k;
        v[k] = split3_piece(W[tile_feature<IN>(2 * c + (e >> 2), q, e & 3) * OUT + out], pc);
    }
    return __builtin_bit_cast(float, v);
}

// one float of the BX f2 region (Bx1Layout)
template <int IN, int OUT>
__device__ __forceinline__ float bx1_element(const float* __restrict__ W, int idx) {
    using BL = Bx1Layout<IN, OUT>;
    if (idx >= BL::p4) {                                           // partial tile, compact: row (q, lane % 4), k step = it * 4 + r
        using PC = P4Compact<BL::KP>;
        const int j = idx - BL::p4, row = j / PC::KPAD, ks = j - row * PC::KPAD;
        return ks < BL::KP ? frag_element<IN, OUT>(W, (BL::OTF * Tiles<IN>::v * 4 + ks) * 64 + 16 * (row >> 2) + (row & 3)) : 0.f;
    }
    const int u = idx >> 2, p = idx & 3, l = u & 63, rest = u >> 6;
    const int pc = rest % 3, ot = rest / 3, q = l >> 4, out = frag_out_feature<OUT>(ot, l);
    bf16x2 v;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = 2 * p + k;
        v[k] = split3_piece(W[tile_feature<IN>(e >> 2, q, e & 3) * OUT + out], pc);
    }
    return __builtin_bit_cast(float, v);
}

template <int D1, int D2, int D3, bool BX = false>
__global__ __launch_bounds__(kPackThreads) void pack_images_kernel(const FusedArgs a, float* img) {
    using LO = FusedLds<D1, D2, D3, BX>;
    const int e = blockIdx.x * kPackThreads + threadIdx.x;
    if (e >= LO::scratch) return;
    float v;
    if (e < LO::br1) v = matrix_element<9, HID, LO::WR1LD>(a.wr1, e - LO::wr1);
    else if (e < LO::wr2) v = a.br1[e - LO::br1];
    else if (e < LO::br2) {
        if constexpr (BX) v = frag_bf3_ld<HID, XD>(a.wr2, XD, XD, e - LO::wr2);
        else v = matrix_element<HID, XD, WLD>(a.wr2, e - LO::wr2);
    } else if (e < LO::wa) v = a.br2[e - LO::br2];
    else if (e < LO::w1) {
        const int k = e - LO::wa, r = k / WLD, col = k - r * WLD;
        if constexpr (BX) v = a.wa ? frag_bf3_ld<XD, XD>(a.wa, XD, XD, k) : frag_bf3_identity<XD>(k);      // gaussian: Wa = I
        else v = a.wa ? matrix_element<XD, XD, WLD>(a.wa, k) : ((col < XD && r == col) ? 1.f : 0.f);      // gaussian: Wa = I
    } else if (e < LO::wh1) {
        if constexpr (BX) v = frag_bf3_ld<XD, XD>(a.w1, XD, XD, e - LO::w1);
        else v = matrix_element<XD, XD, WLD>(a.w1, e - LO::w1);
    } else if (e < LO::bh1) v = matrix_element<5, HID, LO::WH1LD>(a.wh1, e - LO::wh1);
    else if (e < LO::wh2) v = a.bh1[e - LO::bh1];
    else if (e < LO::bh2) {
        v = matrix_element<HID, XD, WLD>(a.wh2, e - LO::wh2);
    }
    else if (e < LO::b1) v = a.bh2[e - LO::bh2];
    else if (e < LO::b2) v = bias_element<D1>(a.hb1, e - LO::b1);
    else if (e < LO::b3) v = bias_element<D2>(a.hb2, e - LO::b2);
    else if (e < LO::w4) v = bias_element<D3>(a.hb3, e - LO::b3);
    else if (e < LO::f_last) v = bias_element<D3>(a.hw4, e - LO::w4);          // w4 is [D3][1]: same padded vector layout as a bias
    else {
        if (e < LO::f1) {
            if constexpr (BX) v = frag_bf3_ld<XD, XD>(a.w_last, XD, XD, e - LO::f_last);
            else v = frag_element<XD, XD>(a.w_last, e - LO::f_last);
        }
        else if (e < LO::f2) {
            if constexpr (BX && D1 == 32) v = bx1_element<XD, 32>(a.hw1, e - LO::f1);
            else v = frag_element<XD, D1>(a.hw1, e - LO::f1);
        }
        else if (e < LO::f3) {
            if constexpr (BX) v = bx1_element<D1, D2>(a.hw2, e - LO::f2);
            else v = frag_element<D1, D2>(a.hw2, e - LO::f2);
        } else if constexpr (BX) v = bx_element<D2, D3>(a.hw3, e - LO::f3);
        else v = frag_element<D2, D3>(a.hw3, e - LO::f3);
    }
    img[e] = v;
}

}  // namespace

namespace rgl {

int fused::launch_pack_image(const FusedArgs& a, float* img, int mode, hipStream_t stream) {
    if (mode == kModeBx) {
        using LO = FusedLds<32, 100, 100, true>;
        hipLaunchKernelGGL((pack_images_kernel<32, 100, 100, true>), dim3((unsigned)((LO::scratch + kPackThreads - 1) / kPackThreads)),
                           dim3(kPackThreads), 0, stream, a, img);
    } else {
        using LO = FusedLds<32, 100, 100, false>;
        hipLaunchKernelGGL((pack_images_kernel<32, 100, 100, false>), dim3((unsigned)((LO::scratch + kPackThreads - 1) / kPackThreads)),
                           dim3(kPackThreads), 0, stream, a, img);
    }
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

// asked first: fused_children_covers(.., mode); `image`: the image slot of a children workspace (carve_children)
int pack_children_images(const RglGraph* g, const RglMlp* head, int P, int A, int H, float* image, hipStream_t stream,
                         FusedImageMode mode) {
    FusedPlan fp = plan_fused(*g, *head, P, A, H, 1, mode);
    if (!fp.ok || !image) return RGL_ERR_BAD_MODE;
    return launch_pack_image(fp.a, image, fp.mode(), stream);
}

}  // namespace rgl

// The image depends on the weights (and on the contraction mode: three-piece bf16 fragments for RGL_CONTRACT_BF16X6) only: a caller
// with fixed weights packs it once (MprlPlanner::children_image).  Whether an image of the planner's mode serves its weights is the
// planner unit's answer (image_serves).
static int image_mode_of(const MprlPlanner* planner) {
    return planner->contraction_dtype == RGL_CONTRACT_BF16X6 ? kModeBx : kModeF32;
}

extern "C" size_t mprl_children_image_bytes(const MprlPlanner* planner) {
    if (!planner) return 0;
    return image_serves(planner->value_graph, planner->value_head, image_mode_of(planner)) ? kImageBytes : 0;
}

extern "C" int mprl_pack_children_image_f32(const MprlPlanner* planner, float* image, size_t image_bytes, rgl_stream_t stream) {
    if (!planner || !image) return RGL_ERR_NULL;
    const int mode = image_mode_of(planner);
    if (!image_serves(planner->value_graph, planner->value_head, mode)) return RGL_ERR_BAD_MODE;
    if (image_bytes < kImageBytes) return RGL_ERR_WORKSPACE;
    FusedArgs a{};
    set_weights(a, planner->value_graph, planner->value_head);
    return launch_pack_image(a, image, mode, (hipStream_t)stream);
}

