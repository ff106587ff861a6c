// rgl_fused.h -- what the three translation units of the fused children kernel share: the kernel and its dispatcher
// (rgl_fused_kernel.hip), the weight-image packer (rgl_fused_image.hip), the planner and driver (rgl_fused.hip, host code only).
// The kernel's arguments, the LDS arithmetic of its forms, the plan of a launch and the calls between the units.
#pragma once
#include "rgl_mlp_chain.h"      // FusedLds

namespace rgl {
namespace fused {

using rgl::kModeBx;      // rgl_search_args.h
using rgl::kModeF32;

// Wave-private LDS scratch of children_fused_kernel (floats).  Packed row pass (softmax, HR <= 20): UW [HRL][32] of the item's parent
// | (r, b) table [16][HRL + 2][2] of the tile; otherwise (a, b) table [16][16 NT + 1][2] | Y [16][XLD].  Between items the same
// space holds Xh [16 NT][XLD] | msh, Zsh [2][16 NT] of the crowd computation.
__host__ __device__ constexpr bool fused_packed_rows(int HR, bool SOFT) { return SOFT && HR <= 20; }
__host__ __device__ constexpr int fused_scratch_floats(int HR, int NT, bool SOFT) {
    const int NP = 16 * NT, HRL = HR < NP ? HR : NP;
    const int main_fl = fused_packed_rows(HR, SOFT) ? HRL * 32 + 16 * (HRL + 2) * 2 : 2 * 16 * (NP + 1) + 16 * XLD;
    const int crowd_fl = NP * XLD + 2 * NP;
    const int fl = main_fl > crowd_fl ? main_fl : crowd_fl;
    return ((fl > kTailLdsInts ? fl : kTailLdsInts) + 3) & ~3;      // ... and, after the last item, the tables of the select step
}

struct FusedArgs {
    const float *wr1, *br1, *wr2, *br2, *wa, *w1;                       // child-side weights (k-major)
    const float *wh1, *bh1, *wh2, *bh2;                                 // w_h (crowd side)
    const float* w_last;                                                // [32][32] last GCN layer
    const float *hw1, *hb1, *hw2, *hb2, *hw3, *hb3, *hw4, *hb4;         // value head, k-major
    const float* child_robot;     // [P][A][9]
    const float* humans;          // [P][H][5] the parents' crowds
    float* value;                 // [P][A]
    float* rows_left;             // [P][A % 16][64]  rows [t_c | H1_0] of the partial last tiles (null when A % 16 == 0)
    int P, A, N, H, SLD, sim;
    int n_full;                   // full tiles per parent = A / 16
    int rem;                      // A % 16
    const float* image;           // FusedLds weight image [0, FusedLds::scratch) prepared in global memory by pack_images_kernel
    int tiles_per_item;           // a work item = this many consecutive FULL tiles of one parent (crowd quantities computed once)
    int items_per_parent;         // = ceil(n_full / tiles_per_item); the last group also carries the partial tile
    int rot;                      // item order: group (o + rot) % items_per_parent at order position o (heaviest group first)
    int parents_per_wg;           // workgroup b owns parents [b k, (b + 1) k): every item of a parent runs on that workgroup's waves
    int image_sync;               // measurements: stage the whole weight image through registers before anything else (round 3)
    int inline_partial;           // few parents per workgroup: the partial tile is an ordinary (padded) tile with its own head
                                  // instead of a row hand-off to the tile-packed pass at the end (a barrier + a serial head)
    int phase_delay;              // measurements (RGL_FUSED_PHASE_DELAY): waves 4..7 start this many 512-cycle sleeps late
    int prio;                     // RGL_FUSED_PRIO: bit 1 (default) = s_setprio 2 inside the head: -0.6 % / -1.3 % at 2048 / 4096 parents; bit 0
                                  // (measurements) = static s_setprio 1 for waves 4..7: nothing (profiles/r06_c_phase_prio_ab.txt)
    int head_early;               // RGL_FUSED_HEAD_EARLY (default 1): the waves that run out of items first score the tile-packed rows of the
                                  // partial tiles while the others still work (0: a pass behind a workgroup barrier, one wave per tile)
    TailArgs tail;                // tail.enabled: select (+ back-up chain + root step) for the owned parents at the end
};

// the level prologue's arguments: a kernel argument of the PRO instantiations only (the others keep FusedArgs' kernarg size)
template <bool PRO> struct PrologueArgs {};
template <> struct PrologueArgs<true> {
    SceneArgs scene;              // the state predictor's scenes of the owned parents (LevelPrologue::scene)
    ChildrenArgs children;        // their reward / next-state pairs
};

constexpr int kFusedWaves = 8;
// PRO: LDS floats below the scene region of the level prologue: the image's first part [0, f_last) in whole 256-float chunks (the
// chunk that holds f_last lands in full, so the scene region starts behind it)
template <class LO> constexpr int kPrologueSceneBase = (LO::f_last + 255) / 256 * 256;
static_assert(B6Floats<HID, XD>::v == HID * XD * 3 / 2 && B6Floats<XD, XD>::v == XD * XD * 3 / 2, "FusedLds sizes its BX matrices so");

// the weight image of the shipped head, the only one the kernels are instantiated for
template <bool BX> using FusedImage = FusedLds<32, 100, 100, BX>;
// LDS floats of a form of the kernel: the weight image | kFusedWaves wave scratches | the image's arrival counter (one int in a
// b128 granule of its own, the LAST kArrivalFloats of the allocation).  The one place this sum is written: the kernel's offsets,
// the planner's "does it fit" (plan_fused) and the dispatcher's "is it compiled" (launch_fused_ts) all read it.
constexpr int kArrivalFloats = 4;
__host__ __device__ constexpr int fused_lds_floats(int HR, int NT, bool SOFT, bool BX) {
    return (BX ? FusedImage<true>::scratch : FusedImage<false>::scratch) + kFusedWaves * fused_scratch_floats(HR, NT, SOFT) + kArrivalFloats;
}
constexpr bool fused_form_fits(int HR, int NT, bool SOFT, bool BX) {
    return fused_lds_floats(HR, NT, SOFT, BX) * sizeof(float) <= (size_t)kLdsBytesPerCu;
}
// What the arithmetic says today, family by family (HR, NT as plan_fused pairs them; SOFT = softmax row normalisation):
// every f32 form fits a CU ...
static_assert(fused_form_fits(8, 1, true, false) && fused_form_fits(8, 1, false, false) && fused_form_fits(20, 1, true, false) &&
              fused_form_fits(20, 1, false, false) && fused_form_fits(20, 2, true, false) && fused_form_fits(20, 2, false, false) &&
              fused_form_fits(32, 2, true, false) && fused_form_fits(32, 2, false, false), "every f32 form fits");
// ... of the bf16x6 forms (larger image) those of at most 16 nodes and the packed row pass of 17..20: launch_fused_children runs the
// others as f32 forms on an image of its own, and launch_fused_ts compiles no kernel for them ...
static_assert(fused_form_fits(8, 1, true, true) && fused_form_fits(8, 1, false, true) && fused_form_fits(20, 1, true, true) &&
              fused_form_fits(20, 1, false, true) && fused_form_fits(20, 2, true, true), "the bf16x6 forms that fit");
static_assert(!fused_form_fits(20, 2, false, true) && !fused_form_fits(32, 2, true, true) && !fused_form_fits(32, 2, false, true),
              "the bf16x6 forms that do not");
// ... and the level prologue's form (prologue_form) is one that does
constexpr int kPrologueHR = 20, kPrologueNT = 2;      // bf16x6, 17..20 nodes, softmax similarity
static_assert(fused_form_fits(kPrologueHR, kPrologueNT, true, true), "the prologue's form is compiled");

// sized for the larger layout: one buffer size whatever the contraction mode (a caller's MprlPlanner::children_image, and the first
// kImageBytes of a children workspace: carve_children, rgl_common.h)
constexpr size_t max2(size_t x, size_t y) { return x > y ? x : y; }
constexpr size_t kImageFloats = max2(FusedImage<false>::scratch, FusedImage<true>::scratch);
constexpr size_t kImageBytes = (kImageFloats * sizeof(float) + 255) & ~(size_t)255;

struct FusedPlan {
    FusedArgs a;
    size_t lds_bytes;
    int grid;
    int hr, nt;
    bool bx;                       // bf16 six-term hybrid of the last head matrix (RGL_CONTRACT_BF16X6)
    const LevelPrologue* pro = nullptr;      // with the level prologue (PrologueArgs)
    int mode() const { return bx ? kModeBx : kModeF32; }
    bool ok;
};

// ---- rgl_fused.hip (planner) ----
// the matrices the kernel and its packed image read (w_last = the graph's last layer: Ws[1] inside the fused kernel's envelope)
void set_weights(FusedArgs& a, const RglGraph& g, const RglMlp& head);
FusedPlan plan_fused(const RglGraph& g, const RglMlp& head, int P, int A, int H, int unit = 1, int mode = kModeF32);
// would a packed image of `mode` serve these weights, whatever the launch sizes?  (mprl_children_image_bytes)
bool image_serves(const RglGraph& g, const RglMlp& head, int mode);
// ---- rgl_fused_kernel.hip ----
// RGL_ERR_BAD_MODE: a form that does not fit a CU (fused_form_fits) has no kernel
int launch_fused(const FusedPlan& pl, bool skip, hipStream_t st);
// ---- rgl_fused_image.hip ----
// one packed image, in the layout of the kernel that will read it (kModeBx: the bf16 / f32 hybrid of the last head matrix)
int launch_pack_image(const FusedArgs& a, float* img, int mode, hipStream_t stream);

}  // namespace fused
}  // namespace rgl
