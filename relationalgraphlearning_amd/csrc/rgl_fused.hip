// rgl_fused.hip -- planner and driver of the fused children kernel (rgl_fused_kernel.hip), host code only: which launches take the
// kernel, which form of it, how their tiles are cut into work items and dealt over the waves, and the call that launches a level
// (launch_fused_children).  Every process-wide cache of the fused path lives in this unit and its switches (rgl_switches.h) are
// asked here: a change to a launch decision recompiles nothing else.
#include "rgl_fused.h"
#include "rgl_scene_body.h"      // the level prologue's chunk arithmetic (prologue_chunk_end, prologue_row_floats), host side

#include <mutex>
#include <unordered_map>

using namespace rgl::fused;

namespace {

// Which launches take the fused kernel.  Measured on MI355X (tools/kiter.py, profiles/r02_*): both organisations end up
// pipe-bound (MFMA + VALU issue, no co-execution) at a shader clock that drops with utilisation.  The fused kernel is one launch
// that reads the child rows and writes the values; from ~3 k tiles (P ~ 500 parents of 81 actions) upwards it is the faster one
// (P = 1024: 76 vs 79 us, 2048: 114 vs 131, 4096: 205 vs 233); below, the two-stage pair (8 waves share a parent, 4 waves per
// SIMD in the head) hides the per-tile latency better.  RGL_CHILDREN_FUSED=1 / RGL_CHILDREN_TWO_STAGE=1 force one (tests):
// fused_policy().

// How the tiles of a launch are cut into work items.  A work item = G consecutive full tiles of one parent (the last group of a
// parent may be shorter, and also carries the parent's partial tile); its wave computes the parent's crowd quantities first, so
// small G repeats crowd work (~0.45 of a tile) while large G leaves waves idle when parents are few.  Two waves share a SIMD
// (pipe-bound: their loads add).
struct ItemPlan { int G, ipp, rot, grid, k_wg, inline_partial; };

inline int fused_cu_count() {
    static const int n_cu = [] { int dev = 0, n = 0; (void)hipGetDevice(&dev);
                                 (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n > 0 ? n : rgl::kCuCount; }();
    return n_cu;
}

// `unit`: parents are handed to workgroups in blocks that are multiples of this (the parents of one root at the deepest level when
// the kernel's tail walks the back-up chain; 1 otherwise).  Workgroup b owns parents [b k, (b + 1) k), k = the smallest multiple of
// `unit` that covers P with one workgroup per CU.  Within a workgroup the items are dealt over the 8 waves in snake passes (waves w
// and w + 4 share a SIMD); the plan simulates that dealing for one full workgroup and takes the cut with the smallest per-SIMD
// makespan (cached per shape: launches repeat).
inline ItemPlan plan_items(int P, int n_full, int rem, int unit) {
    static std::mutex mu;
    static std::unordered_map<unsigned long long, ItemPlan> cache;
    const unsigned long long key = ((unsigned long long)P << 32) ^ ((unsigned long long)unit << 16) ^
                                   ((unsigned long long)n_full << 8) ^ (unsigned long long)rem;
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = cache.find(key);
        if (it != cache.end()) return it->second;
    }
    // in full-tile units (instruction counts of the phases); a tile whose SIMD has no second wave to overlap with runs slower
    constexpr float kCrowd = 0.45f, kPartial = 0.45f, kHead = 0.65f, kSolo = 1.12f;
    const int n_cu = fused_cu_count();
    int k = (P + n_cu - 1) / n_cu;
    if (k < 1) k = 1;
    k = ((k + unit - 1) / unit) * unit;
    const int grid = (P + k - 1) / k;
    const int force_g = fused_forced_g(), force_inline = fused_forced_inline_partial();   // measurements
    ItemPlan best{1, n_full > 0 ? n_full : 1, 0, grid, k, 0};
    float best_cost = -1.f;
    for (int inl = 0; inl <= 1; ++inl) {
        if (inl && !rem) continue;
        if (force_inline >= 0 ? (inl != (force_inline && rem ? 1 : 0)) : (inl && (long)k * rem > 8)) continue;
        const int n_tiles = n_full + inl;                        // tiles that run their own head
        const int CT = n_tiles > 0 ? n_tiles : 1;
        for (int G = CT; G >= 1; --G) {
            if (force_g > 0 && G != (force_g < CT ? force_g : CT)) continue;
            const int ipp = (CT + G - 1) / G;
            if (G > 1 && (ipp - 1) * G >= CT) continue;
            const int last_tiles = n_tiles - (ipp - 1) * G;      // tiles of the last group (n_tiles == 0: 0)
            const float c_full = kCrowd + G;
            const float c_last = kCrowd + (last_tiles > 0 ? last_tiles : 0) + ((rem && !inl) ? kPartial : 0.f);
            const int rot = (ipp > 1 && c_last > c_full) ? ipp - 1 : 0;
            float wload[kFusedWaves] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const long n_items = (long)k * ipp;
            for (long i = 0; i < n_items; ++i) {
                int j = (int)(i / k) + rot;
                if (j >= ipp) j -= ipp;
                const long pass = i / kFusedWaves, r = i - pass * kFusedWaves;
                const int w = (int)((pass & 1) ? kFusedWaves - 1 - r : r);
                wload[w] += j == ipp - 1 ? c_last : c_full;
            }
            // a SIMD's two waves (w, w + 4) share the pipe while both run (their loads add) and the longer one finishes alone at
            // the solo rate: (3.45, 3.45) beats (5.45, 1.45) -- measured at P = 1024: 0.061 vs 0.063 ms (f32), 0.041 vs 0.043 (f16x3)
            float mk = 0.f;
            for (int sidx = 0; sidx < 4; ++sidx) {
                const float hi = wload[sidx] > wload[sidx + 4] ? wload[sidx] : wload[sidx + 4];
                const float lo = wload[sidx] > wload[sidx + 4] ? wload[sidx + 4] : wload[sidx];
                const float v = 2.f * lo + (hi - lo) * kSolo;
                mk = v > mk ? v : mk;
            }
            if (rem && !inl) {                                   // the tile-packed pass behind the barrier
                const long head_tiles = ((long)k * rem + 15) / 16;
                mk += kHead * (float)((head_tiles + kFusedWaves - 1) / kFusedWaves) * (head_tiles > 4 ? 2.f : 1.f) + 0.05f;
            }
            if (best_cost < 0.f || mk < best_cost - 1e-3f) { best_cost = mk; best = ItemPlan{G, ipp, rot, grid, k, inl}; }
        }
    }
    std::lock_guard<std::mutex> lk(mu);
    if (cache.size() > 8192) cache.clear();                    // callers with ever-changing parent counts: bounded memory
    cache.emplace(key, best);
    return best;
}

// the switches that take the fused kernel away whatever the launch
inline bool fused_enabled() { return fast_path_enabled() && rank1_enabled() && fused_policy() >= 0; }

// "Do the weights have the fused kernel's shapes?" -- what plan_fused asks of a model before it looks at a launch's sizes: the
// shipped embeddings and value head on x_dim = 32, and (the kernel's own envelope) two layers with one adjacency whose row
// normalisation the shared-crowd kernels implement.  image_only: what the packed image alone needs -- outside that envelope (three
// layers, another similarity, crowds beyond 32 agents) the f32 image still serves the stage-2 head, launched on its own or run by
// children_deep_kernel behind its parents: the same layout, `w_last` = the graph's last layer.
bool fused_architecture(const RglGraph& g, const RglMlp& head, bool image_only = false) {
    if (g.x_dim != XD || !mlp_is(g.w_r, 9, HID, XD, true) || !mlp_is(g.w_h, 5, HID, XD, true) || head_variant(head) != 0) return false;
    if (image_only) return g.num_layer >= 2 && g.num_layer <= RGL_MAX_GCN_LAYERS;
    return fast_similarity_mode(g) >= 0 && !g.layerwise_graph && g.num_layer == 2;
}

}  // namespace

namespace rgl {
namespace fused {

// The bf16x6 image is in the fused kernel's layout only: it serves where that kernel runs (a bf16x6 plan takes every launch size).
// The f32 image also serves the stage-2 head, so the fused kernel's own switches and thresholds do not enter.
bool image_serves(const RglGraph& g, const RglMlp& head, int mode) {
    return mode == kModeBx ? fused_enabled() && fused_architecture(g, head) : fast_path_enabled() && fused_architecture(g, head, true);
}

void set_weights(FusedArgs& a, const RglGraph& g, const RglMlp& head) {
    a.wr1 = g.w_r.weight[0]; a.br1 = g.w_r.bias[0]; a.wr2 = g.w_r.weight[1]; a.br2 = g.w_r.bias[1];
    a.wa = bilinear_wa(g); a.w1 = g.Ws[0];
    a.w_last = g.Ws[g.num_layer - 1];
    a.hw1 = head.weight[0]; a.hb1 = head.bias[0]; a.hw2 = head.weight[1]; a.hb2 = head.bias[1];
    a.hw3 = head.weight[2]; a.hb3 = head.bias[2]; a.hw4 = head.weight[3]; a.hb4 = head.bias[3];
    a.wh1 = g.w_h.weight[0]; a.bh1 = g.w_h.bias[0]; a.wh2 = g.w_h.weight[1]; a.bh2 = g.w_h.bias[1];
}

// mode kModeBx: the six-term bf16 products are wanted (RGL_CONTRACT_BF16X6): such a plan takes every launch size (the two-stage pair
// has no such head, and the packed image is in this kernel's layout only).
FusedPlan plan_fused(const RglGraph& g, const RglMlp& head, int P, int A, int H, int unit, int mode) {
    FusedPlan pl;
    pl.ok = false;
    pl.bx = mode == kModeBx;                    // any similarity: the head does not depend on it
    if (!fused_enabled()) return pl;
    const int min_tiles = fused_min_tiles();
    if (!pl.bx && fused_policy() == 0 && (long)P * ((A + 15) / 16) < min_tiles) return pl;
    if (!fused_architecture(g, head)) return pl;
    const int N = H + 1;
    if (N > 32 || A < 1) return pl;
    FusedArgs& a = pl.a;
    a.N = N; a.A = A; a.P = P; a.H = H;
    pl.nt = (N + 15) / 16;
    pl.hr = N <= 8 ? 8 : (N <= 20 ? 20 : 32);
    a.SLD = 16 * pl.nt + 1;                      // rows padded to whole MFMA tiles (unconditional access), odd stride
    a.n_full = A / 16;
    a.rem = A % 16;
    a.sim = fast_similarity_mode(g);
    {
        const ItemPlan ip = plan_items(P, a.n_full, a.rem, unit);
        a.tiles_per_item = ip.G;
        a.items_per_parent = ip.ipp;
        a.rot = ip.rot;
        a.parents_per_wg = ip.k_wg;
        a.inline_partial = ip.inline_partial;
        a.tail = TailArgs{};
        pl.grid = ip.grid;
    }
    pl.lds_bytes = (size_t)fused_lds_floats(pl.hr, pl.nt, a.sim == SIM_SOFTMAX, pl.bx) * sizeof(float);
    if (pl.lds_bytes > (size_t)rgl::kLdsBytesPerCu) return pl;      // (such a form has no kernel: launch_fused_ts reads the same function)
    set_weights(a, g, head);
    pl.ok = true;
    return pl;
}

}  // namespace fused
}  // namespace rgl

namespace {

// the plans the prologue form is instantiated for: bf16x6, 17..20 nodes, softmax similarity; and its scene region fits the LDS
inline bool prologue_form(const FusedPlan& pl, int scene_floats) {
    return pl.ok && pl.bx && pl.hr == kPrologueHR && pl.nt == kPrologueNT && pl.a.sim == SIM_SOFTMAX && scene_floats > 0 &&
           (size_t)(kPrologueSceneBase<FusedImage<true>> + scene_floats) * sizeof(float) <= pl.lds_bytes;
}

}  // namespace

namespace rgl {

// The children workspace: the weight image slot | one region as long as the longest of its users' carves (rgl_common.h).
ChildrenWorkspace carve_children(void* base, const MprlPlanner* pl, int P, int H) {
    const int A = pl->num_actions;
    auto rows = [](long long n) { Carver c{nullptr, 0}; c.take<float>(n * 64 * sizeof(float)); return (size_t)c.off; };
    const size_t users[] = {
        rows((long long)P * A),                                      // stage-1 rows of the rank-1, deep and tile kernels
        H + 1 <= 32 ? rows((long long)P * (A % 16)) : 0,             // FusedArgs::rows_left
        predict_humans_workspace_bytes(P, 1, H),
        scene_children_workspace_bytes(P, A, H),
        // the tile kernels, for planners outside the shipped shapes: children of the value graph, scenes of the state predictor
        tiles_forward_workspace_bytes(&pl->value_graph, &pl->value_head, nullptr, P * A, A, H, 0),
        pl->linear_state_predictor ? 0 : tiles_forward_workspace_bytes(&pl->predictor_graph, nullptr, &pl->motion_head, P, 1, H, 0)};
    size_t longest = 0;
    for (const size_t u : users) longest = u > longest ? u : longest;
    Carver c{(char*)base, 0};
    ChildrenWorkspace w;
    w.image = H + 1 <= 32 ? c.take<float>(kImageBytes) : nullptr;
    w.region = c.take<char>((long long)longest);
    w.region_bytes = longest;
    w.bytes = (size_t)c.off;
    return w;
}

// The caller has asked route_value_children: the form of `mode` covers the call (with its prologue, if it carries one), `w` is the
// call's workspace (it holds carve_children's bytes), and own_image says whose image the kernel reads.
int launch_fused_children(const RglGraph* g, const RglMlp* head, const ChildrenCall& c, const ChildrenWorkspace& w, FusedImageMode mode,
                          bool own_image) {
    const int P = c.P, A = c.A, H = c.H;
    if (c.tail_done) *c.tail_done = 0;
    // the search's tail: selection always; the back-up chain + root step at the deepest level when handing whole roots to
    // workgroups does not starve the GPU (few roots with many parents each -- unclipped deep searches -- keep unit = 1)
    const TailArgs* ta = (c.tail && c.tail->enabled && !fused_tail_disabled()) ? c.tail : nullptr;
    int chain = 0;
    const int unit = ta ? tail_ownership(*ta, P, fused_cu_count() / 2, &chain) : 1;
    FusedPlan fp = plan_fused(*g, *head, P, A, H, unit, mode);      // (.ok does not depend on `unit`: the route asked with 1)
    if (!fp.ok) return RGL_ERR_BAD_MODE;
    fp.pro = c.prologue;
    if (!w.image) return RGL_ERR_BAD_MODE;      // (the route asked: a fused plan has at most 32 nodes, and a workspace)
    if (own_image || (!c.image_ready && !c.image)) {
        int rc = launch_pack_image(fp.a, w.image, fp.mode(), c.stream);
        if (rc) return rc;
    }
    fp.a.child_robot = c.child_robot;
    fp.a.humans = c.humans_next;
    fp.a.value = c.child_value;
    fp.a.image = (c.image && !own_image) ? c.image : w.image;
    fp.a.rows_left = (float*)w.region;
    fp.a.image_sync = fused_image_sync();
    fp.a.phase_delay = fused_phase_delay();
    fp.a.prio = fused_prio();
    fp.a.head_early = fused_head_early();
    if (ta) {
        fp.a.tail = *ta;
        fp.a.tail.chain = chain;
    }
    const int rc = launch_fused(fp, g->skip_connection != 0, c.stream);
    if (rc == RGL_OK && ta && c.tail_done) *c.tail_done = chain ? 2 : 1;
    return rc;
}

// Measured (profiles/level_prologue_ab.txt): with 8 and 16 parents per workgroup (configs[2]: 2048 roots) the one launch is 3 % faster
// per step than the three; with 1 and 2 (the 256-root share) it is 6 % slower -- one scene chain per busy wave and most waves idle
// through it, where the stand-alone split scene kernel spreads each scene over two waves.  Below 4 parents per CU the level keeps
// its three launches.
constexpr int kPrologueMinParentsPerCu = 4;

int fused_prologue_region_floats() {
    return fused_lds_floats(kPrologueHR, kPrologueNT, true, true) - kPrologueSceneBase<FusedImage<true>>;
}

bool fused_prologue_fits(const MprlPlanner* pl, int P, int H, size_t workspace_bytes, int scene_floats) {
    if (P < kPrologueMinParentsPerCu * fused_cu_count() - (fused_cu_count() - 1)) return false;     // ceil(P / CUs) < 4
    return scene_floats >= 0 && route_value_children(pl, P, H, workspace_bytes, false, scene_floats).family == kChildrenFused;
}

// host only (route_value_children): does the form of `mode` take the call -- and, with a prologue, is it the prologue's form?
bool fused_children_covers(const RglGraph* g, const RglMlp* head, int P, int A, int H, FusedImageMode mode, int prologue_scene_floats) {
    const FusedPlan fp = plan_fused(*g, *head, P, A, H, 1, mode);
    return prologue_scene_floats >= 0 ? prologue_form(fp, prologue_scene_floats) : fp.ok;
}

}  // namespace rgl

extern "C" int rgl_plan_prologue_embedding(const MprlPlanner* planner, int P, int H, int crowds_per, int unit,
                                           RglPrologueEmbeddingPlan* plan) {
    if (!planner || !plan) return RGL_ERR_NULL;
    if (P < 1 || H < 1 || crowds_per < 1 || unit < 1 || P % crowds_per) return RGL_ERR_BAD_SHAPE;
    *plan = RglPrologueEmbeddingPlan{};
    int scene_floats = 0, chunk_crowds = 0;
    if (!level_prologue_enabled() || !rgl::level_prologue_layout(planner, crowds_per, P, H, &scene_floats, &chunk_crowds)) return RGL_OK;
    if (!rgl::fused_prologue_fits(planner, P, H, ~(size_t)0, scene_floats)) return RGL_OK;
    const FusedPlan fp = plan_fused(planner->value_graph, planner->value_head, P, planner->num_actions, H, unit, kModeBx);
    const int k = fp.a.parents_per_wg;
    const int c1 = prologue_chunk_end(0, k, crowds_per, chunk_crowds);              // a workgroup's first chunk; a full one where k allows
    plan->prologue = 1;
    plan->parents_per_wg = k;
    plan->workgroups = fp.grid;
    plan->chunk_parents = c1;
    plan->chunk_crowds = chunk_crowds;
    plan->human_tiles = (((c1 - 1) / crowds_per + 1) * H + 15) / 16;
    plan->robot_tiles = 1;
    plan->row_floats = prologue_row_floats(H, chunk_crowds);
    for (int c0 = 0; c0 < k; c0 = prologue_chunk_end(c0, k, crowds_per, chunk_crowds)) ++plan->chunks_per_wg;
    return RGL_OK;
}
