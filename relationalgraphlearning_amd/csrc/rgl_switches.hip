// rgl_switches.hip -- the environment switches' table, their parse and their one reader.  Host code only: no kernel.
#include "rgl_switches.h"

#include <cstdlib>
#include <cstring>
#include <mutex>

#include "rgl_hip.h"

namespace {

enum Parse {
    kOnIf1,          // on only if the first character is 1
    kOffIf0,         // on, off only if the first character is 0
    kInt,            // unset or empty: the default, otherwise atoi
    kIntIfSet,       // unset: the default, anything set (the empty string too) through atoi
    kOnUnlessZero,   // unset: on, set: atoi != 0 (empty is off)
    kIsGlobal        // 1 only for exactly "global"
};
enum Read { kOnce, kEveryCall };

struct Switch {
    rgl::SwitchId id;
    const char* name;
    Parse parse;
    int dflt;
    Read read;
    const char* meaning;
};

constexpr Switch kSwitches[] = {
    {rgl::kSwForceGeneric, "RGL_FORCE_GENERIC", kOnIf1, 0, kOnce, "the general VALU kernel instead of the shipped-shape MFMA kernels"},
    {rgl::kSwChildrenTileKernel, "RGL_CHILDREN_TILE_KERNEL", kOnIf1, 0, kOnce, "the full-graph tile kernel instead of the shared-crowd kernels"},
    {rgl::kSwChildrenFused, "RGL_CHILDREN_FUSED", kOnIf1, 0, kOnce, "children: always the fused tile-stream kernel"},
    {rgl::kSwChildrenTwoStage, "RGL_CHILDREN_TWO_STAGE", kOnIf1, 0, kOnce, "children: never the fused kernel (RGL_CHILDREN_FUSED wins)"},
    {rgl::kSwRequireMfmaChildren, "RGL_REQUIRE_MFMA_CHILDREN", kOnIf1, 0, kOnce, "children: an error instead of the general kernel"},
    {rgl::kSwRequireMfmaForward, "RGL_REQUIRE_MFMA_FORWARD", kOnIf1, 0, kEveryCall, "forward: an error instead of the general kernel"},
    {rgl::kSwSceneWideSlots, "RGL_SCENE_WIDE_SLOTS", kOnIf1, 0, kOnce, "split scene kernel: LDS for one scene slot per wave"},
    {rgl::kSwDeepT4, "RGL_DEEP_T4", kOffIf0, 1, kOnce, "deep kernel: a last node tile of <= 4 nodes on the 4 x 4 x 1 MFMA"},
    {rgl::kSwDeepFuseHead, "RGL_DEEP_FUSE_HEAD", kOffIf0, 1, kOnce, "deep kernel: stage 2 behind each workgroup's parents"},
    {rgl::kSwSceneEmbedInside, "RGL_SCENE_EMBED_INSIDE", kOffIf0, 1, kOnce, "small state-predictor launches embed their own rows"},
    {rgl::kSwLevelPrologue, "RGL_LEVEL_PROLOGUE", kOffIf0, 1, kOnce, "a tree level's state predictor and rewards in the fused kernel's prologue"},
    {rgl::kSwFusedG, "RGL_FUSED_G", kInt, 0, kOnce, "fused kernel: tiles per work item (0: planned per launch)"},
    {rgl::kSwFusedInlinePartial, "RGL_FUSED_INLINE_PARTIAL", kInt, -1, kOnce, "fused kernel: a parent's partial tile tile-packed (0) / ordinary (1)"},
    {rgl::kSwFusedMinTiles, "RGL_FUSED_MIN_TILES", kInt, 1200, kOnce, "tiles per launch from which the fused kernel takes the children"},
    {rgl::kSwFusedImageSync, "RGL_FUSED_IMAGE_SYNC", kInt, 0, kOnce, "fused kernel: the weight image staged through registers first"},
    {rgl::kSwFusedPhaseDelay, "RGL_FUSED_PHASE_DELAY", kInt, 0, kOnce, "fused kernel: waves 4..7 start n x 512 cycles late"},
    {rgl::kSwFusedPrio, "RGL_FUSED_PRIO", kInt, 2, kOnce, "fused kernel: bit 1 = priority inside the head, bit 0 = static for waves 4..7"},
    {rgl::kSwFusedHeadEarly, "RGL_FUSED_HEAD_EARLY", kInt, 1, kOnce, "fused kernel: partial-tile rows scored by the first idle waves"},
    {rgl::kSwFusedNoTail, "RGL_FUSED_NO_TAIL", kInt, 0, kOnce, "select / back-up / root as stand-alone kernels (used as != 0)"},
    {rgl::kSwTilesForward, "RGL_TILES_FORWARD", kInt, 1, kEveryCall, "0: never the tile kernels, 2: the tile kernels first"},
    {rgl::kSwBackwardMfma, "RGL_BACKWARD_MFMA", kInt, -1, kEveryCall, "backward: 0 per-scene kernel, 1 tile pipeline, 2 or an error"},
    {rgl::kSwBackwardMfmaMin, "RGL_BACKWARD_MFMA_MIN", kInt, 256, kEveryCall, "scenes from which the tile backward runs by itself"},
    {rgl::kSwSarlGridCap, "RGL_SARL_GRID_CAP", kInt, 0, kEveryCall, "at most n workgroups for the SARL value kernel (0: no cap)"},
    {rgl::kSwSceneSplitBelow, "RGL_SCENE_SPLIT_BELOW", kIntIfSet, -1, kOnce, "scenes below which a scene is split over waves (-1: built in)"},
    {rgl::kSwSceneChildrenBelow, "RGL_SCENE_CHILDREN_BELOW", kIntIfSet, -1, kOnce, "parents below which rewards ride in the scene launch (-1: built in)"},
    {rgl::kSwHeadRowsDirect, "RGL_HEAD_ROWS_DIRECT", kOnUnlessZero, 1, kOnce, "wide heads' rows on head_rows_kernel (0: mlp_rows_kernel)"},
    {rgl::kSwSarlPark, "RGL_SARL_PARK", kIsGlobal, 0, kEveryCall, "global: the SARL value kernel parks in the workspace at any crowd size"},
};
constexpr int kRows = sizeof(kSwitches) / sizeof(kSwitches[0]);

constexpr bool rows_follow_ids() {
    for (int i = 0; i < kRows; ++i)
        if (kSwitches[i].id != i) return false;
    return true;
}
static_assert(kRows == rgl::kSwitchCount && rows_follow_ids(), "one row per SwitchId, in the enum's order");

// a pure function of (row, text or null)
int parse_switch(const Switch& s, const char* e) {
    switch (s.parse) {
        case kOnIf1: return e && e[0] == '1';
        case kOffIf0: return !(e && e[0] == '0');
        case kInt: return e && e[0] ? atoi(e) : s.dflt;
        case kIntIfSet: return e ? atoi(e) : s.dflt;
        case kOnUnlessZero: return !e || atoi(e) != 0;
        case kIsGlobal: return e && !strcmp(e, "global");
    }
    return s.dflt;
}

}  // namespace

int rgl::switch_value(SwitchId id) {
    const Switch& s = kSwitches[id];
    const auto read_now = [&s] { return parse_switch(s, getenv(s.name)); };
    if (s.read == kEveryCall) return read_now();
    static std::once_flag read[kRows];
    static int value[kRows];
    std::call_once(read[id], [&] { value[id] = read_now(); });
    return value[id];
}

extern "C" const char* rgl_switch_name(int i) { return i >= 0 && i < kRows ? kSwitches[i].name : nullptr; }

extern "C" int rgl_switch_parse(int i, const char* text_or_null, int* value) {
    if (!value) return RGL_ERR_NULL;
    if (i < 0 || i >= kRows) return RGL_ERR_BAD_SHAPE;
    *value = parse_switch(kSwitches[i], text_or_null);
    return RGL_OK;
}
