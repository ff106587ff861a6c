// The library's environment switches ("Environment switches"): ONE table (rgl_switches.hip) and the only getenv of
// csrc/.  A switch is a row of that table -- its name, how its text parses, its default, whether it is read once per process (at its
// own first use) or at every call -- and an accessor below.  Host only.
#pragma once

namespace rgl {

enum SwitchId {      // the table's rows, in its order
    kSwForceGeneric, kSwChildrenTileKernel, kSwChildrenFused, kSwChildrenTwoStage, kSwRequireMfmaChildren, kSwRequireMfmaForward,
    kSwSceneWideSlots, kSwDeepT4, kSwDeepFuseHead, kSwSceneEmbedInside, kSwLevelPrologue, kSwFusedG, kSwFusedInlinePartial,
    kSwFusedMinTiles, kSwFusedImageSync, kSwFusedPhaseDelay, kSwFusedPrio, kSwFusedHeadEarly, kSwFusedNoTail, kSwTilesForward,
    kSwBackwardMfma, kSwBackwardMfmaMin, kSwSarlGridCap, kSwSceneSplitBelow, kSwSceneChildrenBelow, kSwHeadRowsDirect, kSwSarlPark,
    kSwitchCount
};

// the switch's value under the process's environment: a once-switch is read at the first call for it, and never again
int switch_value(SwitchId id);

}  // namespace rgl

namespace {

// ---- read once per process ---------------------------------------------------------------------------------------------------------
inline bool fast_path_enabled() { return !rgl::switch_value(rgl::kSwForceGeneric); }
// RGL_CHILDREN_TILE_KERNEL=1 disables the shared-crowd kernels (rank-1, deep) in favour of the tile kernel (tests)
inline bool rank1_enabled() { return !rgl::switch_value(rgl::kSwChildrenTileKernel); }
// 1: always the fused children kernel, -1: never (the two-stage pair), 0: by size.  RGL_CHILDREN_FUSED wins over RGL_CHILDREN_TWO_STAGE
inline int fused_policy() {
    return rgl::switch_value(rgl::kSwChildrenFused) ? 1 : (rgl::switch_value(rgl::kSwChildrenTwoStage) ? -1 : 0);
}
inline bool require_mfma_children() { return rgl::switch_value(rgl::kSwRequireMfmaChildren) != 0; }
inline bool scene_wide_slots() { return rgl::switch_value(rgl::kSwSceneWideSlots) != 0; }
inline bool deep_t4_enabled() { return rgl::switch_value(rgl::kSwDeepT4) != 0; }
inline bool deep_fuse_head_enabled() { return rgl::switch_value(rgl::kSwDeepFuseHead) != 0; }
inline bool scene_embed_inside_enabled() { return rgl::switch_value(rgl::kSwSceneEmbedInside) != 0; }
inline bool level_prologue_enabled() { return rgl::switch_value(rgl::kSwLevelPrologue) != 0; }
inline int fused_forced_g() { return rgl::switch_value(rgl::kSwFusedG); }                            // > 0: tiles per work item
inline int fused_forced_inline_partial() { return rgl::switch_value(rgl::kSwFusedInlinePartial); }   // >= 0: forced
inline int fused_min_tiles() { return rgl::switch_value(rgl::kSwFusedMinTiles); }
inline int fused_image_sync() { return rgl::switch_value(rgl::kSwFusedImageSync); }
inline int fused_phase_delay() { return rgl::switch_value(rgl::kSwFusedPhaseDelay); }
inline int fused_prio() { return rgl::switch_value(rgl::kSwFusedPrio); }
inline int fused_head_early() { return rgl::switch_value(rgl::kSwFusedHeadEarly); }
inline bool fused_tail_disabled() { return rgl::switch_value(rgl::kSwFusedNoTail) != 0; }    // select, back-up and root as stand-alone kernels
inline int scene_split_below_asked() { return rgl::switch_value(rgl::kSwSceneSplitBelow); }         // < 0: the built-in threshold
inline int scene_children_below_asked() { return rgl::switch_value(rgl::kSwSceneChildrenBelow); }   // < 0: the built-in threshold
inline bool rows_direct() { return rgl::switch_value(rgl::kSwHeadRowsDirect) != 0; }
// ---- read at every call (tests set these inside their process) -----------------------------------------------------------------------
inline bool require_mfma_forward() { return rgl::switch_value(rgl::kSwRequireMfmaForward) != 0; }
inline int tiles_forward_mode() { return rgl::switch_value(rgl::kSwTilesForward); }      // 0: never the tile kernels, 2: the tile kernels first
inline int backward_mfma_mode() { return rgl::switch_value(rgl::kSwBackwardMfma); }
inline int backward_mfma_min() { return rgl::switch_value(rgl::kSwBackwardMfmaMin); }
inline int sarl_grid_cap_asked() { return rgl::switch_value(rgl::kSwSarlGridCap); }
inline bool sarl_park_global() { return rgl::switch_value(rgl::kSwSarlPark) != 0; }

}  // namespace
