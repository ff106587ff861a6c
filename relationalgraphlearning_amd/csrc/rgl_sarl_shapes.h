// The shapes the SARL / OM-SARL units are built for (rgl_sarl.hip: evaluation; rgl_sarl_backward.hip: training).  Host code only.
#pragma once
#include "rgl_common.h"

namespace {

inline int sarl_map_floats(const SarlPlanner& pl) { return pl.om_channel_size ? pl.cell_num * pl.cell_num * pl.om_channel_size : 0; }

// the shapes the value kernel is built for; `H` < 0: the planner alone
inline int validate_sarl(const SarlPlanner& pl, int H) {
    const RglMlp* ms[4] = {&pl.mlp1, &pl.mlp2, &pl.attention, &pl.mlp3};
    for (const RglMlp* m : ms) {
        const int rc = rgl::validate_mlp(*m, 0, 0);
        if (rc) return rc;
    }
    if (pl.om_channel_size < 0 || pl.om_channel_size > 3) return RGL_ERR_BAD_MODE;
    if (pl.om_channel_size && (pl.cell_num < 1 || pl.cell_num > 8 || !(pl.cell_size > 0.0))) return RGL_ERR_BAD_SHAPE;
    const int D = 13 + sarl_map_floats(pl);
    if (D != 13 && D != 29 && D != 45 && D != 61) return RGL_ERR_BAD_SHAPE;
    const int att_in = pl.with_global_state ? 200 : 100;
    auto is = [](const RglMlp& m, int n, int d0, int d1, int d2, int d3, int d4, int relu) {
        const int want[5] = {d0, d1, d2, d3, d4};
        if (m.n_layers != n || (m.last_relu != 0) != (relu != 0)) return false;
        for (int l = 0; l <= n; ++l)
            if (m.dims[l] != want[l]) return false;
        return true;
    };
    if (!is(pl.mlp1, 2, D, 150, 100, 0, 0, 1) || !is(pl.mlp2, 2, 100, 100, 50, 0, 0, 0) ||
        !is(pl.attention, 3, att_in, 100, 100, 1, 0, 0) || !is(pl.mlp3, 4, 56, 150, 100, 100, 1, 0))
        return RGL_ERR_BAD_SHAPE;
    if (pl.contraction_dtype != RGL_CONTRACT_F32) return RGL_ERR_BAD_MODE;
    if (H >= 0 && (H < (pl.om_channel_size ? 2 : 1) || H > RGL_SARL_MAX_HUMANS)) return RGL_ERR_BAD_SHAPE;
    return RGL_OK;
}

}  // namespace
