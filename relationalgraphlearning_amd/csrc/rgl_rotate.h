// rotate_row -- CADRL.rotate (cadrl.py:241-276) for one joint row, shared by the translation units that produce path G's pairwise
// relation features: rgl_tree.hip (gcn_rotate_f32, gcn_prepare_f32) and rgl_replay.hip (the replay memory's "gcn" layout and its SARL rows,
// which must store the bits rollout.rotate produces).
#pragma once
#include "rgl_common.h"

namespace {

__device__ __forceinline__ void rotate_row(const float* s, int unicycle, float* o) {
    // cadrl.py:241-276; every product / sum individually rounded like the chain of torch ops: compiled without contraction (plain
    // operators: __fmul_rn / __fadd_rn would bring the contraction of the header they come from along).  tests/path_g_steps.py
    // replays every column bit for bit given this device's atan2f / cosf / sinf.
#pragma clang fp contract(off)
    const float dx = s[5] - s[0], dy = s[6] - s[1];
    const float rot = atan2f(dy, dx);
    const float c = cosf(rot), sn = sinf(rot);
    o[0] = sqrtf(dx * dx + dy * dy);
    o[1] = s[7];
    o[2] = unicycle ? s[8] - rot : 0.f;
    o[3] = s[4];
    o[4] = s[2] * c + s[3] * sn;
    o[5] = s[3] * c - s[2] * sn;
    const float rx = s[9] - s[0], ry = s[10] - s[1];
    o[6] = rx * c + ry * sn;
    o[7] = ry * c - rx * sn;
    o[8] = s[11] * c + s[12] * sn;
    o[9] = s[12] * c - s[11] * sn;
    o[10] = s[13];
    const float ax = s[0] - s[9], ay = s[1] - s[10];
    o[11] = sqrtf(ax * ax + ay * ay);
    o[12] = s[4] + s[13];
}

}  // namespace
