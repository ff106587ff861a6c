// rgl_sarl_maps.h -- the arithmetic of MultiHumanRL.build_occupancy_maps (crowd_nav/policy/multi_human_rl.py:117-171) for one
// (human i, other human j) pair and for one slot of human i's map, shared by the translation units that must produce the same bits:
// rgl_sarl.hip (sarl_maps_kernel: the search's maps, rollout.occupancy_maps) and rgl_replay.hip (the replay memory's SARL rows, which
// must hold what SARL.transform makes of a recorded state).  Float64, every operation rounded on its own: compiled without
// contraction.  Also the host-side predicate both entry points apply to the map parameters.
#pragma once
#include "rgl_common.h"

namespace {

// cell_num, cell_size and the channel count as sarl_occupancy_maps_f32 accepts them: RGL_OK, or the code it answers
inline int sarl_map_params_rc(int cell_num, double cell_size, int channels) {
    if (channels < 1 || channels > 3) return RGL_ERR_BAD_MODE;
    if (cell_num < 1 || cell_num > 8 || !(cell_size > 0.0)) return RGL_ERR_BAD_SHAPE;
    return RGL_OK;
}

// The record of the pair (i, j): the cell of i's grid that j falls into (-1: j == i, or j outside the grid) and, for two and three
// channels, j's velocity in i's frame.  state(h, k) is element k of human h's [px, py, vx, vy, radius] as a double; the states are
// moved on by dt at constant velocity (dt = 0: the states themselves); own_angle = atan2(vy, vx) of human i.
template <class State>
__device__ __forceinline__ void sarl_map_pair(const State& state, int i, int j, double own_angle, double dt, int cell_num,
                                              double cell_size, int channels, int& cell, double& ovx, double& ovy) {
#pragma clang fp contract(off)
    cell = -1;
    ovx = 0.0, ovy = 0.0;
    if (j == i) return;
    const double px = state(i, 0) + state(i, 2) * dt, py = state(i, 1) + state(i, 3) * dt;
    const double half = (double)cell_num / 2.0;
    const double ox = (state(j, 0) + state(j, 2) * dt) - px, oy = (state(j, 1) + state(j, 3) * dt) - py;
    const double rot = atan2(oy, ox) - own_angle;
    const double dist = sqrt(ox * ox + oy * oy);
    const double xi = floor(cos(rot) * dist / cell_size + half), yi = floor(sin(rot) * dist / cell_size + half);
    if (xi >= 0.0 && xi < (double)cell_num && yi >= 0.0 && yi < (double)cell_num) {
        cell = cell_num * (int)yi + (int)xi;
        if (channels != 1) {
            const double vrot = atan2(state(j, 3), state(j, 2)) - own_angle;
            const double speed = sqrt(state(j, 2) * state(j, 2) + state(j, 3) * state(j, 3));
            ovx = cos(vrot) * speed;
            ovy = sin(vrot) * speed;
        }
    }
}

// One slot of human i's map from the H records of its pairs, walked in list order: the sums and counts of a slot form as upstream's
// lists do.
__device__ __forceinline__ float sarl_map_slot(const int* pair_cell, const double* pair_vx, const double* pair_vy, int H, int slot,
                                               int channels) {
#pragma clang fp contract(off)
    double sum = 0.0;
    int count = 0;
    for (int j = 0; j < H; ++j) {
        const int cell = pair_cell[j];
        if (cell < 0) continue;
        if (channels == 1) {
            if (cell == slot) count = 1;
            continue;
        }
        // the slot base is 2 * cell for two AND three channels (:159-164)
        if (channels == 2) {
            if (slot == 2 * cell) { sum += pair_vx[j]; ++count; }
            else if (slot == 2 * cell + 1) { sum += pair_vy[j]; ++count; }
        } else {
            if (slot == 2 * cell) { sum += 1.0; ++count; }
            else if (slot == 2 * cell + 1) { sum += pair_vx[j]; ++count; }
            else if (slot == 2 * cell + 2) { sum += pair_vy[j]; ++count; }
        }
    }
    return channels == 1 ? (count ? 1.f : 0.f) : (count ? (float)(sum / (double)count) : 0.f);
}

}  // namespace
