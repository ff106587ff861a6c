// One environment's time step, the part every step kernel shares: the robot's move, the closest-approach loop over the humans, the
// reward / termination ladder and a human's action under the configured policy (crowd_sim/envs/crowd_sim.py:252-368,
// crowd_sim/envs/utils/agent.py:113-139, crowd_sim/envs/policy/linear.py:16-22).  crowd_step_kernel (rgl_sim.hip, one thread per
// environment) and crowd_step_nonstop_kernel (rgl_nonstop.hip, one wave per environment) both call it: the arithmetic exists once.
#pragma once
#include "rgl_common.h"

namespace {

__device__ __forceinline__ double seg_dist_origin(double px, double py, double ex, double ey) {
    const double sx = ex - px, sy = ey - py;
    if (sx == 0.0 && sy == 0.0) return sqrt(px * px + py * py);
    double u = ((0.0 - px) * sx + (0.0 - py) * sy) / (sx * sx + sy * sy);
    u = u > 1.0 ? 1.0 : (u < 0.0 ? 0.0 : u);
    const double cx = px + u * sx, cy = py + u * sy;
    return sqrt(cx * cx + cy * cy);
}

struct RobotStep {
    double npx, npy, ntheta;    // the robot's next position and heading
    double reward, dmin;        // dmin: -1 after a collision (what the step reports)
    int info, fin;
};

// r: the robot's 9 doubles, hs: the environment's humans [H][5], both BEFORE anyone moves; (a0, a1) the robot's action
__device__ __forceinline__ RobotStep crowd_robot_step(const CrowdSimConfig& cfg, const double* r, const double* hs, int H, double a0,
                                                      double a1, double time) {
    const double dt = cfg.time_step;
    RobotStep o;
    double avx, avy;
    o.ntheta = r[8];
    if (cfg.kinematics == RGL_HOLONOMIC) {
        avx = a0; avy = a1;
        o.npx = r[0] + a0 * dt; o.npy = r[1] + a1 * dt;
    } else {
        const double th = r[8] + a1;
        avx = a0 * cos(a1 + r[8]); avy = a0 * sin(a1 + r[8]);
        o.npx = r[0] + cos(th) * a0 * dt; o.npy = r[1] + sin(th) * a0 * dt;
        o.ntheta = fmod(th, 2.0 * M_PI);
        if (o.ntheta < 0.0) o.ntheta += 2.0 * M_PI;          // python's % returns a non-negative remainder
    }
    bool collision = false;
    double dmin = INFINITY;
    for (int h = 0; h < H; ++h) {
        const double px = hs[h * 5] - r[0], py = hs[h * 5 + 1] - r[1];
        const double vx = hs[h * 5 + 2] - avx, vy = hs[h * 5 + 3] - avy;
        const double d = seg_dist_origin(px, py, px + vx * dt, py + vy * dt) - hs[h * 5 + 4] - r[4];
        if (d < 0.0) { collision = true; break; }          // the reference stops at the first collision
        if (d < dmin) dmin = d;
    }
    const double gx = o.npx - r[5], gy = o.npy - r[6];
    const bool reaching = sqrt(gx * gx + gy * gy) < r[4];
    double rew = 0.0;
    int code = CROWD_INFO_NOTHING, fin = 0;
    if (time >= cfg.time_limit - 1.0) { rew = 0.0; fin = 1; code = CROWD_INFO_TIMEOUT; }
    else if (collision) { rew = cfg.collision_penalty; fin = 1; code = CROWD_INFO_COLLISION; }
    else if (reaching) { rew = cfg.success_reward; fin = 1; code = CROWD_INFO_REACH_GOAL; }
    else if (dmin < cfg.discomfort_dist) { rew = (dmin - cfg.discomfort_dist) * cfg.discomfort_penalty_factor * dt; code = CROWD_INFO_DISCOMFORT; }
    o.reward = rew;
    o.info = code;
    o.fin = fin;
    o.dmin = collision ? -1.0 : dmin;
    return o;
}

// the robot's row after its step (position, velocity and, for a unicycle, heading)
__device__ __forceinline__ void crowd_robot_commit(const CrowdSimConfig& cfg, double* r, const RobotStep& o, double a0, double a1) {
    r[0] = o.npx; r[1] = o.npy;
    if (cfg.kinematics == RGL_HOLONOMIC) { r[2] = a0; r[3] = a1; }
    else { r[8] = o.ntheta; r[2] = a0 * cos(o.ntheta); r[3] = a0 * sin(o.ntheta); }
}

// what human h of an environment does, decided on the state before anyone moves (crowd_sim.py:257-268).  hs [H][5], goals [H][2],
// vpref [H] and given [H][2] are the environment's rows; only the arrays the policy reads are touched (the others may be null)
__device__ __forceinline__ void crowd_human_velocity(const CrowdSimConfig& cfg, const double* hs, const double* goals, const double* vpref,
                                                     const double* given, int h, double& hvx, double& hvy) {
    if (cfg.human_policy == CROWD_HUMAN_LINEAR) {
        const double th = atan2(goals[h * 2 + 1] - hs[h * 5 + 1], goals[h * 2] - hs[h * 5]);
        const double vp = vpref[h];
        hvx = cos(th) * vp; hvy = sin(th) * vp;
    } else if (cfg.human_policy == CROWD_HUMAN_CONSTANT_VELOCITY) {
        hvx = hs[h * 5 + 2]; hvy = hs[h * 5 + 3];
    } else {
        hvx = given[h * 2]; hvy = given[h * 2 + 1];
    }
}

}  // namespace
