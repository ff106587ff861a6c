// rgl_sim.hip -- batched crowd-simulator step: B independent environments advance one time step on device.
// Per environment: human actions (linear-to-goal / constant velocity / supplied), robot-vs-human closest-approach
// test over the step, goal test, the reward / termination ladder with the configured constants, kinematic update of
// every agent, clock.  All arithmetic in float64 like the reference's python floats.
//
// Follows (reference paths): crowd_sim/envs/crowd_sim.py:252-368 (step), crowd_sim/envs/utils/agent.py:113-139
// (compute_position, step), crowd_sim/envs/policy/linear.py:16-22 (Linear.predict), crowd_sim/envs/utils/utils.py:4-26.
#include "rgl_common.h"
#include "rgl_sim_step.h"        // the robot's step, the reward ladder, a human's action

namespace {

// one thread per environment
__global__ void crowd_step_kernel(const CrowdSimConfig cfg, double* __restrict__ robot, double* __restrict__ humans,
                                  const double* __restrict__ human_goals, const double* __restrict__ human_vpref,
                                  const double* __restrict__ robot_action, const double* __restrict__ human_actions,
                                  double* __restrict__ time, int* __restrict__ done, int B, int H, int update,
                                  float* __restrict__ reward, int* __restrict__ info, double* __restrict__ dmin_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (done[b]) {                       // finished episodes are frozen
        reward[b] = 0.f;
        info[b] = CROWD_INFO_DONE;
        dmin_out[b] = INFINITY;
        return;
    }
    double* r = robot + (size_t)b * 9;
    double* hs = humans + (size_t)b * H * 5;
    const double dt = cfg.time_step;
    const double a0 = robot_action[2 * b], a1 = robot_action[2 * b + 1];
    const RobotStep o = crowd_robot_step(cfg, r, hs, H, a0, a1, time[b]);
    reward[b] = (float)o.reward;
    info[b] = o.info;
    dmin_out[b] = o.dmin;
    if (!update) return;
    // humans act on the state BEFORE anyone moves (crowd_sim.py:257-268), then everybody steps
    const double* env_goals = human_goals ? human_goals + (size_t)b * H * 2 : nullptr;
    const double* env_vpref = human_vpref ? human_vpref + (size_t)b * H : nullptr;
    const double* env_given = human_actions ? human_actions + (size_t)b * H * 2 : nullptr;
    for (int h = 0; h < H; ++h) {
        double hvx, hvy;
        crowd_human_velocity(cfg, hs, env_goals, env_vpref, env_given, h, hvx, hvy);
        hs[h * 5] += hvx * dt;
        hs[h * 5 + 1] += hvy * dt;
        hs[h * 5 + 2] = hvx;
        hs[h * 5 + 3] = hvy;
    }
    crowd_robot_commit(cfg, r, o, a0, a1);
    time[b] += dt;
    done[b] = o.fin;
}

__global__ void crowd_observe_kernel(const double* __restrict__ robot, const double* __restrict__ humans, int B, int H,
                                     float* __restrict__ robot32, float* __restrict__ humans32) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * 9) robot32[i] = (float)robot[i];
    if (i < B * H * 5) humans32[i] = (float)humans[i];
}

}  // namespace

extern "C" int crowd_step_f64(const CrowdSimConfig* cfg, double* robot, double* humans, const double* human_goals,
                              const double* human_vpref, const double* robot_action, const double* human_actions,
                              double* time, int* done, int B, int H, int update, float* reward, int* info, double* dmin,
                              rgl_stream_t stream) {
    if (!cfg || !robot || !humans || !robot_action || !time || !done || !reward || !info || !dmin) return RGL_ERR_NULL;
    if (B < 1 || H < 1) return RGL_ERR_BAD_SHAPE;
    if (cfg->kinematics != RGL_HOLONOMIC && cfg->kinematics != RGL_UNICYCLE) return RGL_ERR_BAD_MODE;
    if (cfg->human_policy == CROWD_HUMAN_LINEAR && (!human_goals || !human_vpref)) return RGL_ERR_NULL;
    if (cfg->human_policy == CROWD_HUMAN_GIVEN && update && !human_actions) return RGL_ERR_NULL;
    if (cfg->human_policy < CROWD_HUMAN_GIVEN || cfg->human_policy > CROWD_HUMAN_CONSTANT_VELOCITY) return RGL_ERR_BAD_MODE;
    hipLaunchKernelGGL(crowd_step_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)stream, *cfg, robot, humans,
                       human_goals, human_vpref, robot_action, human_actions, time, done, B, H, update, reward, info, dmin);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

extern "C" int crowd_observe_f32(const double* robot, const double* humans, int B, int H, float* robot32, float* humans32,
                                 rgl_stream_t stream) {
    if (!robot || !humans || !robot32 || !humans32) return RGL_ERR_NULL;
    if (B < 1 || H < 1) return RGL_ERR_BAD_SHAPE;
    const int n = B * (H * 5 > 9 ? H * 5 : 9);
    hipLaunchKernelGGL(crowd_observe_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, robot, humans, B, H,
                       robot32, humans32);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}
