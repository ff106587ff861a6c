// The one-step search of MultiHumanRL.predict (crowd_nav/policy/multi_human_rl.py:36-64): prepare -> value network -> select.
// Path G (gcn_predict_f32, rgl_tree.hip) and SARL / OM-SARL (sarl_predict_f32, rgl_sarl.hip) differ in the value network between
// the two steps alone; the steps, their launchers and the workspace buffers both searches begin with are written here once.
#pragma once
#include "rgl_rotate.h"
#include "rgl_tail.h"

namespace {

// One thread per (scene, action, human): propagate, rotate; thread h == 0 also does compute_reward.
__global__ void gcn_prepare_kernel(const float* __restrict__ robot, const float* __restrict__ humans,
                                   const double* __restrict__ robot64, const double* __restrict__ humans64,
                                   const double* __restrict__ actions, int B, int H, int A, int kinematics, double dt,
                                   float* __restrict__ self6, float* __restrict__ hum7, float* __restrict__ reward) {
    // python-float arithmetic: every float64 product and sum below is rounded on its own (a contracted end-point clearance turns an
    // exact contact, clearance 0, into a collision)
#pragma clang fp contract(off)
    // blockDim.x is a multiple of H: the H threads of a (root, action) pair sit in one workgroup, each contributes ITS human's
    // end-point clearance (one float64 sqrt per thread) and thread h == 0 takes the minimum -- it used to walk all H itself
    extern __shared__ double clearance[];
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < (long long)B * A * H;
    const long long cidx = live ? idx : 0;
    const int h = (int)(cidx % H);
    const long long sa = cidx / H;
    const int a = (int)(sa % A), b = (int)(sa / A);
    const float* r = robot + (size_t)b * 9;
    const double* r64 = robot64 ? robot64 + (size_t)b * 9 : nullptr;        // the float64 state the fp32 row was rounded from
    auto R = [&](int i) { return r64 ? r64[i] : (double)r[i]; };
    const double a0 = actions[2 * a], a1 = actions[2 * a + 1];
    // CADRL.propagate in float64, as python floats
    double nr[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) nr[i] = R(i);
    if (kinematics == RGL_HOLONOMIC) {
        nr[0] = R(0) + a0 * dt;
        nr[1] = R(1) + a1 * dt;
        nr[2] = a0;
        nr[3] = a1;
    } else {
        const double th = R(8) + a1;
        nr[2] = a0 * cos(th);
        nr[3] = a0 * sin(th);
        nr[0] = R(0) + nr[2] * dt;
        nr[1] = R(1) + nr[3] * dt;
        nr[8] = th;
    }
    const float* hu = humans + ((size_t)b * H + h) * 5;
    const double* hb64 = humans64 ? humans64 + (size_t)b * H * 5 : nullptr;
    auto HB = [&](int j, int i) { return hb64 ? hb64[j * 5 + i] : (double)humans[((size_t)b * H + j) * 5 + i]; };
    float s[14], o[13];
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i] = (float)nr[i];
    s[9] = (float)(HB(h, 0) + HB(h, 2) * dt);
    s[10] = (float)(HB(h, 1) + HB(h, 3) * dt);
    s[11] = hb64 ? (float)HB(h, 2) : hu[2];
    s[12] = hb64 ? (float)HB(h, 3) : hu[3];
    s[13] = hb64 ? (float)HB(h, 4) : hu[4];
    rotate_row(s, kinematics == RGL_UNICYCLE, o);
    if (live) {
        float* h7 = hum7 + ((size_t)sa * H + h) * 7;
#pragma unroll
        for (int i = 0; i < 7; ++i) h7[i] = o[6 + i];
    }
    {   // compute_reward (multi_human_rl.py:73-96): END-point distance of my human, float64
        const double hx = HB(h, 0) + HB(h, 2) * dt;
        const double hy = HB(h, 1) + HB(h, 3) * dt;
        const double ddx = nr[0] - hx, ddy = nr[1] - hy;
        clearance[threadIdx.x] = sqrt(ddx * ddx + ddy * ddy) - nr[4] - HB(h, 4);
    }
    __syncthreads();
    if (live && h == 0) {
        float* s6 = self6 + (size_t)sa * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) s6[i] = o[i];
        bool collision = false;
        double dmin = INFINITY;
        for (int j = 0; j < H; ++j) {
            const double d = clearance[threadIdx.x + j];
            if (d < 0.0) collision = true;
            if (d < dmin) dmin = d;
        }
        const double gx = nr[0] - nr[5], gy = nr[1] - nr[6];
        const bool reaching = sqrt(gx * gx + gy * gy) < nr[4];
        double rew;
        if (collision) rew = -0.25;
        else if (reaching) rew = 1.0;
        else if (dmin < 0.2) rew = (dmin - 0.2) * 0.5 * dt;
        else rew = 0.0;
        reward[sa] = (float)rew;
    }
}

// `robot64` / `humans64`: the float64 roots, read instead of the float32 rows when BOTH are given
inline int launch_gcn_prepare(int kinematics, int A, double dt, const double* actions, const double* robot64, const double* humans64,
                              const float* robot, const float* humans, int B, int H, float* self6, float* hum7, float* reward,
                              hipStream_t st) {
    const long long threads = (long long)B * A * H;
    const int block = (H >= 256 ? 1 : 256 / H) * H;        // whole (root, action) groups per workgroup
    const bool r64 = robot64 && humans64;
    hipLaunchKernelGGL(gcn_prepare_kernel, dim3((unsigned)((threads + block - 1) / block)), dim3(block), block * sizeof(double), st,
                       robot, humans, r64 ? robot64 : nullptr, r64 ? humans64 : nullptr, actions, B, H, A, kinematics, dt, self6, hum7,
                       reward);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

// value = reward + gamma^(dt v_pref) V in float64 (multi_human_rl.py:58) and the strict `>` walk of :60-64: 16 lanes per root
// (kRootLanes) take the A action values side by side, then a first-maximum reduction -- one thread walking 81 actions cost 25 us
// per call.  `best_attention` (or null; SARL): row best_action of `attention` [B][A][H], zeros where no action was chosen.
__global__ void onestep_select_kernel(const float* __restrict__ robot, const float* __restrict__ reward, const float* __restrict__ value,
                                      const float* __restrict__ attention, int B, int A, int H, double gamma, double dt,
                                      float* __restrict__ action_values, int* __restrict__ best_action, float* __restrict__ best_value,
                                      float* __restrict__ best_attention) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = t / kRootLanes, sub = t % kRootLanes;
    const bool live = b < B;
    double best = -INFINITY;
    int ba = -1;
    if (live) {
        const double disc = pow(gamma, dt * (double)robot[(size_t)b * 9 + 7]);
        for (int a = sub; a < A; a += kRootLanes) {
            const double v = (double)reward[(size_t)b * A + a] + disc * (double)value[(size_t)b * A + a];
            action_values[(size_t)b * A + a] = (float)v;
            if (v > best) {
                best = v;
                ba = a;
            }
        }
    }
#pragma unroll
    for (int m = kRootLanes / 2; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(best, m);
        const int oa = __shfl_xor(ba, m);
        const bool take = oa >= 0 && (ba < 0 || ov > best || (ov == best && oa < ba));
        if (take) {
            best = ov;
            ba = oa;
        }
    }
    if (live) {
        if (sub == 0) {
            best_action[b] = ba;
            if (best_value) best_value[b] = ba >= 0 ? (float)best : 0.f;      // = action_values[b][ba]: what callers used to gather
        }
        if (best_attention)
            for (int h = sub; h < H; h += kRootLanes)
                best_attention[(size_t)b * H + h] = ba >= 0 ? attention[((size_t)b * A + ba) * H + h] : 0.f;
    }
}

inline int launch_onestep_select(const float* robot, const float* reward, const float* value, const float* attention, int B, int A,
                                 int H, double gamma, double dt, float* action_values, int* best_action, float* best_value,
                                 float* best_attention, hipStream_t st) {
    hipLaunchKernelGGL(onestep_select_kernel, dim3((unsigned)(((long long)B * kRootLanes + 255) / 256)), dim3(256), 0, st, robot, reward,
                       value, attention, B, A, H, gamma, dt, action_values, best_action, best_value, best_attention);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

// what both searches' workspaces begin with, for S = B A candidate scenes of H humans
struct OneStepScratch {
    float* self6;       // [S][6]
    float* hum7;        // [S][H][7]
    float* reward;      // [S]
    float* value;       // [S]
    long long bytes;
};

inline OneStepScratch carve_onestep(void* base, long long S, int H) {
    Carver c{(char*)base, 0};
    OneStepScratch w;
    w.self6 = c.take<float>(S * 6 * 4);
    w.hum7 = c.take<float>(S * H * 7 * 4);
    w.reward = c.take<float>(S * 4);
    w.value = c.take<float>(S * 4);
    w.bytes = c.off;
    return w;
}

}  // namespace
