// rgl_orca.hip -- ORCA (optimal reciprocal collision avoidance) for the crowd simulator's agents, on device.
// One thread per (environment, agent) computes that agent's new velocity exactly as RVO2 2.0's doStep does for an agent
// without obstacles (Agent::computeNeighbors, Agent::computeNewVelocity, linearProgram1/2/3), written from the algorithm's
// statement: every quantity is a float32 rounded once from the caller's float64, every operation is an individually rounded
// float32 operation (no contraction, correctly rounded division and square root), so the result is what Python-RVO2 returns.
// The one known difference: RVO2 finds the neighbours by walking a kd-tree, this kernel walks the agents in index order;
// the kept set and its order can differ only when two candidates lie at exactly the same distance at the cut-off.
//
// Follows (reference paths): crowd_sim/envs/policy/orca.py:75-161 (ORCA.predict, CentralizedORCA.predict) as
// crowd_sim/envs/crowd_sim.py:256-262 (step) calls them.
//
// Per thread the neighbour list, the ORCA lines and LP3's projected lines live in LDS as thread-minor structure-of-arrays
// (field f of entry k of thread t at [(4k + f) * blockDim + t]): the lanes of a wave touch consecutive dwords, no bank
// conflicts, whatever data-dependent entry each lane is at.  The neighbour list (distSq, index) shares the projected lines'
// space: it is consumed while the ORCA lines are built, before LP3 projects anything.
#include "rgl_common.h"

namespace {

constexpr float kRvoEpsilon = 1e-5f;
constexpr int kOrcaBlock = 64;            // one wave per block: max_neighbors 32 -> 64 KiB of LDS per block

struct V2 { float x, y; };

// RVO2's Vector2 arithmetic.  `a / s` multiplies by 1.0f / s (Vector2::operator/), `normalize(v)` is v / abs(v).
__device__ __forceinline__ V2 sub(V2 a, V2 b) {
#pragma clang fp contract(off)
    return {a.x - b.x, a.y - b.y};
}
__device__ __forceinline__ V2 add(V2 a, V2 b) {
#pragma clang fp contract(off)
    return {a.x + b.x, a.y + b.y};
}
__device__ __forceinline__ V2 scale(float s, V2 a) {
#pragma clang fp contract(off)
    return {a.x * s, a.y * s};
}
__device__ __forceinline__ float dot(V2 a, V2 b) {
#pragma clang fp contract(off)
    return a.x * b.x + a.y * b.y;
}
__device__ __forceinline__ float det(V2 a, V2 b) {
#pragma clang fp contract(off)
    return a.x * b.y - a.y * b.x;
}
__device__ __forceinline__ float abs_sq(V2 a) {
#pragma clang fp contract(off)
    return a.x * a.x + a.y * a.y;
}
__device__ __forceinline__ V2 div(V2 a, float s) {
#pragma clang fp contract(off)
    const float inv = 1.0f / s;
    return {a.x * inv, a.y * inv};
}
__device__ __forceinline__ V2 normalize(V2 a) { return div(a, sqrtf(abs_sq(a))); }

// one thread's lines in LDS: entry k at base[(4k + f) * stride], f = point.x, point.y, direction.x, direction.y
struct Lines {
    float* base;
    int stride;
    __device__ V2 point(int k) const { return {base[(4 * k) * stride], base[(4 * k + 1) * stride]}; }
    __device__ V2 dir(int k) const { return {base[(4 * k + 2) * stride], base[(4 * k + 3) * stride]}; }
    __device__ void set(int k, V2 p, V2 d) const {
        base[(4 * k) * stride] = p.x;
        base[(4 * k + 1) * stride] = p.y;
        base[(4 * k + 2) * stride] = d.x;
        base[(4 * k + 3) * stride] = d.y;
    }
};

__device__ bool linear_program1(const Lines& L, int line, float radius, V2 opt, bool direction_opt, V2& result) {
#pragma clang fp contract(off)
    const V2 p = L.point(line), d = L.dir(line);
    const float dp = dot(p, d);
    const float disc = dp * dp + radius * radius - abs_sq(p);
    if (disc < 0.0f) return false;                 // the max-speed circle misses the line entirely
    const float sd = sqrtf(disc);
    float t_left = -dp - sd, t_right = -dp + sd;
    for (int i = 0; i < line; ++i) {
        const V2 pi = L.point(i), di = L.dir(i);
        const float den = det(d, di);
        const float num = det(di, sub(p, pi));
        if (fabsf(den) <= kRvoEpsilon) {           // (almost) parallel lines
            if (num < 0.0f) return false;
            continue;
        }
        const float t = num / den;
        if (den >= 0.0f) t_right = t < t_right ? t : t_right;          // std::min(t_right, t)
        else t_left = t_left < t ? t : t_left;                         // std::max(t_left, t)
        if (t_left > t_right) return false;
    }
    if (direction_opt) {
        result = add(p, scale(dot(opt, d) > 0.0f ? t_right : t_left, d));
    } else {
        const float t = dot(d, sub(opt, p));
        result = add(p, scale(t < t_left ? t_left : (t > t_right ? t_right : t), d));
    }
    return true;
}

__device__ int linear_program2(const Lines& L, int n, float radius, V2 opt, bool direction_opt, V2& result) {
#pragma clang fp contract(off)
    if (direction_opt) result = scale(radius, opt);
    else if (abs_sq(opt) > radius * radius) result = scale(radius, normalize(opt));
    else result = opt;
    for (int i = 0; i < n; ++i) {
        if (det(L.dir(i), sub(L.point(i), result)) > 0.0f) {     // the result violates line i
            const V2 keep = result;
            if (!linear_program1(L, i, radius, opt, direction_opt, result)) {
                result = keep;
                return i;
            }
        }
    }
    return n;
}

__device__ void linear_program3(const Lines& L, const Lines& P, int n, int begin, float radius, V2& result) {
#pragma clang fp contract(off)
    float distance = 0.0f;
    for (int i = begin; i < n; ++i) {
        const V2 pi = L.point(i), di = L.dir(i);
        if (det(di, sub(pi, result)) > distance) {
            int np = 0;
            for (int j = 0; j < i; ++j) {
                const V2 pj = L.point(j), dj = L.dir(j);
                V2 point;
                const float den = det(di, dj);
                if (fabsf(den) <= kRvoEpsilon) {
                    if (dot(di, dj) > 0.0f) continue;              // same direction: line j is implied
                    point = scale(0.5f, add(pi, pj));
                } else {
                    point = add(pi, scale(det(dj, sub(pi, pj)) / den, di));
                }
                P.set(np++, point, normalize(sub(dj, di)));
            }
            const V2 keep = result;
            if (linear_program2(P, np, radius, V2{-di.y, di.x}, true, result) < np) result = keep;
            distance = det(di, sub(pi, result));
        }
    }
}

// float64 -> float32 agent view of one environment: agents [0, H) are the humans and agent H the robot (humans entry), or
// agent 0 the robot and agents [1, H] the humans (robot entry)
struct Crowd {
    const double* robot;      // [9]
    const double* humans;     // [H][5]
    int H;
    bool robot_first;
    __device__ const double* row(int a) const {
        if (robot_first) return a == 0 ? robot : humans + (size_t)(a - 1) * 5;
        return a == H ? robot : humans + (size_t)a * 5;
    }
};

// radius as ORCA.predict adds it: radius + 0.01 + safety_space in float64, then rounded
__device__ __forceinline__ float orca_radius(double r, double safety) {
#pragma clang fp contract(off)
    return (float)(r + 0.01 + safety);
}

// preferred velocity toward the goal in float64 (`velocity / speed if speed > 1`), then rounded
__device__ __forceinline__ V2 orca_pref(double px, double py, double gx, double gy) {
#pragma clang fp contract(off)
    double dx = gx - px, dy = gy - py;
    const double speed = sqrt(dx * dx + dy * dy);
    if (speed > 1.0) { dx = dx / speed; dy = dy / speed; }
    return {(float)dx, (float)dy};
}

// new velocity of agent `self` among `n_agents` (RVO2 Agent::computeNeighbors + computeNewVelocity, no obstacles)
__device__ V2 orca_new_velocity(const CrowdOrcaParams& prm, const Crowd& c, int n_agents, int self, V2 pref, float max_speed,
                                float* lds) {
#pragma clang fp contract(off)
    const int stride = blockDim.x;
    const Lines lines{lds + threadIdx.x, stride};
    const Lines proj{lds + (size_t)4 * prm.max_neighbors * stride + threadIdx.x, stride};
    float* nd = proj.base;                                   // neighbour k: distSq at [2k], agent index at [2k + 1]
    const double* me = c.row(self);
    const V2 pos{(float)me[0], (float)me[1]}, vel{(float)me[2], (float)me[3]};
    const float radius = orca_radius(me[4], prm.safety_space);
    const float nbr_dist = (float)prm.neighbor_dist;
    const int maxn = prm.max_neighbors;

    // neighbours: the maxn nearest within neighbor_dist, ascending distSq (KdTree::queryAgentTreeRecursive's insertion)
    int nn = 0;
    if (maxn > 0) {
        float range_sq = nbr_dist * nbr_dist;
        for (int a = 0; a < n_agents; ++a) {
            if (a == self) continue;
            const double* o = c.row(a);
            const float dsq = abs_sq(sub(pos, V2{(float)o[0], (float)o[1]}));
            if (!(dsq < range_sq)) continue;
            if (nn < maxn) ++nn;
            int k = nn - 1;
            while (k != 0 && dsq < nd[(2 * (k - 1)) * stride]) {
                nd[(2 * k) * stride] = nd[(2 * (k - 1)) * stride];
                nd[(2 * k + 1) * stride] = nd[(2 * (k - 1) + 1) * stride];
                --k;
            }
            nd[(2 * k) * stride] = dsq;
            nd[(2 * k + 1) * stride] = __int_as_float(a);
            if (nn == maxn) range_sq = nd[(2 * (nn - 1)) * stride];
        }
    }

    // one ORCA half-plane per neighbour, in list order
    const float inv_th = 1.0f / (float)prm.time_horizon;
    const float inv_dt = 1.0f / (float)prm.time_step;
    for (int k = 0; k < nn; ++k) {
        const double* o = c.row(__float_as_int(nd[(2 * k + 1) * stride]));
        const V2 rel_pos = sub(V2{(float)o[0], (float)o[1]}, pos);
        const V2 rel_vel = sub(vel, V2{(float)o[2], (float)o[3]});
        const float dist_sq = abs_sq(rel_pos);
        const float R = radius + orca_radius(o[4], prm.safety_space);
        const float R_sq = R * R;
        V2 direction, u;
        if (dist_sq > R_sq) {                                // no collision
            const V2 w = sub(rel_vel, scale(inv_th, rel_pos));
            const float w_len_sq = abs_sq(w);
            const float dp1 = dot(w, rel_pos);
            if (dp1 < 0.0f && dp1 * dp1 > R_sq * w_len_sq) {      // project on the cut-off circle
                const float w_len = sqrtf(w_len_sq);
                const V2 unit_w = div(w, w_len);
                direction = {unit_w.y, -unit_w.x};
                u = scale(R * inv_th - w_len, unit_w);
            } else {                                          // project on a leg
                const float leg = sqrtf(dist_sq - R_sq);
                if (det(rel_pos, w) > 0.0f)
                    direction = div(V2{rel_pos.x * leg - rel_pos.y * R, rel_pos.x * R + rel_pos.y * leg}, dist_sq);
                else
                    direction = div(V2{-(rel_pos.x * leg + rel_pos.y * R), -(-rel_pos.x * R + rel_pos.y * leg)}, dist_sq);
                u = sub(scale(dot(rel_vel, direction), direction), rel_vel);
            }
        } else {                                             // collision: the cut-off circle of one time step
            const V2 w = sub(rel_vel, scale(inv_dt, rel_pos));
            const float w_len = sqrtf(abs_sq(w));
            const V2 unit_w = div(w, w_len);
            direction = {unit_w.y, -unit_w.x};
            u = scale(R * inv_dt - w_len, unit_w);
        }
        lines.set(k, add(vel, scale(0.5f, u)), direction);
    }

    V2 result;
    const int fail = linear_program2(lines, nn, max_speed, pref, false, result);
    if (fail < nn) linear_program3(lines, proj, nn, fail, max_speed, result);
    return result;
}

// humans entry: thread (b, h) for h < H; the robot, when visible, is agent H
__global__ void crowd_orca_humans_kernel(const CrowdOrcaParams prm, const double* __restrict__ robot,
                                         const double* __restrict__ humans, const double* __restrict__ human_goals,
                                         const double* __restrict__ human_vpref, const int* __restrict__ done, int B, int H,
                                         int robot_visible, double* __restrict__ out) {
    extern __shared__ float orca_lds[];
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * H) return;
    const int b = (int)(gid / H), h = (int)(gid % H);
    if (done && done[b]) return;
    const Crowd c{robot + (size_t)b * 9, humans + (size_t)b * H * 5, H, false};
    const double* me = c.row(h);
    const double* g = human_goals + ((size_t)b * H + h) * 2;
    const V2 pref = orca_pref(me[0], me[1], g[0], g[1]);
    const float max_speed = prm.max_speed_rule == CROWD_ORCA_MAX_SPEED_VPREF ? (float)human_vpref[(size_t)b * H + h] : 1.0f;
    const V2 v = orca_new_velocity(prm, c, H + (robot_visible ? 1 : 0), h, pref, max_speed, orca_lds);
    out[gid * 2] = (double)v.x;
    out[gid * 2 + 1] = (double)v.y;
}

// robot entry: thread b; agent 0 is the robot (max_speed = its v_pref), the humans' preferred velocities are (0, 0) and do not
// enter agent 0's answer
__global__ void crowd_orca_robot_kernel(const CrowdOrcaParams prm, const double* __restrict__ robot,
                                        const double* __restrict__ humans, const int* __restrict__ done, int B, int H,
                                        double* __restrict__ out) {
    extern __shared__ float orca_lds[];
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (done && done[b]) return;
    const double* r = robot + (size_t)b * 9;
    const Crowd c{r, humans + (size_t)b * H * 5, H, true};
    const V2 pref = orca_pref(r[0], r[1], r[5], r[6]);
    const V2 v = orca_new_velocity(prm, c, H + 1, 0, pref, (float)r[7], orca_lds);
    out[(size_t)b * 2] = (double)v.x;
    out[(size_t)b * 2 + 1] = (double)v.y;
}

int check_params(const CrowdOrcaParams* prm) {
    if (prm->max_neighbors < 0 || prm->max_neighbors > CROWD_ORCA_MAX_NEIGHBORS) return RGL_ERR_BAD_SHAPE;
    if (prm->max_speed_rule != CROWD_ORCA_MAX_SPEED_ONE && prm->max_speed_rule != CROWD_ORCA_MAX_SPEED_VPREF) return RGL_ERR_BAD_MODE;
    return RGL_OK;
}

size_t lds_bytes(const CrowdOrcaParams* prm) {
    return (size_t)kOrcaBlock * prm->max_neighbors * 8 * sizeof(float);   // lines + projected lines, 4 floats each
}

}  // namespace

extern "C" int crowd_orca_humans_f64(const CrowdOrcaParams* params, const double* robot, const double* humans,
                                     const double* human_goals, const double* human_vpref, const int* done, int B, int H,
                                     int robot_visible, double* out, rgl_stream_t stream) {
    if (!params || !robot || !humans || !human_goals || !out) return RGL_ERR_NULL;
    if (B < 1 || H < 1) return RGL_ERR_BAD_SHAPE;
    const int rc = check_params(params);
    if (rc) return rc;
    if (params->max_speed_rule == CROWD_ORCA_MAX_SPEED_VPREF && !human_vpref) return RGL_ERR_NULL;
    const long long n = (long long)B * H;
    hipLaunchKernelGGL(crowd_orca_humans_kernel, dim3((unsigned)((n + kOrcaBlock - 1) / kOrcaBlock)), dim3(kOrcaBlock),
                       lds_bytes(params), (hipStream_t)stream, *params, robot, humans, human_goals, human_vpref, done, B, H,
                       robot_visible, out);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

extern "C" int crowd_orca_robot_f64(const CrowdOrcaParams* params, const double* robot, const double* humans, const int* done,
                                    int B, int H, double* out, rgl_stream_t stream) {
    if (!params || !robot || !humans || !out) return RGL_ERR_NULL;
    if (B < 1 || H < 1) return RGL_ERR_BAD_SHAPE;
    const int rc = check_params(params);
    if (rc) return rc;
    hipLaunchKernelGGL(crowd_orca_robot_kernel, dim3((B + kOrcaBlock - 1) / kOrcaBlock), dim3(kOrcaBlock), lds_bytes(params),
                       (hipStream_t)stream, *params, robot, humans, done, B, H, out);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}
