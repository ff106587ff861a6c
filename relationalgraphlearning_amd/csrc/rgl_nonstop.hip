// The simulator step with nonstop humans (include/rgl_hip.h has the contract): crowd_step_f64's step -- the same device functions,
// rgl_sim_step.h -- and, in the same launch, upstream's regeneration of every human that reaches its goal
// (crowd_sim/envs/crowd_sim.py:346-349: `human.step(action); if nonstop and human.reached_destination(): generate_human(human)`),
// drawn from the environment's own numpy stream with the scene generator's rejection loop (rgl_scene_place.h).
//
// Mapping: one environment per wave, one workgroup of 64 lanes each.  A human's action is decided on the state before anyone moves
// and its arrival depends on its own step alone, so lane h moves human h (and h + 64) and tests its arrival in parallel; what
// upstream's human order decides is the CLEARANCE LIST of a regeneration, and only that part runs in index order: for an arrived
// human i the list holds the robot at its new position, humans before i as their steps and regenerations left them, human i itself
// where it just arrived (old goal, new radius) and humans after i where they stood before the step.  The list lives in LDS
// (SceneLds, agent 0 = the robot, agent 1 + h = human h) and starts as the state before the step; `front` counts the humans already
// moved in it.  Most steps have no arrival: then neither the list nor the stream's 624 words are touched, the words stay in global
// memory and only the position moves by the policy's draws.  On the first arrival (or when the policy's draws cross a block) the
// words come into LDS, as next_u32 of rgl_explore.hip brings them, and go back at the end.
//
// The arrival test and the clearance tests round like numpy (closer_than: no contraction, correctly rounded sqrt).
#include "rgl_common.h"
#include "rgl_mt19937.h"
#include "rgl_scene_place.h"
#include "rgl_sim_step.h"

namespace {

constexpr int kStateWords = CROWD_EXPLORE_STATE_WORDS;
static_assert(kStateWords == kMtN + 1, "state = 624 words and the position");
constexpr int kSlots = RGL_MAX_NODES / kWave;        // humans per lane: h = lane + 64 * slot
static_assert(kSlots * kWave == RGL_MAX_NODES, "every human has a lane and a slot");

struct NonstopArgs {
    CrowdSimConfig sim;
    CrowdSceneConfig scene;
    double *robot, *humans, *goals, *vpref;
    const double *robot_action, *human_actions;
    double* time;
    int* done;
    unsigned* state;
    int *status, *attempts;
    float* reward;
    int* info;
    double* dmin;
    int H, policy_draws;
};

__device__ void words_to_lds(SceneLds& s, const unsigned* global, bool& in_lds, int lane) {
    if (in_lds) return;
    for (int k = lane; k < kMtN; k += kWave) s.mt[k] = global[k];
    __syncthreads();
    in_lds = true;
}

__global__ __launch_bounds__(kWave) void crowd_step_nonstop_kernel(const NonstopArgs a) {
    __shared__ SceneLds s;
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    const int H = a.H;
    int* attempts = a.attempts ? a.attempts + b * H : nullptr;
    if (__builtin_amdgcn_readfirstlane(a.done[b]) != 0) {        // finished episodes are frozen and draw nothing
        if (lane == 0) {
            a.reward[b] = 0.f;
            a.info[b] = CROWD_INFO_DONE;
            a.dmin[b] = INFINITY;
        }
        if (attempts)
            for (int h = lane; h < H; h += kWave) attempts[h] = 0;
        return;
    }
    const CrowdSimConfig& cfg = a.sim;
    const CrowdSceneConfig& scene = a.scene;
    double* r = a.robot + b * 9;
    double* hs = a.humans + b * H * 5;
    double* goals = a.goals + b * H * 2;
    double* vpref = a.vpref + b * H;
    const double* given = a.human_actions ? a.human_actions + b * H * 2 : nullptr;
    unsigned* global = a.state + b * kStateWords;
    const double dt = cfg.time_step;

    // 1. the policy's draws of this decision
    Stream st{__builtin_amdgcn_readfirstlane((int)global[kMtN]), 0};
    if (st.pos < 0 || st.pos > kMtN) st.pos = kMtN;              // never index past the words, whatever the caller left there
    bool in_lds = false;
    long long ahead = 2ll * a.policy_draws + st.pos;             // in words from the start of the current block
    while (ahead > kMtN) {
        words_to_lds(s, global, in_lds, lane);
        mt_twist(s.mt, lane);
        ahead -= kMtN;
    }
    st.pos = (int)ahead;

    // 2. the robot's step and the ladder (every lane the same values), each lane's humans moved in registers.  Every lane reads the
    // robot's and all humans' rows here and other lanes store them in part 4 with no barrier in between when nobody arrives: that
    // is in order only because the workgroup is exactly ONE wave (__launch_bounds__(kWave), launched with kWave threads), whose
    // lanes execute the loads before the stores.  A wider block needs a __syncthreads() before part 4.
    const double a0 = a.robot_action[2 * b], a1 = a.robot_action[2 * b + 1];
    const RobotStep o = crowd_robot_step(cfg, r, hs, H, a0, a1, a.time[b]);
    double npx[kSlots], npy[kSlots], hvx[kSlots], hvy[kSlots], new_vpref[kSlots];
    bool arrived[kSlots], regenerated[kSlots];
    bool any = false;
    for (int q = 0; q < kSlots; ++q) {
        const int h = lane + kWave * q;
        arrived[q] = regenerated[q] = false;
        npx[q] = npy[q] = hvx[q] = hvy[q] = new_vpref[q] = 0.0;
        if (h < H) {
            crowd_human_velocity(cfg, hs, goals, vpref, given, h, hvx[q], hvy[q]);
            npx[q] = hs[h * 5] + hvx[q] * dt;
            npy[q] = hs[h * 5 + 1] + hvy[q] * dt;
            arrived[q] = closer_than(npx[q] - goals[h * 2], npy[q] - goals[h * 2 + 1], hs[h * 5 + 4]);
            if (attempts) attempts[h] = 0;
        }
        any = any || arrived[q];
    }
    int flagged = 0;
    if (__ballot(any) != 0ull) {                                 // wave-uniform: the barriers below are met by every lane
        // 3. the clearance list as it stands before any human has moved
        words_to_lds(s, global, in_lds, lane);
        if (lane == 0) s.px[0] = o.npx, s.py[0] = o.npy, s.gx[0] = r[5], s.gy[0] = r[6], s.rad[0] = r[4];
        for (int h = lane; h < H; h += kWave)
            s.px[1 + h] = hs[h * 5], s.py[1 + h] = hs[h * 5 + 1], s.gx[1 + h] = goals[h * 2], s.gy[1 + h] = goals[h * 2 + 1],
                     s.rad[1 + h] = hs[h * 5 + 4];
        __syncthreads();
        int front = 0;                                           // humans [0, front) of the list have moved
        for (int q = 0; q < kSlots; ++q) {
            unsigned long long todo = __ballot(arrived[q]);      // humans 64 q + lane, in index order
            while (todo) {
                const int owner = __ffsll(todo) - 1;
                todo &= todo - 1;
                const int i = kWave * q + owner;
                for (int p = 0; p < kSlots; ++p) {               // humans front .. i step: their new positions enter the list
                    const int h = lane + kWave * p;
                    if (h >= front && h <= i) s.px[1 + h] = npx[p], s.py[1 + h] = npy[p];
                }
                front = i + 1;
                __syncthreads();
                Human hm{vpref[i], s.rad[1 + i], 1.0, 0.0, 0.0, 0};
                if (scene.randomize_attributes) {
                    redraw_attributes(s, st, hm, lane);
                    __syncthreads();                             // every lane has read the old radius
                    if (lane == 0) s.rad[1 + i] = hm.radius;
                    __syncthreads();
                }
                double px = 0.0, py = 0.0, gx = 0.0, gy = 0.0;
                bool placed;
                if (scene.scenario == CROWD_SCENARIO_CIRCLE_CROSSING) {
                    placed = place<PLACE_CIRCLE>(scene, s, st, hm, H + 1, lane);
                    px = hm.x, py = hm.y, gx = -px, gy = -py;
                } else {
                    hm.sign = draw(s, st, lane) > 0.5 ? -1.0 : 1.0;
                    placed = place<PLACE_SQUARE_POSITION>(scene, s, st, hm, H + 1, lane);
                    px = hm.x, py = hm.y;
                    placed = placed && place<PLACE_SQUARE_GOAL>(scene, s, st, hm, H + 1, lane);
                    gx = hm.x, gy = hm.y;
                }
                __syncthreads();                                 // the last round's reads of the list are over
                if (placed && lane == 0) s.px[1 + i] = px, s.py[1 + i] = py, s.gx[1 + i] = gx, s.gy[1 + i] = gy;
                if (lane == owner) {
                    regenerated[q] = placed;
                    new_vpref[q] = hm.v_pref;
                    if (attempts) attempts[i] = hm.attempts;
                    if (!placed && scene.randomize_attributes) vpref[i] = hm.v_pref;      // the attributes were drawn before the loop
                }
                if (!placed) flagged = 1;
                __syncthreads();
            }
        }
    }

    // 4. everybody's new state
    for (int q = 0; q < kSlots; ++q) {
        const int h = lane + kWave * q;
        if (h >= H) continue;
        if (regenerated[q]) {
            hs[h * 5] = s.px[1 + h], hs[h * 5 + 1] = s.py[1 + h], hs[h * 5 + 2] = 0.0, hs[h * 5 + 3] = 0.0, hs[h * 5 + 4] = s.rad[1 + h];
            goals[h * 2] = s.gx[1 + h], goals[h * 2 + 1] = s.gy[1 + h];
            vpref[h] = new_vpref[q];
        } else {
            hs[h * 5] = npx[q], hs[h * 5 + 1] = npy[q], hs[h * 5 + 2] = hvx[q], hs[h * 5 + 3] = hvy[q];
            if (arrived[q]) hs[h * 5 + 4] = s.rad[1 + h];        // at the cap: the redrawn radius stays
        }
    }
    if (in_lds) {
        __syncthreads();
        for (int k = lane; k < kMtN; k += kWave) global[k] = s.mt[k];
    }
    if (lane == 0) {
        global[kMtN] = (unsigned)st.pos;
        if (flagged) a.status[b] = 1;
        a.reward[b] = (float)o.reward;
        a.info[b] = o.info;
        a.dmin[b] = o.dmin;
        crowd_robot_commit(cfg, r, o, a0, a1);
        a.time[b] += dt;
        a.done[b] = o.fin;
    }
}

}  // namespace

extern "C" int crowd_step_nonstop_f64(const CrowdNonstopJob* job) {
    if (!job) return RGL_ERR_NULL;
    if (!job->robot || !job->humans || !job->human_goals || !job->human_vpref || !job->robot_action || !job->time || !job->done ||
        !job->state || !job->status || !job->reward || !job->info || !job->dmin)
        return RGL_ERR_NULL;
    if (job->B < 1 || job->H < 1 || job->H + 1 > RGL_MAX_NODES || job->policy_draws < 0 || job->scene.max_attempts < 1)
        return RGL_ERR_BAD_SHAPE;
    const CrowdSimConfig& cfg = job->sim;
    if (cfg.kinematics != RGL_HOLONOMIC && cfg.kinematics != RGL_UNICYCLE) return RGL_ERR_BAD_MODE;
    if (cfg.human_policy < CROWD_HUMAN_GIVEN || cfg.human_policy > CROWD_HUMAN_CONSTANT_VELOCITY) return RGL_ERR_BAD_MODE;
    if (cfg.human_policy == CROWD_HUMAN_GIVEN && !job->human_actions) return RGL_ERR_NULL;
    if (job->scene.scenario != CROWD_SCENARIO_CIRCLE_CROSSING && job->scene.scenario != CROWD_SCENARIO_SQUARE_CROSSING)
        return RGL_ERR_BAD_MODE;
    NonstopArgs a;
    a.sim = job->sim, a.scene = job->scene;
    a.robot = job->robot, a.humans = job->humans, a.goals = job->human_goals, a.vpref = job->human_vpref;
    a.robot_action = job->robot_action, a.human_actions = job->human_actions;
    a.time = job->time, a.done = job->done, a.state = job->state, a.status = job->status, a.attempts = job->attempts;
    a.reward = job->reward, a.info = job->info, a.dmin = job->dmin;
    a.H = job->H, a.policy_draws = job->policy_draws;
    hipLaunchKernelGGL(crowd_step_nonstop_kernel, dim3((unsigned)job->B), dim3(kWave), 0, (hipStream_t)job->stream, a);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}
