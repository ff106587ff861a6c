// Seeded scene generation on device: CrowdSim.reset's generate_human loop (crowd_sim/envs/crowd_sim.py:117-169, 185-203) for a
// whole batch of (phase, case) seeds in one launch, consuming the legacy numpy stream exactly like sim.generate_scene does on the
// host (tests/scenegen_cpu.py is the plain-integer restatement this file is written from).
//
// Mapping: one case per wave, one workgroup of 64 lanes per case, and the 64 lanes are 64 successive ATTEMPTS of the human being
// placed.  An attempt consumes a fixed number of doubles (circle: angle and two noise terms; square: px, py or gx, gy), so attempt
// i of a round reads the stream at a known offset whether or not the attempts before it fail: every lane tempers its own words,
// evaluates its own candidate (float64 sin / cos) and tests it against the agents placed so far; the
// first accepting lane wins and the stream position moves past exactly the attempts up to it -- the accept / reject decisions and
// the draw count of the sequential loop.  A 19-human circle needs thousands of attempts per case, which one-candidate-per-wave
// (placed agents over the lanes) would evaluate one at a time with at most 20 of 64 lanes busy; a 5-human scene accepts in the
// first round either way.  The 624-word MT19937 state and the placed agents (5 doubles each) live in LDS, 7.6 KB per case.
//
// The stream is integer arithmetic plus exact double operations, so it equals numpy's bit for bit; the clearance tests must ROUND
// like numpy's `sqrt(dx * dx + dy * dy) < radius + radius_j + discomfort_dist`: no contraction into fused multiply-adds anywhere in
// this file (hipcc's default is -ffp-contract=fast, see rgl_train.hip), correctly rounded sqrt.
//
// Bounded: a human that has not been placed after cfg.max_attempts attempts ends its case with status 1 (upstream's loop has no
// exit; with randomize_attributes on a crowded circle it may never find room).
#include "rgl_common.h"
#include "rgl_mt19937.h"
#include "rgl_scene_place.h"      // SceneLds, Stream, draw, closer_than, place<>

namespace {

__global__ __launch_bounds__(kWave) void crowd_generate_scenes_kernel(const CrowdSceneConfig cfg, const unsigned* __restrict__ seeds,
                                                                      int H, double* __restrict__ robot, double* __restrict__ humans,
                                                                      double* __restrict__ goals, double* __restrict__ vpref,
                                                                      int* __restrict__ status, int* __restrict__ draws) {
#pragma clang fp contract(off)
    __shared__ SceneLds s;
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    mt_seed(s.mt, seeds[b], lane);
    Stream st{kMtN, 0};
    const double R = cfg.circle_radius;
    if (lane == 0) {
        const double row[9] = {0.0, -R, 0.0, 0.0, cfg.robot_radius, 0.0, R, cfg.robot_v_pref, 3.141592653589793 / 2};
        for (int c = 0; c < 9; ++c) robot[b * 9 + c] = row[c];
        s.px[0] = 0.0, s.py[0] = -R, s.gx[0] = 0.0, s.gy[0] = R, s.rad[0] = cfg.robot_radius;
    }
    __syncthreads();
    int flagged = 0;
    for (int i = 0; i < H && !flagged; ++i) {
        const int n = i + 1;                             // agents placed so far, the robot first
        Human h{cfg.human_v_pref, cfg.human_radius, 1.0, 0.0, 0.0, 0};
        if (cfg.randomize_attributes) redraw_attributes(s, st, h, lane);
        double px, py, gx, gy;
        if (cfg.scenario == CROWD_SCENARIO_CIRCLE_CROSSING) {
            if (!place<PLACE_CIRCLE>(cfg, s, st, h, n, lane)) { flagged = 1; break; }
            px = h.x, py = h.y, gx = -px, gy = -py;
        } else {
            h.sign = draw(s, st, lane) > 0.5 ? -1.0 : 1.0;
            if (!place<PLACE_SQUARE_POSITION>(cfg, s, st, h, n, lane)) { flagged = 1; break; }
            px = h.x, py = h.y;
            if (!place<PLACE_SQUARE_GOAL>(cfg, s, st, h, n, lane)) { flagged = 1; break; }
            gx = h.x, gy = h.y;
        }
        if (lane == 0) {
            s.px[n] = px, s.py[n] = py, s.gx[n] = gx, s.gy[n] = gy, s.rad[n] = h.radius;
            double* hr = humans + (b * H + i) * 5;
            hr[0] = px, hr[1] = py, hr[2] = 0.0, hr[3] = 0.0, hr[4] = h.radius;
            goals[(b * H + i) * 2] = gx, goals[(b * H + i) * 2 + 1] = gy;
            vpref[b * H + i] = h.v_pref;
        }
        __syncthreads();
    }
    if (lane == 0) {
        status[b] = flagged;
        draws[b] = st.draws;
    }
}

}  // namespace

extern "C" int crowd_generate_scenes_f64(const CrowdSceneConfig* cfg, const unsigned* seeds, int B, int H, double* robot,
                                         double* humans, double* goals, double* vpref, int* status, int* draws,
                                         rgl_stream_t stream) {
    if (!cfg || !seeds || !robot || !humans || !goals || !vpref || !status || !draws) return RGL_ERR_NULL;
    if (B < 1 || H < 1 || H + 1 > RGL_MAX_NODES || cfg->max_attempts < 1) return RGL_ERR_BAD_SHAPE;
    if (cfg->scenario != CROWD_SCENARIO_CIRCLE_CROSSING && cfg->scenario != CROWD_SCENARIO_SQUARE_CROSSING) return RGL_ERR_BAD_MODE;
    hipLaunchKernelGGL(crowd_generate_scenes_kernel, dim3((unsigned)B), dim3(kWave), 0, (hipStream_t)stream, *cfg, seeds, H, robot,
                       humans, goals, vpref, status, draws);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}
