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

namespace {

struct SceneLds {
    unsigned mt[kMtN];
    double px[RGL_MAX_NODES], py[RGL_MAX_NODES], gx[RGL_MAX_NODES], gy[RGL_MAX_NODES], rad[RGL_MAX_NODES];
};

struct Stream {
    int pos;        // next word of mt[] (624: twist first); the same in every lane
    int draws;      // random_sample / uniform calls consumed
};

// one double for the whole wave (every lane gets the same value)
__device__ double draw(SceneLds& s, Stream& st, int lane) {
    unsigned w[2];
    for (int t = 0; t < 2; ++t) {
        if (st.pos == kMtN) {
            mt_twist(s.mt, lane);
            st.pos = 0;
        }
        w[t] = temper(s.mt[st.pos++]);
    }
    ++st.draws;
    return to_double(w[0], w[1]);
}

// numpy's `sqrt(dx * dx + dy * dy) < margin` with its roundings
__device__ __forceinline__ bool closer_than(double dx, double dy, double margin) {
#pragma clang fp contract(off)
    return sqrt(dx * dx + dy * dy) < margin;
}

enum { PLACE_CIRCLE = 0, PLACE_SQUARE_POSITION = 1, PLACE_SQUARE_GOAL = 2 };

struct Human {
    double v_pref, radius, sign;
    double x, y;        // the accepted candidate of the last place() call
    int attempts;
};

// One rejection loop of generate_human.  Returns false when the human's attempt budget ran out.
template <int KIND>
__device__ bool place(const CrowdSceneConfig& cfg, SceneLds& s, Stream& st, Human& h, int n, int lane) {
#pragma clang fp contract(off)
    constexpr int kDoubles = KIND == PLACE_CIRCLE ? 3 : 2;
    constexpr int kWords = 2 * kDoubles;
    for (;;) {
        if (h.attempts >= cfg.max_attempts) return false;
        if (st.pos == kMtN) {
            mt_twist(s.mt, lane);
            st.pos = 0;
        }
        const int left = cfg.max_attempts - h.attempts;
        const int whole = (kMtN - st.pos) / kWords;      // attempts that lie wholly in the current block of 624 words
        double u[kDoubles];
        int m;                                           // attempts of this round: lane i < m evaluates attempt i
        if (whole == 0) {                                // the next attempt straddles the twist: one attempt, drawn wave-wide
            for (int t = 0; t < kDoubles; ++t) u[t] = draw(s, st, lane);
            st.draws -= kDoubles;                        // counted below like every other attempt
            m = 1;
        } else {
            m = min(min(whole, left), kWave);
            if (lane < m) {
                const unsigned* w = s.mt + st.pos + kWords * lane;
                for (int t = 0; t < kDoubles; ++t) u[t] = to_double(temper(w[2 * t]), temper(w[2 * t + 1]));
            }
        }
        bool ok = false;
        double x = 0.0, y = 0.0;
        if (lane < m) {
            if (KIND == PLACE_CIRCLE) {
                const double angle = u[0] * 3.141592653589793 * 2;
                const double px_noise = (u[1] - 0.5) * h.v_pref;
                const double py_noise = (u[2] - 0.5) * h.v_pref;
                x = cfg.circle_radius * cos(angle) + px_noise;
                y = cfg.circle_radius * sin(angle) + py_noise;
            } else {
                const double sign = KIND == PLACE_SQUARE_POSITION ? h.sign : -h.sign;
                x = u[0] * cfg.square_width * 0.5 * sign;
                y = (u[1] - 0.5) * cfg.square_width;
            }
            ok = true;
            for (int j = 0; j < n; ++j) {                // LDS broadcast reads: every lane asks for agent j
                const double margin = h.radius + s.rad[j] + cfg.discomfort_dist;
                if (KIND != PLACE_SQUARE_GOAL) ok = ok && !closer_than(x - s.px[j], y - s.py[j], margin);
                if (KIND != PLACE_SQUARE_POSITION) ok = ok && !closer_than(x - s.gx[j], y - s.gy[j], margin);
            }
        }
        const unsigned long long accepted = __ballot(ok);
        const int used = accepted ? __ffsll(accepted) : m;      // attempts consumed: up to and including the first accepted
        h.attempts += used;
        st.draws += kDoubles * used;
        if (whole != 0) st.pos += kWords * used;
        if (accepted) {
            h.x = __shfl(x, used - 1, kWave);
            h.y = __shfl(y, used - 1, kWave);
            return true;
        }
    }
}

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
        if (cfg.randomize_attributes) {
            h.v_pref = 0.5 + (1.5 - 0.5) * draw(s, st, lane);
            h.radius = 0.3 + (0.5 - 0.3) * draw(s, st, lane);
        }
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
