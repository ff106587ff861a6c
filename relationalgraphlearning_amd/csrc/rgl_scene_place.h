// generate_human's rejection loops for one wave of 64 lanes (crowd_sim/envs/crowd_sim.py:117-169): the agents placed so far and the
// 624 MT19937 words in LDS, the wave-wide draw, numpy's clearance test and place<>(), whose 64 lanes are 64 successive attempts.
// Shared by the scene generator (rgl_scenegen.hip, which explains the mapping) and the nonstop step (rgl_nonstop.hip).
//
// The clearance tests must ROUND like numpy's `sqrt(dx * dx + dy * dy) < radius + radius_j + discomfort_dist`: no contraction into
// fused multiply-adds (hipcc's default is -ffp-contract=fast, see rgl_train.hip), correctly rounded sqrt.
#pragma once
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

// Human.sample_random_attributes (crowd_sim/envs/utils/agent.py:42-48): numpy's uniform(lo, hi) = lo + (hi - lo) * u, two roundings
__device__ void redraw_attributes(SceneLds& s, Stream& st, Human& h, int lane) {
#pragma clang fp contract(off)
    h.v_pref = 0.5 + (1.5 - 0.5) * draw(s, st, lane);
    h.radius = 0.3 + (0.5 - 0.3) * draw(s, st, lane);
}

// One rejection loop of generate_human against agents 0 .. n - 1 of `s`.  Returns false when the human's attempt budget ran out.
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

}  // namespace
