// Epsilon-greedy exploration on device with every training case's own numpy stream (include/rgl_hip.h has the contract).
//
// Upstream seeds numpy once per case (CrowdSim.reset, crowd_sim/envs/crowd_sim.py:185-191), lets generate_human consume doubles
// and then continues the SAME stream in every predict of the episode: `probability = np.random.random()` and, when
// `probability < epsilon`, `np.random.choice(len(action_space))` (crowd_nav/policy/model_predictive_rl.py:208-210,
// multi_human_rl.py:34-36).  With ORCA or linear humans and sim.nonstop_human off nothing else draws.  With nonstop humans the
// step regenerates arriving humans from the same stream (rgl_nonstop.hip) and `state` is then the simulator's own, shared by both
// consumers.  Either way an exploring episode of case k is a function of k, epsilon and the weights.  These kernels carry that stream per environment: `state[b]` is the 624 MT19937 words plus the
// position of the next word (624: twist first), as the scene generator's Stream::pos.
//
// One decision of a live environment: u = random_sample() (two words); explored = u < epsilon (strict, float64); if explored and
// n_actions > 1, numpy's legacy masked rejection on 32-bit draws: mask = smallest 2^k - 1 >= n - 1, one word at a time,
// v = word & mask until v <= n - 1 (n = 1: index 0, nothing drawn).  A finished environment draws nothing: upstream no longer
// calls predict for it.  Upstream's reach_destination early return (no draw) is NOT implemented: it cannot occur for a live
// environment of a seeded scene -- step ends an episode whose next position is within the robot's radius of the goal, and start
// and goal are 2R apart -- so every decision of a live environment draws.
//
// Mapping: one environment per wave, one workgroup of 64 lanes each (the twist's barriers are the workgroup's).  The draw is
// sequential and wave-uniform; words are read straight from global memory, and only when the position reaches 624 are the words
// brought into LDS (2.5 KB), twisted cooperatively and written back -- a decision takes 2 words plus about 1.6 when it explores,
// so an episode meets a couple of twists at most.  Integer arithmetic plus to_double's exact operations: bit for bit numpy's.
#include "rgl_common.h"
#include "rgl_mt19937.h"

#include <cmath>

namespace {

constexpr int kStateWords = CROWD_EXPLORE_STATE_WORDS;
static_assert(kStateWords == kMtN + 1, "state = 624 words and the position");

__global__ __launch_bounds__(kWave) void crowd_explore_seed_kernel(const unsigned* __restrict__ seeds, const int* __restrict__ draws,
                                                                   unsigned* __restrict__ state) {
    __shared__ unsigned mt[kMtN];
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    mt_seed(mt, seeds[b], lane);
    const int d = draws[b];
    const long long words = d > 0 ? 2ll * d : 0;                 // 32-bit outputs the scene took
    const long long twists = (words + kMtN - 1) / kMtN;
    for (long long t = 0; t < twists; ++t) mt_twist(mt, lane);
    unsigned* out = state + b * kStateWords;
    for (int k = lane; k < kMtN; k += kWave) out[k] = mt[k];
    if (lane == 0) out[kMtN] = (unsigned)(twists ? words - kMtN * (twists - 1) : kMtN);
}

// the wave's view of one environment's stream: global words until the first twist of this launch, LDS afterwards
struct ExploreStream {
    unsigned* global;       // state[b]
    unsigned* lds;          // 624 words
    int pos;
    bool in_lds;
};

__device__ unsigned next_u32(ExploreStream& st, int lane) {
    if (st.pos == kMtN) {
        if (!st.in_lds) {
            for (int k = lane; k < kMtN; k += kWave) st.lds[k] = st.global[k];
            __syncthreads();
            st.in_lds = true;
        }
        mt_twist(st.lds, lane);
        st.pos = 0;
    }
    const unsigned y = st.in_lds ? st.lds[st.pos] : st.global[st.pos];
    ++st.pos;
    return (unsigned)__builtin_amdgcn_readfirstlane((int)temper(y));      // the same in every lane: keep it scalar
}

__global__ __launch_bounds__(kWave) void crowd_explore_select_kernel(const int* __restrict__ greedy, const int* __restrict__ done,
                                                                     const double* __restrict__ table, unsigned* state,
                                                                     int* __restrict__ chosen, double* __restrict__ action,
                                                                     int* __restrict__ explored, double epsilon, int n_actions) {
    __shared__ unsigned mt[kMtN];
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    int pick = __builtin_amdgcn_readfirstlane(greedy[b]);
    int took = 0;
    if (__builtin_amdgcn_readfirstlane(done[b]) == 0) {          // wave-uniform: the barriers below are met by every lane
        ExploreStream st{state + b * kStateWords, mt, 0, false};
        st.pos = __builtin_amdgcn_readfirstlane((int)st.global[kMtN]);
        if (st.pos < 0 || st.pos > kMtN) st.pos = kMtN;          // never index past the words, whatever the caller left there
        const unsigned w0 = next_u32(st, lane);
        const unsigned w1 = next_u32(st, lane);
        took = to_double(w0, w1) < epsilon ? 1 : 0;
        if (took) {
            pick = 0;
            if (n_actions > 1) {
                unsigned mask = (unsigned)(n_actions - 1);
                mask |= mask >> 1, mask |= mask >> 2, mask |= mask >> 4, mask |= mask >> 8, mask |= mask >> 16;
                unsigned v;
                do {
                    v = next_u32(st, lane) & mask;
                } while (v > (unsigned)(n_actions - 1));
                pick = (int)v;
            }
        }
        if (st.in_lds) {
            __syncthreads();
            for (int k = lane; k < kMtN; k += kWave) st.global[k] = st.lds[k];
        }
        if (lane == 0) st.global[kMtN] = (unsigned)st.pos;
    }
    const bool in_range = pick >= 0 && pick < n_actions;
    if (lane < 2) action[b * 2 + lane] = in_range ? table[(long long)pick * 2 + lane] : (double)NAN;
    if (lane == 0) {
        chosen[b] = pick;
        if (explored) explored[b] = took;
    }
}

}  // namespace

extern "C" int crowd_explore_seed_u32(const unsigned* seeds, const int* draws, int B, unsigned* state, rgl_stream_t stream) {
    if (!seeds || !draws || !state) return RGL_ERR_NULL;
    if (B < 1) return RGL_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(crowd_explore_seed_kernel, dim3((unsigned)B), dim3(kWave), 0, (hipStream_t)stream, seeds, draws, state);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

extern "C" int crowd_explore_select_f64(const CrowdExploreJob* job) {
    if (!job || !job->greedy || !job->done || !job->table || !job->state || !job->chosen || !job->action) return RGL_ERR_NULL;
    if (job->B < 1 || job->n_actions < 1 || job->n_actions > RGL_MAX_ACTIONS) return RGL_ERR_BAD_SHAPE;
    if (!(job->epsilon >= 0.0 && job->epsilon <= 1.0)) return RGL_ERR_BAD_MODE;       // NaN fails both comparisons
    hipLaunchKernelGGL(crowd_explore_select_kernel, dim3((unsigned)job->B), dim3(kWave), 0, (hipStream_t)job->stream, job->greedy,
                       job->done, job->table, job->state, job->chosen, job->action, job->explored, job->epsilon, job->n_actions);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}
