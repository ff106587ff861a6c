// rgl_replay.hip -- the replay memory filled on device: what VectorExplorer.update_memory pushes tuple by tuple (crowd_nav/utils/
// explorer.py:113-140 through crowd_nav/utils/memory.py) for a whole batch of finished episodes, in three launches.
//
// The episodes arrive as the explorer recorded them: robot [T][B][9], humans [T][B][H][5], rewards [T][B], info [T][B] (CROWD_INFO_*;
// 5 = the episode had finished earlier).  Episode b has L_b live steps (a prefix of its column); it is stored when its last end code
// is a collision or a reached goal, and then contributes the L_b - 1 tuples (state i, value i, reward i, state i + 1).  Tuples are
// numbered episode-major, j = offset[b] + i, in the order the host path pushes them; where tuple j goes is the caller's slot map
// (RglReplayRun: the ring arithmetic of ReplayMemory.push for a whole call, trimmed on the host so that no slot is named twice).
//
//   1. replay_episodes_kernel   a thread per episode: L_b, the stored flag, the tuple count, and -- imitation learning -- the
//                               returns-to-go of its steps in float64, product and sum rounded on their own like the host's python
//                               floats, cast to float32 into the workspace
//   2. replay_offsets_kernel    one workgroup: exclusive prefix sum of the tuple counts (any B: 256 episodes a pass, a carry between)
//   3. replay_scatter_kernel    a wave per recorded state (t, b): the state's floats (MPRL: the robot row and the humans; path G: the H
//                               rotated rows, staged in LDS) go to tuple t's state fields and to tuple t - 1's next-state fields, lanes
//                               on consecutive floats of both; lane 0 adds tuple t's value and reward
//
//      replay_sarl_scatter_kernel  the third launch of rgl_replay_push_sarl_f32: a workgroup per recorded state builds the (H, D) rows
//                               SARL.transform makes of it -- the 13 rotated features and, with maps, the cell_num^2 channels
//                               occupancy-map slots of each human (rgl_sarl_maps.h: sarl_maps_kernel's arithmetic from the float32
//                               states widened to float64, dt = 0) -- and stores them the same way
//
// The SARL kernel's LDS.  A state's humans i are walked in groups of G = min(H, kSarlPairRecords / H) humans, kSarlPairRecords =
// 1 024: a group holds the G H pair records (cell, vx, vy: 20 bytes each, at most 20 480 bytes), its G own angles (at most 256
// bytes) and its G staged rows of D floats (G <= 32, D <= 13 + 8 * 8 * 3 = 205: at most 26 240 bytes), 46 976 bytes at the
// most and 1 760 bytes at H = 5, D = 61.  The size is the launch's dynamic LDS, so that small crowds are not charged for large
// ones.  Up to kSarlOneWaveHumans = 32 humans -- one group -- a workgroup is one wave: such states are many and small, and a wave
// per state keeps every wave of a CU on float64 pairs instead of waiting at a barrier.  Above, four waves share a state's groups:
// the threads walk the G H pairs of a group flattened (any H, 256 pairs a pass), then the G n_slots slots, then the G D floats.
//
// Every slot element is stored by exactly one thread of one launch: a surviving tuple's state fields by the wave of (t, b), its
// next-state fields by the wave of (t + 1, b), and no two surviving tuples share a slot.  Nothing of a step t >= L_b is read.
#include "rgl_rotate.h"
#include "rgl_sarl_maps.h"

#include <climits>

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kRowFloats = 13;                       // a rotated row

struct ReplayWorkspace {
    int* counts;        // [B] tuples of episode b (0: not stored)
    int* offsets;       // [B + 1] first tuple of episode b; [B] = N
    float* values;      // [T][B] value of tuple (t, b), imitation learning only
    size_t bytes;
};

inline ReplayWorkspace carve(void* base, int T, int B) {
    Carver c{(char*)base, 0};
    ReplayWorkspace w;
    w.counts = c.take<int>((long long)B * sizeof(int));
    w.offsets = c.take<int>(((long long)B + 1) * sizeof(int));
    w.values = c.take<float>((long long)T * B * sizeof(float));
    w.bytes = (size_t)c.off;
    return w;
}

__global__ void replay_episodes_kernel(const int* __restrict__ info, const float* __restrict__ rewards, int T, int B,
                                       int imitation_learning, double step_discount, int* __restrict__ counts,
                                       float* __restrict__ values) {
    // togo[t] = r[t] + d * togo[t + 1] as update_memory computes it with python floats: two roundings per step
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int L = 0, outcome = 0;
    for (int t = 0; t < T; ++t) {
        const int code = info[(size_t)t * B + b];
        if (code != CROWD_INFO_DONE) ++L;
        if (code >= CROWD_INFO_COLLISION && code <= CROWD_INFO_TIMEOUT) outcome = code;
    }
    const bool stored = outcome == CROWD_INFO_COLLISION || outcome == CROWD_INFO_REACH_GOAL;
    const int n = stored && L > 1 ? L - 1 : 0;
    counts[b] = n;
    if (!imitation_learning || n == 0) return;
    double togo = 0.0;
    for (int t = L - 1; t >= 0; --t) {
        const double product = step_discount * togo;
        togo = (double)rewards[(size_t)t * B + b] + product;
        if (t < n) values[(size_t)t * B + b] = (float)togo;          // round to nearest, as torch.tensor([togo], dtype=float32)
    }
}

__global__ __launch_bounds__(kBlock) void replay_offsets_kernel(const int* __restrict__ counts, int B, int* __restrict__ offsets) {
    __shared__ int wave_total[kBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int carry = 0;
    for (int base = 0; base < B; base += kBlock) {
        const int b = base + threadIdx.x;
        const int mine = b < B ? counts[b] : 0;
        int incl = mine;
        for (int d = 1; d < kWave; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == kWave - 1) wave_total[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kBlock / kWave; ++w) {
            if (w < wave) before += wave_total[w];
            total += wave_total[w];
        }
        if (b < B) offsets[b] = carry + before + incl - mine;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[B] = carry;
}

struct ScatterArgs {
    const float* robot;
    const float* humans;
    const float* rewards;
    const float* values;
    const int* counts;
    const int* offsets;
    float* fields[RGL_REPLAY_MAX_FIELDS];
    RglReplayRun runs[RGL_REPLAY_MAX_RUNS];
    long long states;      // T * B
    int B, H, n_runs, gcn, unicycle, imitation_learning;
};

// where tuple j of the call goes, or -1: overwritten later in the same call (or past what the caller's map covers)
__device__ __forceinline__ long long slot_of(const ScatterArgs& a, long long j) {
    long long slot = -1;
    for (int r = 0; r < a.n_runs; ++r) {
        const long long k = j - a.runs[r].first;
        if (k >= 0 && k < a.runs[r].count) slot = a.runs[r].slot + k;
    }
    return slot;
}

__global__ __launch_bounds__(kWave) void replay_scatter_kernel(const ScatterArgs a) {
    __shared__ float rotated[(RGL_MAX_NODES - 1) * kRowFloats];
    const int lane = threadIdx.x;
    const int H = a.H;
    for (long long s = blockIdx.x; s < a.states; s += gridDim.x) {          // s = t * B + b, uniform over the wave
        const int b = (int)(s % a.B);
        const long long t = s / a.B;
        const int n = a.counts[b];
        if (n == 0 || t > n) continue;                                       // states 0..n of a stored episode make its n tuples
        const long long j = (long long)a.offsets[b] + t;
        const long long cur = t < n ? slot_of(a, j) : -1;                    // tuple t: this is its state
        const long long prev = t > 0 ? slot_of(a, j - 1) : -1;               // tuple t - 1: this is its next state
        if (cur < 0 && prev < 0) continue;
        if (a.gcn) {
            for (int h = lane; h < H; h += kWave) {
                float joint[14], o[kRowFloats];
#pragma unroll
                for (int k = 0; k < 9; ++k) joint[k] = a.robot[s * 9 + k];
#pragma unroll
                for (int k = 0; k < 5; ++k) joint[9 + k] = a.humans[(s * H + h) * 5 + k];
                rotate_row(joint, a.unicycle, o);
#pragma unroll
                for (int k = 0; k < kRowFloats; ++k) rotated[h * kRowFloats + k] = o[k];
            }
            __syncthreads();
            const int row = H * kRowFloats;
            for (int k = lane; k < row; k += kWave) {
                const float v = rotated[k];
                if (cur >= 0) a.fields[0][cur * row + k] = v;
                if (prev >= 0) a.fields[3][prev * row + k] = v;
            }
            __syncthreads();
            if (lane == 0 && cur >= 0) {
                a.fields[1][cur] = a.imitation_learning ? a.values[s] : 0.f;
                a.fields[2][cur] = a.rewards[s];
            }
        } else {
            const int row = H * 5;
            for (int k = lane; k < 9 + row; k += kWave) {
                if (k < 9) {
                    const float v = a.robot[s * 9 + k];
                    if (cur >= 0) a.fields[0][cur * 9 + k] = v;
                    if (prev >= 0) a.fields[4][prev * 9 + k] = v;
                } else {
                    const float v = a.humans[s * row + (k - 9)];
                    if (cur >= 0) a.fields[1][cur * row + (k - 9)] = v;
                    if (prev >= 0) a.fields[5][prev * row + (k - 9)] = v;
                }
            }
            if (lane == 0 && cur >= 0) {
                a.fields[2][cur] = a.imitation_learning ? a.values[s] : 0.f;
                a.fields[3][cur] = a.rewards[s];
            }
        }
    }
}

constexpr int kSarlPairRecords = 1024;               // pair records of one group of humans in LDS
constexpr int kSarlOneWaveHumans = 32;               // up to here a workgroup is one wave (and a state one group)

inline int sarl_group(int H) { return H < kSarlPairRecords / H ? H : kSarlPairRecords / H; }

struct SarlScatterArgs {
    ScatterArgs s;         // gcn unused
    int cell_num, channels, group;
    double cell_size;
};

inline size_t sarl_lds_bytes(int H, int D, int channels) {
    const size_t G = (size_t)sarl_group(H), P = channels ? G * H : 0;
    return P * (2 * sizeof(double) + sizeof(int)) + G * sizeof(double) + G * D * sizeof(float);
}

template <int WAVES>
__global__ __launch_bounds__(kWave * WAVES) void replay_sarl_scatter_kernel(const SarlScatterArgs sa) {
#pragma clang fp contract(off)
    extern __shared__ double sarl_lds[];
    const ScatterArgs& a = sa.s;
    constexpr int kThreads = kWave * WAVES;
    const int tid = threadIdx.x;
    const int H = a.H, G = sa.group, channels = sa.channels;
    const int n_slots = sa.cell_num * sa.cell_num * channels, D = kRowFloats + n_slots;
    const int P = channels ? G * H : 0;
    double* own_angle = sarl_lds;                              // [G]
    double* pair_vx = own_angle + G;                           // [G][H]
    double* pair_vy = pair_vx + P;
    int* pair_cell = (int*)(pair_vy + P);                      // -1: j == i, or j outside i's grid
    float* staged = (float*)(pair_cell + P);                   // [G][D]
    for (long long s = blockIdx.x; s < a.states; s += gridDim.x) {          // s = t * B + b, uniform over the workgroup
        const int b = (int)(s % a.B);
        const long long t = s / a.B;
        const int n = a.counts[b];
        if (n == 0 || t > n) continue;                                       // not stored, or beyond the episode: nothing computed
        const long long j0 = (long long)a.offsets[b] + t;
        const long long cur = t < n ? slot_of(a, j0) : -1;
        const long long prev = t > 0 ? slot_of(a, j0 - 1) : -1;
        if (cur < 0 && prev < 0) continue;                                   // neither tuple survives the call
        auto state = [&](int h, int k) { return (double)a.humans[(s * H + h) * 5 + k]; };
        const long long row = (long long)H * D;
        for (int i0 = 0; i0 < H; i0 += G) {
            const int g = H - i0 < G ? H - i0 : G;
            for (int r = tid; r < g; r += kThreads) {
                float joint[14], o[kRowFloats];
#pragma unroll
                for (int k = 0; k < 9; ++k) joint[k] = a.robot[s * 9 + k];
#pragma unroll
                for (int k = 0; k < 5; ++k) joint[9 + k] = a.humans[(s * H + i0 + r) * 5 + k];
                rotate_row(joint, a.unicycle, o);
#pragma unroll
                for (int k = 0; k < kRowFloats; ++k) staged[r * D + k] = o[k];
                if (channels) own_angle[r] = atan2(state(i0 + r, 3), state(i0 + r, 2));
            }
            if (channels) {
                __syncthreads();
                for (int p = tid; p < g * H; p += kThreads) {
                    const int r = p / H, j = p - r * H;
                    int cell;
                    double ovx, ovy;
                    sarl_map_pair(state, i0 + r, j, own_angle[r], 0.0, sa.cell_num, sa.cell_size, channels, cell, ovx, ovy);
                    pair_cell[p] = cell;
                    pair_vx[p] = ovx;
                    pair_vy[p] = ovy;
                }
                __syncthreads();
                for (int q = tid; q < g * n_slots; q += kThreads) {
                    const int r = q / n_slots, slot = q - r * n_slots;
                    staged[r * D + kRowFloats + slot] =
                        sarl_map_slot(pair_cell + r * H, pair_vx + r * H, pair_vy + r * H, H, slot, channels);
                }
            }
            __syncthreads();
            const long long at = (long long)i0 * D;
            for (int k = tid; k < g * D; k += kThreads) {
                const float v = staged[k];
                if (cur >= 0) a.fields[0][cur * row + at + k] = v;
                if (prev >= 0) a.fields[3][prev * row + at + k] = v;
            }
            __syncthreads();                                                 // the next group (or state) stages over these
        }
        if (tid == 0 && cur >= 0) {
            a.fields[1][cur] = a.imitation_learning ? a.values[s] : 0.f;
            a.fields[2][cur] = a.rewards[s];
        }
    }
}

// the checks of a push in their order; `rows` answers for what the layout asks of the job and gives its number of fields
template <class Rows>
inline int check_job(const RglReplayPushJob* job, const Rows& rows) {
    if (!job || !job->robot || !job->humans || !job->rewards || !job->info) return RGL_ERR_NULL;
    if (job->T < 1 || job->B < 1 || job->H < 1 || job->H + 1 > RGL_MAX_NODES || job->capacity < 1) return RGL_ERR_BAD_SHAPE;
    if ((long long)job->T * job->B > INT_MAX) return RGL_ERR_BAD_SHAPE;             // tuple indices of one call are 32-bit
    int n_fields = 0;
    const int rows_rc = rows(n_fields);
    if (rows_rc) return rows_rc;
    if (job->kinematics != RGL_HOLONOMIC && job->kinematics != RGL_UNICYCLE) return RGL_ERR_BAD_MODE;
    for (int f = 0; f < n_fields; ++f)
        if (!job->fields[f]) return RGL_ERR_NULL;
    // the slot map names slots of the memory only: whatever the device finds in `info`, no store leaves the fields
    if (job->n_runs < 0 || job->n_runs > RGL_REPLAY_MAX_RUNS) return RGL_ERR_BAD_SHAPE;
    for (int r = 0; r < job->n_runs; ++r) {
        const RglReplayRun& run = job->runs[r];
        if (run.first < 0 || run.slot < 0 || run.count < 0 || run.count > job->capacity || run.slot > job->capacity - run.count)
            return RGL_ERR_BAD_SHAPE;
    }
    return RGL_OK;
}

}  // namespace

extern "C" size_t rgl_replay_push_workspace_bytes(int T, int B) {
    if (T < 1 || B < 1 || (long long)T * B > INT_MAX) return 0;
    return carve(nullptr, T, B).bytes;
}

namespace {

// what both pushes do behind their checks: the workspace and the three launches.  `rows`: the SARL scatter with these maps; null:
// the scatter of the job's own layout
inline int push(const RglReplayPushJob* job, const RglReplaySarlRows* rows) {
    if (!job->workspace) return RGL_ERR_NULL;
    const int T = job->T, B = job->B;
    const ReplayWorkspace w = carve(job->workspace, T, B);
    if (job->workspace_bytes < w.bytes) return RGL_ERR_WORKSPACE;
    if (job->n_runs == 0) return RGL_OK;                                            // nothing of this call survives: no launch
    hipStream_t stream = (hipStream_t)job->stream;
    hipLaunchKernelGGL(replay_episodes_kernel, dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, job->info,
                       job->rewards, T, B, job->imitation_learning, job->step_discount, w.counts, w.values);
    RGL_LAUNCH_CHECK();
    hipLaunchKernelGGL(replay_offsets_kernel, dim3(1), dim3(kBlock), 0, stream, w.counts, B, w.offsets);
    RGL_LAUNCH_CHECK();
    SarlScatterArgs sa;
    ScatterArgs& a = sa.s;
    a.robot = job->robot, a.humans = job->humans, a.rewards = job->rewards, a.values = w.values;
    a.counts = w.counts, a.offsets = w.offsets;
    for (int f = 0; f < RGL_REPLAY_MAX_FIELDS; ++f) a.fields[f] = job->fields[f];
    for (int r = 0; r < RGL_REPLAY_MAX_RUNS; ++r) a.runs[r] = job->runs[r];
    a.states = (long long)T * B;
    a.B = B, a.H = job->H, a.n_runs = job->n_runs, a.gcn = job->layout == RGL_REPLAY_GCN;      // (the SARL scatter does not read gcn)
    a.unicycle = job->kinematics == RGL_UNICYCLE, a.imitation_learning = job->imitation_learning != 0;
    const dim3 grid((unsigned)(a.states < 65536 ? a.states : 65536));
    if (!rows) {
        hipLaunchKernelGGL(replay_scatter_kernel, grid, dim3(kWave), 0, stream, a);
    } else {
        sa.cell_num = rows->channels ? rows->cell_num : 0, sa.channels = rows->channels, sa.cell_size = rows->cell_size;
        sa.group = sarl_group(a.H);
        const size_t lds = sarl_lds_bytes(a.H, kRowFloats + sa.cell_num * sa.cell_num * sa.channels, sa.channels);
        if (a.H <= kSarlOneWaveHumans)
            hipLaunchKernelGGL(replay_sarl_scatter_kernel<1>, grid, dim3(kWave), lds, stream, sa);
        else
            hipLaunchKernelGGL(replay_sarl_scatter_kernel<4>, grid, dim3(4 * kWave), lds, stream, sa);
    }
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

}  // namespace

extern "C" int rgl_replay_push_f32(const RglReplayPushJob* job) {
    const int rc = check_job(job, [&](int& n_fields) {
        if (job->layout != RGL_REPLAY_MPRL && job->layout != RGL_REPLAY_GCN) return RGL_ERR_BAD_MODE;
        n_fields = job->layout == RGL_REPLAY_MPRL ? 6 : 4;
        return RGL_OK;
    });
    if (rc) return rc;
    return push(job, nullptr);
}

extern "C" int rgl_replay_push_sarl_f32(const RglReplayPushJob* job, const RglReplaySarlRows* rows) {
    if (!rows) return RGL_ERR_NULL;
    const int rc = check_job(job, [&](int& n_fields) {
        n_fields = 4;
        if (rows->channels == 0) return RGL_OK;                                     // no maps: the 13 rotated features alone
        const int maps_rc = sarl_map_params_rc(rows->cell_num, rows->cell_size, rows->channels);
        if (maps_rc) return maps_rc;
        return job->H < 2 ? RGL_ERR_BAD_SHAPE : RGL_OK;                             // maps of a single human: no other humans
    });
    if (rc) return rc;
    return push(job, rows);
}
