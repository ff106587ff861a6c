// rgl_sarl.hip -- SARL / OM-SARL evaluation: the occupancy maps of MultiHumanRL.build_occupancy_maps
// (crowd_nav/policy/multi_human_rl.py:117-171), the attention value network of crowd_nav/policy/sarl.py:28-73 and the one-step
// search of multi_human_rl.py:36-64 around them.  The search's first and last steps (prepare, select) are the ones path G runs: rgl_onestep.h.
//
// The value network is one f32 MFMA launch over all scenes.  A wave owns sixteen scenes; MFMA tile h holds human h of those sixteen
// scenes as the B operand (column n = scene n), the weights are the A operand.  A 16 x 16 x 4 product leaves output feature
// 16 mt + 4 g + i of scene n in register i of lane (g, n) (g = lane / 16, n = lane % 16).  The next layer takes the four k of its
// k-step (t, i) from exactly those registers -- k-step (t, i) multiplies the input features {16 t + 4 g + i : g = 0..3} -- so an
// activation never leaves the lane that computed it, and the mean over humans, the softmax over humans and the weighted sum are
// element-wise over the wave's own tiles.  The A fragments of that k order are laid out once per call by sarl_pack_kernel
// ([t][mt][lane][i]: one 16-byte load per lane serves four MFMAs) and read from L2: the four MLPs hold 415 KB, more than a CU's LDS.
// The LDS parks the per-human mlp1 outputs of a tile's scenes (they are read twice: by the mean, and by mlp2 / attention once the
// mean is known), later overwritten by the mlp2 outputs and the attention score of the same human: 7 424 bytes per human, which a
// CU's LDS holds for up to kSarlLdsHumans humans.  Above that the same slots live in a region of the workspace per workgroup (the
// kernel's SarlValueGlobalArgs form); what bounds H is then gcn_prepare_f32's H + 1 <= RGL_MAX_NODES (RGL_SARL_MAX_HUMANS).  A
// workgroup is one wave below kSarlWideFrom humans and four waves sharing one tile above.
#include "rgl_mfma.h"
#include "rgl_onestep.h"
#include "rgl_sarl_maps.h"
#include "rgl_sarl_shapes.h"

namespace {

constexpr int kSarlLayers = 11;         // mlp1.{0,2} mlp2.{0,2} attention.{0,2,4} mlp3.{0,2,4,6}
constexpr int kT150 = 10, kT100 = 7, kT50 = 4;      // 16-feature tiles of the shipped widths
constexpr int kParkRegs = 4 * kT100 + 1;            // a human's slot: 28 registers of the wave + its attention score
constexpr int kParkFloats = kParkRegs * 64;

struct SarlPackJob {
    const float* src;           // k-major [K][M]
    const float* bias;          // [M]
    long long dst;              // float offset of the packed layer: [KT][MT][64][4] fragments, then [MT][16] bias
    int K, M, KT, MT;
    int split_tile, split_cols; // k-tiles below split_tile read columns [0, split_cols) from their first feature on, the tiles from
                                // split_tile on read columns split_cols.. (the concatenations: mean behind mlp1's rows, the
                                // weighted feature behind the six self features)
};
struct SarlPackArgs {
    SarlPackJob job[kSarlLayers];
    float* out;
};

__global__ void sarl_pack_kernel(const SarlPackArgs pa) {
    const SarlPackJob& j = pa.job[blockIdx.y];
    const long long n_frag = (long long)j.MT * j.KT * 256, total = n_frag + j.MT * 16;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (e < n_frag) {
            const int i = (int)(e & 3), lane = (int)((e >> 2) & 63);
            const int tt = (int)(e >> 8), mt = tt % j.MT, t = tt / j.MT;
            const int g = lane >> 4, m = lane & 15;
            const int kidx = 16 * t + 4 * g + i, row = 16 * mt + m;
            int col;
            bool ok;
            if (t < j.split_tile) {
                col = kidx;
                ok = col < j.split_cols;
            } else {
                col = j.split_cols + kidx - 16 * j.split_tile;
                ok = col < j.K;
            }
            if (ok && row < j.M) v = j.src[(size_t)col * j.M + row];
        } else {
            const int row = (int)(e - n_frag);
            if (row < j.M) v = j.bias[row];
        }
        pa.out[j.dst + e] = v;
    }
}

// out = W in + b over one 16-scene tile: KT input tiles, MT output tiles, every output tile an accumulator of its own (MT independent
// MFMA chains in flight per k-step)
template <int KT, int MT, bool RELU>
__device__ __forceinline__ void sarl_layer(const f32x4 (&in)[KT], f32x4 (&out)[MT], const float* __restrict__ wp, unsigned lane) {
    // the layer's base stays a scalar the compiler cannot see through: the hundreds of fragment addresses of a pass over the network
    // are loop invariants, and hoisted out of the tile loop they spill; as scalar base + lane offset + immediate they cost nothing
    const char* w = reinterpret_cast<const char*>(wp);
    asm volatile("" : "+s"(w));
    const unsigned lane_off = lane * 16u, bias_off = (lane >> 4) * 16u;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) out[mt] = *reinterpret_cast<const f32x4*>(w + (size_t)(MT * KT * 1024 + 64 * mt) + bias_off);
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        f32x4 a[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4*>(w + (size_t)((t * MT + mt) * 1024) + lane_off);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) out[mt] = mfma4(a[mt][i], in[t][i], out[mt]);
        load_fence();
    }
    if (RELU) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) out[mt][i] = fmaxf(out[mt][i], 0.f);
    }
}

// float offset of packed layer l: a function of the two template parameters of the value kernel alone
constexpr int sarl_layer_offset(int kt0, bool global, int l) {
    const int KT[kSarlLayers] = {kt0, kT150, kT100, kT100, global ? 2 * kT100 : kT100, kT100, kT100, 1 + kT50, kT150, kT100, kT100};
    const int MT[kSarlLayers] = {kT150, kT100, kT100, kT50, kT100, kT100, 1, kT150, kT100, kT100, 1};
    int off = 0;
    for (int i = 0; i < l; ++i) off += MT[i] * KT[i] * 256 + MT[i] * 16;
    return off;
}

struct SarlValueArgs {
    const float* packed;
    const float* rows;          // [S][H][D], or null: the three arrays below
    const float* self6;         // [S][6]
    const float* hum7;          // [S][H][7]
    const float* maps;          // [S / scenes_per_root][H][D - 13]; unread when D == 13
    float* value;               // [S]
    float* attention;           // [S][H]
    int S, H, D, scenes_per_root, n_tiles;
};
struct SarlValueGlobalArgs : SarlValueArgs {
    float* park;                // the parking slots of the global form: [grid][H][kParkRegs][64]
};

// The barrier between a tile's passes over its parking slots.  The slots of the global form are written and read with plain vector
// stores and loads by waves of ONE workgroup, hence through one CU's L1 and in the order the barrier sets; every wave drains its own
// stores (and the loads a later store to the same slot must not overtake) before it arrives.
template <bool GPARK>
__device__ __forceinline__ void sarl_park_barrier() {
    if constexpr (GPARK) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// KT0: 16-feature tiles of a row (input_dim 13 | 29 | 45 | 61); GLOBAL: with_global_state; WAVES: waves of the workgroup, which
// all work on the same sixteen scenes -- wave w takes the humans h = w, w + WAVES, .. through mlp1 and through mlp2 / attention, and
// the waves take turns with a tile's softmax, weighted sum and mlp3.  One wave per workgroup while four such workgroups' parking
// space fits a CU; at larger H a one-wave workgroup would leave SIMDs idle behind its LDS.
// ARGS = SarlValueGlobalArgs: the form for more humans than a CU's LDS parks (and for any H under RGL_SARL_PARK=global).  `park` is
// then the workgroup's own region of the workspace instead of its LDS -- the same slots at the same offsets, the same passes and
// barriers, hence the same bits.  No other workgroup touches the region, and a workgroup reads no slot it has not written for the
// tile at hand.
template <int KT0, bool GLOBAL, int WAVES, class ARGS = SarlValueArgs>
__global__ __launch_bounds__(64 * WAVES) void sarl_value_kernel(const ARGS va) {
    constexpr bool GPARK = std::is_same<ARGS, SarlValueGlobalArgs>::value;
    extern __shared__ float park_lds[];
    float* park;                            // [H][kParkRegs][64]
    if constexpr (GPARK) park = va.park + (size_t)blockIdx.x * ((size_t)va.H * kParkFloats);
    else park = park_lds;
    const int wave = threadIdx.x >> 6;
    const unsigned lane = threadIdx.x & 63;
    const int g = lane >> 4, n = lane & 15;
    const int H = va.H, D = va.D;
    auto W = [&](auto l) { return va.packed + sarl_layer_offset(KT0, GLOBAL, decltype(l)::value); };

    int turn = 0;
    for (int tile = blockIdx.x; tile < va.n_tiles; tile += gridDim.x, ++turn) {
        const int s = tile * 16 + n;
        const bool live = s < va.S;
        const size_t sc = (size_t)(live ? s : va.S - 1);       // the partial last tile computes its last scene again, writes nothing
        const size_t root = sc / (size_t)va.scenes_per_root;

        // ---- mlp1 per human; its outputs parked ----
        for (int h = wave; h < H; h += WAVES) {
            f32x4 x[KT0];
#pragma unroll
            for (int t = 0; t < KT0; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int f = 16 * t + 4 * g + i;
                    float v = 0.f;
                    if (va.rows) {
                        if (f < D) v = va.rows[(sc * H + h) * D + f];
                    } else if (f < 6) {
                        v = va.self6[sc * 6 + f];
                    } else if (f < 13) {
                        v = va.hum7[(sc * H + h) * 7 + (f - 6)];
                    } else if (f < D) {
                        v = va.maps[(root * H + h) * (size_t)(D - 13) + (f - 13)];
                    }
                    x[t][i] = v;
                }
            f32x4 h1[kT150], y[kT100];
            sarl_layer<KT0, kT150, true>(x, h1, W(std::integral_constant<int, 0>{}), lane);
            sarl_layer<kT150, kT100, true>(h1, y, W(std::integral_constant<int, 1>{}), lane);
            float* slot = park + (size_t)h * kParkFloats + lane;
#pragma unroll
            for (int r = 0; r < kT100; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) slot[(4 * r + i) * 64] = y[r][i];
        }
        sarl_park_barrier<GPARK>();
        f32x4 mean[kT100];
        if constexpr (GLOBAL) {     // torch.mean over the humans: the sum in human order, divided
#pragma unroll
            for (int r = 0; r < kT100; ++r) mean[r] = zero4();
            for (int h = 0; h < H; ++h) {
                const float* slot = park + (size_t)h * kParkFloats + lane;
#pragma unroll
                for (int r = 0; r < kT100; ++r)
#pragma unroll
                    for (int i = 0; i < 4; ++i) mean[r][i] += slot[(4 * r + i) * 64];
            }
            const float fh = (float)H;
#pragma unroll
            for (int r = 0; r < kT100; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) mean[r][i] = mean[r][i] / fh;
            if (WAVES > 1) sarl_park_barrier<GPARK>();     // every wave has read every slot before any slot changes its content
        }

        // ---- mlp2 and the attention score per human; the slot now keeps the mlp2 output and the score ----
        for (int h = wave; h < H; h += WAVES) {
            float* slot = park + (size_t)h * kParkFloats + lane;
            constexpr int KA = GLOBAL ? 2 * kT100 : kT100;
            f32x4 ain[KA];
#pragma unroll
            for (int r = 0; r < kT100; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) ain[r][i] = slot[(4 * r + i) * 64];
            if constexpr (GLOBAL) {
#pragma unroll
                for (int r = 0; r < kT100; ++r) ain[kT100 + r] = mean[r];
            }
            {
                f32x4 a1[kT100], a2[kT100], sco[1];
                sarl_layer<KA, kT100, true>(ain, a1, W(std::integral_constant<int, 4>{}), lane);
                sarl_layer<kT100, kT100, true>(a1, a2, W(std::integral_constant<int, 5>{}), lane);
                sarl_layer<kT100, 1, false>(a2, sco, W(std::integral_constant<int, 6>{}), lane);
                if (g == 0) park[(size_t)h * kParkFloats + 4 * kT100 * 64 + n] = sco[0][0];      // output feature 0 of scene n
            }
            {
                f32x4 yin[kT100], m1[kT100], feat[kT50];
#pragma unroll
                for (int r = 0; r < kT100; ++r) yin[r] = ain[r];
                sarl_layer<kT100, kT100, true>(yin, m1, W(std::integral_constant<int, 2>{}), lane);
                sarl_layer<kT100, kT50, false>(m1, feat, W(std::integral_constant<int, 3>{}), lane);
#pragma unroll
                for (int r = 0; r < kT50; ++r)
#pragma unroll
                    for (int i = 0; i < 4; ++i) slot[(4 * r + i) * 64] = feat[r][i];
            }
        }
        sarl_park_barrier<GPARK>();        // scores and mlp2 outputs of every human are in place (one wave: lanes 0..15 wrote the scores)

        // ---- softmax over the humans (sarl.py:57-63 with an all-ones mask), weighted sum of the mlp2 outputs: one wave's turn ----
        const bool mine = wave == turn % WAVES;
        f32x4 joint[1 + kT50];
        if (mine) {
            float smax = -INFINITY;
            for (int h = 0; h < H; ++h) smax = fmaxf(smax, park[(size_t)h * kParkFloats + 4 * kT100 * 64 + n]);
            float ssum = 0.f;
            for (int h = 0; h < H; ++h) ssum = f32_add(ssum, expf(f32_sub(park[(size_t)h * kParkFloats + 4 * kT100 * 64 + n], smax)));
#pragma unroll
            for (int r = 0; r <= kT50; ++r) joint[r] = zero4();
            for (int h = 0; h < H; ++h) {
                const float w = f32_div(expf(f32_sub(park[(size_t)h * kParkFloats + 4 * kT100 * 64 + n], smax)), ssum);
                if (live && g == 0) va.attention[sc * H + h] = w;
                const float* slot = park + (size_t)h * kParkFloats + lane;
#pragma unroll
                for (int r = 0; r < kT50; ++r)
#pragma unroll
                    for (int i = 0; i < 4; ++i) joint[1 + r][i] = f32_add(joint[1 + r][i], f32_mul(w, slot[(4 * r + i) * 64]));
            }
        }
        sarl_park_barrier<GPARK>();        // the next tile's parking waits for these reads; mlp3 below touches no LDS
        if (mine) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {       // the six self features of the first row (sarl.py:42), tile 0 of mlp3's input
                const int f = 4 * g + i;
                joint[0][i] = f < 6 ? (va.rows ? va.rows[sc * H * D + f] : va.self6[sc * 6 + f]) : 0.f;
            }
            f32x4 p1[kT150], p2[kT100], p3[kT100], val[1];
            sarl_layer<1 + kT50, kT150, true>(joint, p1, W(std::integral_constant<int, 7>{}), lane);
            sarl_layer<kT150, kT100, true>(p1, p2, W(std::integral_constant<int, 8>{}), lane);
            sarl_layer<kT100, kT100, true>(p2, p3, W(std::integral_constant<int, 9>{}), lane);
            sarl_layer<kT100, 1, false>(p3, val, W(std::integral_constant<int, 10>{}), lane);
            if (live && g == 0) va.value[sc] = val[0][0];
        }
    }
}

constexpr int kMapsMaxHumans = RGL_MAX_NODES - 1;

// One wave per (root, human i) of the maps: multi_human_rl.py:117-171 in float64, every operation rounded on its own.  The lanes
// first take the other humans j one each -- the cell j falls into (or none) and j's velocity in i's frame, computed once and left in
// LDS -- then a slot each, walking the j in list order over those records: the sums and counts of a slot form as upstream's lists
// do.  The states are the roots' next human states p + v dt (dt = 0: the states themselves).
__global__ __launch_bounds__(64) void sarl_maps_kernel(const double* __restrict__ humans64, const float* __restrict__ humans32, int B, int H, double dt,
                                 int cell_num, double cell_size, int channels, float* __restrict__ maps) {
#pragma clang fp contract(off)
    __shared__ double pair_vx[kMapsMaxHumans], pair_vy[kMapsMaxHumans];
    __shared__ int pair_cell[kMapsMaxHumans];       // -1: j == i, or j outside i's grid
    const int n_slots = cell_num * cell_num * channels;
    const long long bi = blockIdx.x;
    const int i = (int)(bi % H);
    const long long b = bi / H;
    auto HB = [&](int j, int k) {
        const size_t at = ((size_t)b * H + j) * 5 + k;
        return humans64 ? humans64[at] : (double)humans32[at];
    };
    const double own_angle = atan2(HB(i, 3), HB(i, 2));
    for (int j = threadIdx.x; j < H; j += 64) {
        int cell;
        double ovx, ovy;
        sarl_map_pair(HB, i, j, own_angle, dt, cell_num, cell_size, channels, cell, ovx, ovy);
        pair_cell[j] = cell;
        pair_vx[j] = ovx;
        pair_vy[j] = ovy;
    }
    __syncthreads();
    for (int slot = threadIdx.x; slot < n_slots; slot += 64)
        maps[(size_t)bi * n_slots + slot] = sarl_map_slot(pair_cell, pair_vx, pair_vy, H, slot, channels);
}

struct SarlLayout {
    int KT[kSarlLayers], MT[kSarlLayers];
    long long off[kSarlLayers], total;      // floats
};

inline SarlLayout sarl_layout(const SarlPlanner& pl) {
    SarlLayout L;
    const int D = 13 + sarl_map_floats(pl);
    const int kt0 = (D + 15) / 16, ka = pl.with_global_state ? 2 * kT100 : kT100;
    const int KT[kSarlLayers] = {kt0, kT150, kT100, kT100, ka, kT100, kT100, 1 + kT50, kT150, kT100, kT100};
    const int MT[kSarlLayers] = {kT150, kT100, kT100, kT50, kT100, kT100, 1, kT150, kT100, kT100, 1};
    for (int l = 0; l < kSarlLayers; ++l) {
        L.KT[l] = KT[l];
        L.MT[l] = MT[l];
        L.off[l] = sarl_layer_offset(kt0, pl.with_global_state != 0, l);
    }
    L.total = L.off[kSarlLayers - 1] + (long long)MT[kSarlLayers - 1] * KT[kSarlLayers - 1] * 256 + MT[kSarlLayers - 1] * 16;
    return L;
}

int launch_sarl_pack(const SarlPlanner& pl, const SarlLayout& L, float* packed, hipStream_t st) {
    SarlPackArgs pa;
    const RglMlp* ms[4] = {&pl.mlp1, &pl.mlp2, &pl.attention, &pl.mlp3};
    int l = 0;
    for (int m = 0; m < 4; ++m)
        for (int k = 0; k < ms[m]->n_layers; ++k, ++l) {
            SarlPackJob& j = pa.job[l];
            j.src = ms[m]->weight[k];
            j.bias = ms[m]->bias[k];
            j.dst = L.off[l];
            j.K = ms[m]->dims[k];
            j.M = ms[m]->dims[k + 1];
            j.KT = L.KT[l];
            j.MT = L.MT[l];
            j.split_tile = j.KT;
            j.split_cols = j.K;
        }
    if (pl.with_global_state) {     // attention.0: [mlp1 row | mean]
        pa.job[4].split_tile = kT100;
        pa.job[4].split_cols = 100;
    }
    pa.job[7].split_tile = 1;       // mlp3.0: [self6 | weighted feature]
    pa.job[7].split_cols = 6;
    pa.out = packed;
    hipLaunchKernelGGL(sarl_pack_kernel, dim3(16, kSarlLayers), dim3(256), 0, st, pa);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

constexpr int kSarlWideFrom = 7;     // humans from which a workgroup is four waves: below, four one-wave workgroups' LDS fit a CU

template <int KT0, bool GLOBAL, int WAVES>
int launch_sarl_value_as(const SarlValueArgs& va, hipStream_t st) {
    auto kern = sarl_value_kernel<KT0, GLOBAL, WAVES>;
    const size_t lds = (size_t)va.H * kParkFloats * sizeof(float);
    if (lds > (size_t)rgl::kLdsBytesPerCu) return RGL_ERR_LDS;
    // persistent: as many workgroups as the LDS lets a CU hold (at most 8 waves), each walking tiles grid apart
    int cap = rgl::kCuCount * rgl::workgroups_per_cu_by_lds(lds, 8 / WAVES);
    const int asked = sarl_grid_cap_asked();     // tests: fewer workgroups, so that small launches walk several tiles too
    if (asked >= 1 && asked < cap) cap = asked;
    const int grid = va.n_tiles < cap ? va.n_tiles : cap;
    return rgl::launch_lds(kern, dim3(grid), dim3(64 * WAVES), lds, st, va);
}

constexpr int kSarlLdsHumans = 20;      // humans whose slots a CU's LDS holds (148 KB of 160 KB); above, the slots live in the workspace
constexpr int kSarlGlobalWaves = 4;     // waves of a workgroup of the global form, at any H
constexpr int kSarlGlobalPerCu = 2;     // workgroups of the global form per CU: what its registers allow (profiles/sarl_dense.txt)

// RGL_SARL_PARK=global (read per launch; tests): the global form at any H.  Anything else: LDS up to kSarlLdsHumans humans.
inline bool sarl_parks_globally(int H) {
    if (H > kSarlLdsHumans) return true;
    return sarl_park_global();
}

inline int sarl_global_grid(long long n_tiles) {
    int cap = rgl::kCuCount * kSarlGlobalPerCu;
    const int asked = sarl_grid_cap_asked();
    if (asked >= 1 && asked < cap) cap = asked;
    return n_tiles < cap ? (int)n_tiles : cap;
}

// bytes of the parking regions a launch over S scenes of H humans uses: one per workgroup of its grid; 0 for the LDS form
inline long long sarl_park_bytes(long long S, int H) {
    if (!sarl_parks_globally(H)) return 0;
    return align_up256((long long)sarl_global_grid((S + 15) / 16) * H * kParkFloats * (long long)sizeof(float));
}

template <int KT0, bool GLOBAL>
int launch_sarl_value_global(const SarlValueArgs& va, float* park, hipStream_t st) {
    SarlValueGlobalArgs ga;
    static_cast<SarlValueArgs&>(ga) = va;
    ga.park = park;
    hipLaunchKernelGGL((sarl_value_kernel<KT0, GLOBAL, kSarlGlobalWaves, SarlValueGlobalArgs>), dim3(sarl_global_grid(va.n_tiles)),
                       dim3(64 * kSarlGlobalWaves), 0, st, ga);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

template <int KT0, bool GLOBAL>
int launch_sarl_value_waves(const SarlValueArgs& va, float* park, hipStream_t st) {
    if (park) return launch_sarl_value_global<KT0, GLOBAL>(va, park, st);
    return va.H >= kSarlWideFrom ? launch_sarl_value_as<KT0, GLOBAL, 4>(va, st) : launch_sarl_value_as<KT0, GLOBAL, 1>(va, st);
}

// park / park_bytes: the workspace behind the packed weights, used (and required) where sarl_parks_globally(H)
int launch_sarl_value(const SarlPlanner& pl, const SarlLayout& L, const float* packed, const float* rows, const float* self6,
                      const float* hum7, const float* maps, long long S, int scenes_per_root, int H, float* value, float* attention,
                      float* park, size_t park_bytes, hipStream_t st) {
    SarlValueArgs va;
    va.packed = packed;
    va.rows = rows;
    va.self6 = self6;
    va.hum7 = hum7;
    va.maps = maps;
    va.value = value;
    va.attention = attention;
    va.S = (int)S;
    va.H = H;
    va.D = 13 + sarl_map_floats(pl);
    va.scenes_per_root = scenes_per_root;
    va.n_tiles = (int)((S + 15) / 16);
    if (!sarl_parks_globally(H)) park = nullptr;
    else if (!park || park_bytes < (size_t)sarl_park_bytes(S, H)) return RGL_ERR_WORKSPACE;
    const bool gs = pl.with_global_state != 0;
    switch (L.KT[0]) {
        case 1: return gs ? launch_sarl_value_waves<1, true>(va, park, st) : launch_sarl_value_waves<1, false>(va, park, st);
        case 2: return gs ? launch_sarl_value_waves<2, true>(va, park, st) : launch_sarl_value_waves<2, false>(va, park, st);
        case 3: return gs ? launch_sarl_value_waves<3, true>(va, park, st) : launch_sarl_value_waves<3, false>(va, park, st);
        default: return gs ? launch_sarl_value_waves<4, true>(va, park, st) : launch_sarl_value_waves<4, false>(va, park, st);
    }
}

constexpr long long kSarlMaxScenes = 1ll << 26;     // S * H * 61 stays far inside size_t; S itself inside int

// sarl_value_f32's workspace: the packed weights | the parking regions of a launch over S scenes of H humans (S = 0: the weights alone)
struct SarlValueScratch {
    float* packed;
    float* park;
    long long park_bytes, bytes;
};

inline SarlValueScratch carve_sarl_value(void* base, const SarlPlanner& pl, long long S, int H) {
    Carver c{(char*)base, 0};
    SarlValueScratch w;
    w.packed = c.take<float>(sarl_layout(pl).total * 4);
    w.park_bytes = sarl_park_bytes(S, H);
    w.park = c.take<float>(w.park_bytes);
    w.bytes = c.off;
    return w;
}

// sarl_predict_f32's workspace: the one-step buffers | attention weights [S][H] | maps [B][H][map floats] | sarl_value_f32's
struct SarlPredictScratch {
    OneStepScratch one;
    float* attention;
    float* maps;
    SarlValueScratch net;
    long long bytes;
};

inline SarlPredictScratch carve_sarl_predict(void* base, const SarlPlanner& pl, int B, int H) {
    const long long S = (long long)B * pl.num_actions;
    SarlPredictScratch w;
    w.one = carve_onestep(base, S, H);
    Carver c{(char*)base, w.one.bytes};
    w.attention = c.take<float>(S * H * 4);
    w.maps = c.take<float>((long long)B * H * sarl_map_floats(pl) * 4 + 4);
    w.net = carve_sarl_value(base ? c.base + c.off : nullptr, pl, S, H);
    w.bytes = c.off + w.net.bytes;
    return w;
}

}  // namespace

extern "C" int sarl_occupancy_maps_f32(const double* humans_f64, const float* humans, int B, int H, double time_step, int cell_num,
                                       double cell_size, int om_channel_size, float* maps, rgl_stream_t stream) {
    if ((!humans_f64 && !humans) || !maps) return RGL_ERR_NULL;
    if (sarl_map_params_rc(cell_num, cell_size, om_channel_size) == RGL_ERR_BAD_MODE) return RGL_ERR_BAD_MODE;
    if (B < 1 || H < 2 || H + 1 > RGL_MAX_NODES || sarl_map_params_rc(cell_num, cell_size, om_channel_size)) return RGL_ERR_BAD_SHAPE;
    const long long total = (long long)B * H * cell_num * cell_num * om_channel_size;
    if (total > (1ll << 31) - 256) return RGL_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(sarl_maps_kernel, dim3((unsigned)((long long)B * H)), dim3(64), 0, (hipStream_t)stream, humans_f64, humans, B,
                       H, time_step, cell_num, cell_size, om_channel_size, maps);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

extern "C" size_t sarl_value_workspace_bytes(const SarlPlanner* planner) {
    if (!planner || validate_sarl(*planner, -1)) return 0;
    return (size_t)carve_sarl_value(nullptr, *planner, 0, 0).bytes;
}

extern "C" size_t sarl_value_workspace_bytes_for(const SarlPlanner* planner, int n_scenes, int H) {
    if (!planner || n_scenes < 1 || n_scenes > kSarlMaxScenes || validate_sarl(*planner, H)) return 0;
    return (size_t)carve_sarl_value(nullptr, *planner, n_scenes, H).bytes;
}

extern "C" int sarl_value_f32(const SarlPlanner* planner, const float* rows, const float* self6, const float* hum7, const float* maps,
                              int n_scenes, int scenes_per_root, int H, void* workspace, size_t workspace_bytes, float* value,
                              float* attention, rgl_stream_t stream) {
    if (!planner || !workspace || !value || !attention) return RGL_ERR_NULL;
    const int rc = validate_sarl(*planner, H);
    if (rc) return rc;
    const SarlPlanner& pl = *planner;
    if (!rows && (!self6 || !hum7 || (pl.om_channel_size && !maps))) return RGL_ERR_NULL;
    if (n_scenes < 1 || n_scenes > kSarlMaxScenes) return RGL_ERR_BAD_SHAPE;
    if (rows) scenes_per_root = 1;
    if (scenes_per_root < 1 || n_scenes % scenes_per_root) return RGL_ERR_BAD_SHAPE;
    const SarlValueScratch w = carve_sarl_value(workspace, pl, n_scenes, H);
    if (workspace_bytes < (size_t)w.bytes) return RGL_ERR_WORKSPACE;
    const SarlLayout L = sarl_layout(pl);
    hipStream_t st = (hipStream_t)stream;
    const int prc = launch_sarl_pack(pl, L, w.packed, st);
    if (prc) return prc;
    return launch_sarl_value(pl, L, w.packed, rows, self6, hum7, maps, n_scenes, scenes_per_root, H, value, attention, w.park,
                             (size_t)w.park_bytes, st);
}

extern "C" size_t sarl_predict_workspace_bytes(const SarlPlanner* planner, int B, int H) {
    if (!planner || B < 1 || validate_sarl(*planner, H)) return 0;
    const long long S = (long long)B * planner->num_actions;
    if (planner->num_actions < 1 || planner->num_actions > RGL_MAX_ACTIONS || S > kSarlMaxScenes) return 0;
    return (size_t)carve_sarl_predict(nullptr, *planner, B, H).bytes;
}

extern "C" int sarl_predict_f32(const SarlPlanner* planner, const float* robot, const float* humans, int B, int H, void* workspace,
                                size_t workspace_bytes, float* action_values, int* best_action, float* best_value,
                                float* best_attention, rgl_stream_t stream) {
    if (!planner || !robot || !humans || !workspace || !action_values || !best_action) return RGL_ERR_NULL;
    if (B < 1) return RGL_ERR_BAD_SHAPE;
    const SarlPlanner& pl = *planner;
    // validate_sarl bounds H by RGL_MAX_NODES - 1: with the three checks behind it, everything gcn_prepare_f32 asks of a search
    int rc = validate_sarl(pl, H);
    if (rc) return rc;
    const int A = pl.num_actions;
    if (A < 1 || A > RGL_MAX_ACTIONS) return RGL_ERR_BAD_SHAPE;
    if (pl.kinematics != RGL_HOLONOMIC && pl.kinematics != RGL_UNICYCLE) return RGL_ERR_BAD_MODE;
    if (!pl.actions) return RGL_ERR_NULL;
    const long long S = (long long)B * A;
    if (S > kSarlMaxScenes) return RGL_ERR_BAD_SHAPE;
    const SarlPredictScratch w = carve_sarl_predict(workspace, pl, B, H);
    if (workspace_bytes < (size_t)w.bytes) return RGL_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // propagate, constant-velocity humans, rotate, reward: path G's first step as it stands
    rc = launch_gcn_prepare(pl.kinematics, A, pl.time_step, pl.actions, pl.root_robot_f64, pl.root_humans_f64, robot, humans, B, H,
                            w.one.self6, w.one.hum7, w.one.reward, st);
    if (rc) return rc;
    if (pl.om_channel_size) {       // once per root and human: without query_env the maps do not depend on the action (:52-55)
        const bool r64 = pl.root_robot_f64 && pl.root_humans_f64;      // as launch_gcn_prepare chooses its source
        rc = sarl_occupancy_maps_f32(r64 ? pl.root_humans_f64 : nullptr, humans, B, H, pl.time_step, pl.cell_num, pl.cell_size,
                                     pl.om_channel_size, w.maps, stream);
        if (rc) return rc;
    }
    const SarlLayout L = sarl_layout(pl);
    rc = launch_sarl_pack(pl, L, w.net.packed, st);
    if (rc) return rc;
    rc = launch_sarl_value(pl, L, w.net.packed, nullptr, w.one.self6, w.one.hum7, w.maps, S, A, H, w.one.value, w.attention, w.net.park,
                           (size_t)w.net.park_bytes, st);
    if (rc) return rc;
    return launch_onestep_select(robot, w.one.reward, w.one.value, w.attention, B, A, H, pl.gamma, pl.time_step, action_values,
                                 best_action, best_value, best_attention, st);
}
