// rgl_lstm.hip -- LSTM-RL / OM-LSTM-RL evaluation: the two value networks of crowd_nav/policy/lstm_rl.py:9-69, the distance sort of
// LstmRL.predict (:94-108) and the one-step search of multi_human_rl.py:36-64 around them.  The search's other steps (prepare,
// maps, select) are the ones path G and SARL run: rgl_onestep.h, sarl_occupancy_maps_f32.
//
// The value network is one f32 MFMA launch over all scenes.  As in rgl_sarl.hip a wave owns sixteen scenes (column n = scene n of
// every B operand), the weights are the A operand, and a 16 x 16 x 4 product leaves output row 16 mt + 4 g + i of scene n in
// register i of lane (g, n) (g = lane / 16, n = lane % 16).  The 200 gate rows of nn.LSTM (torch's order i, f, g, o, 50 units each)
// are packed as row = 4 j + q -- unit j, gate q -- into 13 output tiles: the accumulator of tile mt in lane (g, n) then IS the four
// gate pre-activations of unit j = 4 mt + g of scene n, and the cell update c <- s(f) c + s(i) tanh(g), h <- s(o) tanh(c) is
// element-wise on the four registers of one accumulator.  c and h cost 13 registers each and never leave them: the next step's
// recurrent product takes h of tile mt as the B operand of its k-step mt (k = g: the units 4 mt .. 4 mt + 3), W_hh's columns being
// packed in that order, 13 x 13 MFMAs per step.  Nothing is parked, so no LDS and no workspace form depends on H, and a workgroup is
// one wave.  `lengths` (pack_padded_sequence's hn) is a per-lane select between the old and the new (c, h).
//
// The weight fragments ([t][mt][lane][i]: one 16-byte load per lane serves four MFMAs, lstm_pack_kernel lays them out once per
// call) are read from L2 through the vector cache, as SARL's are, not staged in LDS.  The recurrent and input fragments a step
// re-reads are 104 KB at the most, which the LDS of a CU would hold for ONE workgroup only: all waves of a CU in one workgroup, behind
// a staging prologue and its barrier, and mlp1 and the head (another 230 KB, read H times and once per tile) would still come from
// L2.  Reading everything the one way keeps one layer routine for mlp1, the LSTM and the head, and leaves occupancy to the registers
// alone; tools/lstm_time.py reports the kernel's share of the f32 MFMA peak, which is where a shortfall of this choice would show.
#include "rgl_mfma.h"
#include "rgl_onestep.h"
#include "rgl_sarl_maps.h"

namespace {

constexpr int kHid = 50;                            // lstm_hidden_dim of the shipped networks
constexpr int kGateTiles = 13;                      // 4 kHid gate rows as row = 4 unit + gate: 16-row tiles (units 50, 51: zero rows)
constexpr int kHidGroups = 4;                       // h as the B operands of 13 k-steps, four k-steps to an f32x4
constexpr int kT150 = 10, kT100 = 7, kT50 = 4;      // 16-feature tiles of the shipped widths
constexpr int kLstmLayers = 10;                     // mlp1.{0,2,4,6} | W_ih | W_hh | mlp.{0,2,4,6}; without the module mlp1 is empty
constexpr int kLIh = 4, kLHh = 5, kLHead = 6;

struct LstmPackJob {
    const float* src;           // k-major [K][M] (an RglMlp layer), or torch's [M][K] (torch_layout: the LSTM tensors)
    const float* bias;          // [M]
    const float* bias2;         // [M] or null: added to `bias` (b_ih + b_hh)
    long long dst;              // float offset of the packed layer: [KT][MT][64][4] fragments, then [MT][16] bias
    int K, M, KT, MT;
    int split_tile, split_cols; // k-tiles below split_tile read columns [0, split_cols) in feature order (16 t + 4 g + i), the tiles
                                // from split_tile on read columns split_cols.. (the head: h behind the six self features)
    int torch_layout;
    int gate_rows;              // packed row 4 j + q reads source row q kHid + j (j < kHid; the rest zero)
    int unit_order;             // the k-tiles from split_tile on hold h: k index 16 t' + 4 i + g (k-step 4 t' + i, k = g)
};
struct LstmPackArgs {
    LstmPackJob job[kLstmLayers];
    float* out;
};

__global__ void lstm_pack_kernel(const LstmPackArgs pa) {
    const LstmPackJob& j = pa.job[blockIdx.y];
    const long long n_frag = (long long)j.MT * j.KT * 256, total = n_frag + j.MT * 16;
    auto src_row = [&](int row) {       // -1: a padding row
        if (!j.gate_rows) return row < j.M ? row : -1;
        const int unit = row >> 2, gate = row & 3;
        return unit < kHid ? gate * kHid + unit : -1;
    };
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (e < n_frag) {
            const int i = (int)(e & 3), lane = (int)((e >> 2) & 63);
            const int tt = (int)(e >> 8), mt = tt % j.MT, t = tt / j.MT;
            const int g = lane >> 4, m = lane & 15;
            const int row = src_row(16 * mt + m);
            int col;
            bool ok;
            if (t < j.split_tile) {
                col = 16 * t + 4 * g + i;
                ok = col < j.split_cols;
            } else {
                const int tl = t - j.split_tile;
                col = j.split_cols + (j.unit_order ? 16 * tl + 4 * i + g : 16 * tl + 4 * g + i);
                ok = col < j.K;
            }
            if (ok && row >= 0) v = j.torch_layout ? j.src[(size_t)row * j.K + col] : j.src[(size_t)col * j.M + row];
        } else {
            const int row = src_row((int)(e - n_frag));
            if (row >= 0) v = j.bias2 ? j.bias[row] + j.bias2[row] : j.bias[row];
        }
        pa.out[j.dst + e] = v;
    }
}

// out (+)= W in (+ b) over one 16-scene tile: KT input tiles, MT output tiles, every output tile an accumulator of its own (MT
// independent MFMA chains in flight per k-step).  INIT: out starts from the bias; otherwise the products are added to what out holds
// (the recurrent product on top of the input product).  KSTEPS: the k-steps that carry anything (h: 13 of 16).
template <int KT, int MT, bool RELU, bool INIT = true, int KSTEPS = 4 * KT>
__device__ __forceinline__ void lstm_layer(const f32x4 (&in)[KT], f32x4 (&out)[MT], const float* __restrict__ wp, unsigned lane) {
    // the layer's base stays a scalar the compiler cannot see through, as in rgl_sarl.hip: hoisted fragment addresses would spill
    const char* w = reinterpret_cast<const char*>(wp);
    asm volatile("" : "+s"(w));
    const unsigned lane_off = lane * 16u, bias_off = (lane >> 4) * 16u;
    if (INIT) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) out[mt] = *reinterpret_cast<const f32x4*>(w + (size_t)(MT * KT * 1024 + 64 * mt) + bias_off);
    }
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        f32x4 a[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4*>(w + (size_t)((t * MT + mt) * 1024) + lane_off);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * t + i < KSTEPS) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) out[mt] = mfma4(a[mt][i], in[t][i], out[mt]);
            }
        load_fence();
    }
    if (RELU) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) out[mt][i] = fmaxf(out[mt][i], 0.f);
    }
}

// KT / MT of packed layer l for rows of kt0 tiles; the module's four layers are empty without it
constexpr int lstm_layer_kt(int kt0, bool interact, int l) {
    const int KT[kLstmLayers] = {interact ? kt0 : 0, interact ? kT150 : 0, interact ? kT100 : 0, interact ? kT100 : 0,
                                 interact ? kT50 : kt0, kHidGroups, 1 + kHidGroups, kT150, kT100, kT100};
    return KT[l];
}
constexpr int lstm_layer_mt(bool interact, int l) {
    const int MT[kLstmLayers] = {interact ? kT150 : 0, interact ? kT100 : 0, interact ? kT100 : 0, interact ? kT50 : 0,
                                 kGateTiles, kGateTiles, kT150, kT100, kT100, 1};
    return MT[l];
}
// float offset of packed layer l (l = kLstmLayers: the total): a function of the two template parameters of the value kernel alone
constexpr int lstm_layer_offset(int kt0, bool interact, int l) {
    int off = 0;
    for (int i = 0; i < l; ++i) off += lstm_layer_mt(interact, i) * lstm_layer_kt(kt0, interact, i) * 256 + lstm_layer_mt(interact, i) * 16;
    return off;
}

// 1 / (1 + e^-x): e^-x overflows to +inf at x < -88.7 and the quotient is then 0; nothing here forms inf / inf or inf - inf.
// tanhf is the device library's, which saturates to +-1.
__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

struct LstmValueArgs {
    const float* packed;
    const float* rows;          // [S][H][D], or null: the three arrays below
    const float* self6;         // [S][6]
    const float* hum7;          // [S][H][7]
    const float* maps;          // [S / scenes_per_root][H][D - 13]; unread when D == 13
    const int* lengths;         // [S], each in 1..H, or null: every scene runs H steps
    float* value;               // [S]
    int S, H, D, scenes_per_root, n_tiles;
};

// KT0: 16-feature tiles of a row (input_dim 13 | 29 | 45 | 61); INTERACT: ValueNetwork2 (mlp1 in front of the LSTM).  A workgroup is
// one wave and walks the tiles of sixteen scenes grid apart.
template <int KT0, bool INTERACT>
__global__ __launch_bounds__(64) void lstm_value_kernel(const LstmValueArgs va) {
    const unsigned lane = threadIdx.x;
    const int g = lane >> 4, n = lane & 15;
    const int H = va.H, D = va.D;
    auto W = [&](auto l) { return va.packed + lstm_layer_offset(KT0, INTERACT, decltype(l)::value); };
    constexpr int KTI = INTERACT ? kT50 : KT0;      // tiles of what the LSTM reads

    for (int tile = blockIdx.x; tile < va.n_tiles; tile += gridDim.x) {
        const int s = tile * 16 + n;
        const bool live = s < va.S;
        const size_t sc = (size_t)(live ? s : va.S - 1);       // the partial last tile computes its last scene again, writes nothing
        const size_t root = sc / (size_t)va.scenes_per_root;
        const int len = va.lengths ? va.lengths[sc] : H;

        float c[kGateTiles];
        f32x4 hg[kHidGroups];       // hg[t][i] = h of tile 4 t + i: unit 4 (4 t + i) + g of scene n
#pragma unroll
        for (int mt = 0; mt < kGateTiles; ++mt) c[mt] = 0.f;
#pragma unroll
        for (int t = 0; t < kHidGroups; ++t) hg[t] = zero4();

        for (int h = 0; h < H; ++h) {
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
            f32x4 gates[kGateTiles];
            if constexpr (INTERACT) {
                f32x4 e[kT50];
                {
                    f32x4 p1[kT150], p2[kT100];
                    lstm_layer<KT0, kT150, true>(x, p1, W(std::integral_constant<int, 0>{}), lane);
                    lstm_layer<kT150, kT100, true>(p1, p2, W(std::integral_constant<int, 1>{}), lane);
                    f32x4 p3[kT100];
                    lstm_layer<kT100, kT100, true>(p2, p3, W(std::integral_constant<int, 2>{}), lane);
                    lstm_layer<kT100, kT50, false>(p3, e, W(std::integral_constant<int, 3>{}), lane);
                }
                lstm_layer<kT50, kGateTiles, false>(e, gates, W(std::integral_constant<int, kLIh>{}), lane);
            } else {
                lstm_layer<KTI, kGateTiles, false>(x, gates, W(std::integral_constant<int, kLIh>{}), lane);
            }
            if (h > 0)      // h_0 = 0: the first step has no recurrent term
                lstm_layer<kHidGroups, kGateTiles, false, false, kGateTiles>(hg, gates, W(std::integral_constant<int, kLHh>{}), lane);
            const bool step = h < len;
#pragma unroll
            for (int mt = 0; mt < kGateTiles; ++mt) {
                const float gi = lstm_sigmoid(gates[mt][0]), gf = lstm_sigmoid(gates[mt][1]);
                const float gg = tanhf(gates[mt][2]), go = lstm_sigmoid(gates[mt][3]);
                const float cn = gf * c[mt] + gi * gg;
                const float hn = go * tanhf(cn);
                c[mt] = step ? cn : c[mt];
                hg[mt >> 2][mt & 3] = step ? hn : hg[mt >> 2][mt & 3];
            }
        }

        // ---- the head on [row 0's six self features | h] ----
        f32x4 joint[1 + kHidGroups];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = 4 * g + i;
            joint[0][i] = f < 6 ? (va.rows ? va.rows[sc * H * D + f] : va.self6[sc * 6 + f]) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < kHidGroups; ++t) joint[1 + t] = hg[t];
        f32x4 q1[kT150], q2[kT100], q3[kT100], val[1];
        lstm_layer<1 + kHidGroups, kT150, true, true, 4 + kGateTiles>(joint, q1, W(std::integral_constant<int, kLHead>{}), lane);
        lstm_layer<kT150, kT100, true>(q1, q2, W(std::integral_constant<int, kLHead + 1>{}), lane);
        lstm_layer<kT100, kT100, true>(q2, q3, W(std::integral_constant<int, kLHead + 2>{}), lane);
        lstm_layer<kT100, 1, false>(q3, val, W(std::integral_constant<int, kLHead + 3>{}), lane);
        if (live && g == 0) va.value[sc] = val[0][0];
    }
}

// One workgroup per root: thread h takes human h's float64 distance to the robot, sqrt(dx dx + dy dy) with every operation rounded
// on its own, and its place in the order by DECREASING distance -- stable, as python's sorted(.., reverse=True) keeps the order of
// ties: rank(h) = #{j : d_j > d_h} + #{j < h : d_j = d_h}.  The humans are written in that order, float32 and (given float64 roots)
// float64, and order[b][rank] = h.
__global__ __launch_bounds__(128) void lstm_sort_kernel(const float* __restrict__ robot, const float* __restrict__ humans,
                                                        const double* __restrict__ robot64, const double* __restrict__ humans64, int H,
                                                        float* __restrict__ sorted, double* __restrict__ sorted64, int* __restrict__ order) {
#pragma clang fp contract(off)
    __shared__ double dist[RGL_MAX_NODES];
    const size_t b = blockIdx.x;
    const int h = threadIdx.x;
    if (h < H) {
        const size_t at = (b * H + h) * 5;
        const double rx = robot64 ? robot64[b * 9] : (double)robot[b * 9], ry = robot64 ? robot64[b * 9 + 1] : (double)robot[b * 9 + 1];
        const double dx = (humans64 ? humans64[at] : (double)humans[at]) - rx;
        const double dy = (humans64 ? humans64[at + 1] : (double)humans[at + 1]) - ry;
        const double xx = dx * dx, yy = dy * dy;
        dist[h] = sqrt(xx + yy);
    }
    __syncthreads();
    if (h < H) {
        const double d = dist[h];
        const bool nan = d != d;        // a NaN distance compares with nothing: such humans go last, in their given order, so that
                                        // the ranks stay a permutation whatever the states hold
        int rank = 0;
        for (int j = 0; j < H; ++j) {
            const double dj = dist[j];
            const bool before = dj != dj ? (nan && j < h) : (nan || dj > d || (j < h && dj == d));
            rank += before ? 1 : 0;
        }
        const size_t from = (b * H + h) * 5, to = (b * H + rank) * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            sorted[to + k] = humans[from + k];
            if (sorted64) sorted64[to + k] = humans64[from + k];
        }
        if (order) order[b * H + rank] = h;
    }
}

inline int lstm_map_floats(const LstmPlanner& pl) { return pl.om_channel_size ? pl.cell_num * pl.cell_num * pl.om_channel_size : 0; }

// the shapes the value kernel is built for; `H` < 0: the planner alone
inline int validate_lstm(const LstmPlanner& pl, int H) {
    int rc = pl.with_interaction_module ? rgl::validate_mlp(pl.mlp1, 0, 0) : RGL_OK;
    if (rc) return rc;
    rc = rgl::validate_mlp(pl.mlp, 0, 0);
    if (rc) return rc;
    if (!pl.weight_ih || !pl.weight_hh || !pl.bias_ih || !pl.bias_hh) return RGL_ERR_NULL;
    if (pl.om_channel_size < 0 || pl.om_channel_size > 3) return RGL_ERR_BAD_MODE;
    if (pl.om_channel_size && (pl.cell_num < 1 || pl.cell_num > 8 || !(pl.cell_size > 0.0))) return RGL_ERR_BAD_SHAPE;
    const int D = 13 + lstm_map_floats(pl);
    if (D != 13 && D != 29 && D != 45 && D != 61) return RGL_ERR_BAD_SHAPE;
    auto is = [](const RglMlp& m, int d0, int d1, int d2, int d3, int d4) {
        const int want[5] = {d0, d1, d2, d3, d4};
        if (m.n_layers != 4 || m.last_relu) return false;
        for (int l = 0; l <= 4; ++l)
            if (m.dims[l] != want[l]) return false;
        return true;
    };
    if (pl.lstm_hidden_dim != kHid || (pl.with_interaction_module && !is(pl.mlp1, D, 150, 100, 100, 50)) ||
        !is(pl.mlp, 6 + kHid, 150, 100, 100, 1))
        return RGL_ERR_BAD_SHAPE;
    if (pl.contraction_dtype != RGL_CONTRACT_F32) return RGL_ERR_BAD_MODE;
    if (H >= 0 && (H < (pl.om_channel_size ? 2 : 1) || H > RGL_SARL_MAX_HUMANS)) return RGL_ERR_BAD_SHAPE;
    return RGL_OK;
}

struct LstmLayout {
    int KT[kLstmLayers], MT[kLstmLayers];
    long long off[kLstmLayers], total;      // floats
};

inline LstmLayout lstm_layout(const LstmPlanner& pl) {
    LstmLayout L;
    const int kt0 = (13 + lstm_map_floats(pl) + 15) / 16;
    const bool interact = pl.with_interaction_module != 0;
    for (int l = 0; l < kLstmLayers; ++l) {
        L.KT[l] = lstm_layer_kt(kt0, interact, l);
        L.MT[l] = lstm_layer_mt(interact, l);
        L.off[l] = lstm_layer_offset(kt0, interact, l);
    }
    L.total = lstm_layer_offset(kt0, interact, kLstmLayers);
    return L;
}

int launch_lstm_pack(const LstmPlanner& pl, const LstmLayout& L, float* packed, hipStream_t st) {
    LstmPackArgs pa;
    const int D = 13 + lstm_map_floats(pl);
    auto mlp_job = [&](int l, const RglMlp& m, int k) {
        LstmPackJob& j = pa.job[l];
        j = LstmPackJob{};
        j.src = m.weight[k];
        j.bias = m.bias[k];
        j.dst = L.off[l];
        j.K = m.dims[k];
        j.M = m.dims[k + 1];
        j.KT = L.KT[l];
        j.MT = L.MT[l];
        j.split_tile = j.KT;
        j.split_cols = j.K;
    };
    for (int k = 0; k < 4; ++k) {
        if (pl.with_interaction_module) mlp_job(k, pl.mlp1, k);
        else pa.job[k] = LstmPackJob{};       // KT = MT = 0: nothing to write
        mlp_job(kLHead + k, pl.mlp, k);
    }
    pa.job[kLHead].split_tile = 1;      // mlp.0: [self6 | h], h in the order of its registers
    pa.job[kLHead].split_cols = 6;
    pa.job[kLHead].unit_order = 1;
    for (int l = kLIh; l <= kLHh; ++l) {
        LstmPackJob& j = pa.job[l];
        j = LstmPackJob{};
        j.dst = L.off[l];
        j.M = 4 * kHid;
        j.KT = L.KT[l];
        j.MT = L.MT[l];
        j.torch_layout = 1;
        j.gate_rows = 1;
    }
    LstmPackJob& ih = pa.job[kLIh];
    ih.src = pl.weight_ih;
    ih.bias = pl.bias_ih;       // the two biases of torch's cell as one
    ih.bias2 = pl.bias_hh;
    ih.K = pl.with_interaction_module ? 50 : D;
    ih.split_tile = ih.KT;
    ih.split_cols = ih.K;
    LstmPackJob& hh = pa.job[kLHh];
    hh.src = pl.weight_hh;
    hh.bias = pl.bias_hh;       // the slot is written, never read: the recurrent product adds to the input product
    hh.K = kHid;
    hh.unit_order = 1;
    pa.out = packed;
    hipLaunchKernelGGL(lstm_pack_kernel, dim3(16, kLstmLayers), dim3(256), 0, st, pa);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

constexpr int kLstmWavesPerCu = 8;      // one-wave workgroups a CU runs side by side: what the kernel's registers allow

template <int KT0>
int launch_lstm_value_as(bool interact, const LstmValueArgs& va, hipStream_t st) {
    // persistent: the workgroups walk tiles grid apart.  RGL_SARL_GRID_CAP (tests) asks for fewer, so that small launches walk several
    int cap = rgl::kCuCount * kLstmWavesPerCu;
    const int asked = sarl_grid_cap_asked();
    if (asked >= 1 && asked < cap) cap = asked;
    const int grid = va.n_tiles < cap ? va.n_tiles : cap;
    if (interact) hipLaunchKernelGGL((lstm_value_kernel<KT0, true>), dim3(grid), dim3(64), 0, st, va);
    else hipLaunchKernelGGL((lstm_value_kernel<KT0, false>), dim3(grid), dim3(64), 0, st, va);
    RGL_LAUNCH_CHECK();
    return RGL_OK;
}

int launch_lstm_value(const LstmPlanner& pl, const float* packed, const float* rows, const float* self6, const float* hum7,
                      const float* maps, const int* lengths, long long S, int scenes_per_root, int H, float* value, hipStream_t st) {
    LstmValueArgs va;
    va.packed = packed;
    va.rows = rows;
    va.self6 = self6;
    va.hum7 = hum7;
    va.maps = maps;
    va.lengths = lengths;
    va.value = value;
    va.S = (int)S;
    va.H = H;
    va.D = 13 + lstm_map_floats(pl);
    va.scenes_per_root = scenes_per_root;
    va.n_tiles = (int)((S + 15) / 16);
    const bool im = pl.with_interaction_module != 0;
    switch ((va.D + 15) / 16) {
        case 1: return launch_lstm_value_as<1>(im, va, st);
        case 2: return launch_lstm_value_as<2>(im, va, st);
        case 3: return launch_lstm_value_as<3>(im, va, st);
        default: return launch_lstm_value_as<4>(im, va, st);
    }
}

constexpr long long kLstmMaxScenes = 1ll << 26;     // S * H * 61 stays far inside size_t; S itself inside int

// lstm_value_f32's workspace: the packed weights
struct LstmValueScratch {
    float* packed;
    long long bytes;
};

inline LstmValueScratch carve_lstm_value(void* base, const LstmPlanner& pl) {
    Carver c{(char*)base, 0};
    LstmValueScratch w;
    w.packed = c.take<float>(lstm_layout(pl).total * 4);
    w.bytes = c.off;
    return w;
}

// lstm_predict_f32's workspace: the one-step buffers | the sorted humans, float32 and float64 | maps [B][H][map floats] | lstm_value_f32's
struct LstmPredictScratch {
    OneStepScratch one;
    float* sorted;
    double* sorted64;
    float* maps;
    LstmValueScratch net;
    long long bytes;
};

inline LstmPredictScratch carve_lstm_predict(void* base, const LstmPlanner& pl, int B, int H) {
    const long long S = (long long)B * pl.num_actions;
    LstmPredictScratch w;
    w.one = carve_onestep(base, S, H);
    Carver c{(char*)base, w.one.bytes};
    w.sorted = c.take<float>((long long)B * H * 5 * 4);
    w.sorted64 = c.take<double>((long long)B * H * 5 * 8);
    w.maps = c.take<float>((long long)B * H * lstm_map_floats(pl) * 4 + 4);
    w.net = carve_lstm_value(base ? c.base + c.off : nullptr, pl);
    w.bytes = c.off + w.net.bytes;
    return w;
}

}  // namespace

extern "C" size_t lstm_value_workspace_bytes(const LstmPlanner* planner) {
    if (!planner || validate_lstm(*planner, -1)) return 0;
    return (size_t)carve_lstm_value(nullptr, *planner).bytes;
}

extern "C" int lstm_value_f32(const LstmPlanner* planner, const float* rows, const float* self6, const float* hum7, const float* maps,
                              const int* lengths, int n_scenes, int H, int D, int scenes_per_root, void* workspace,
                              size_t workspace_bytes, float* value, rgl_stream_t stream) {
    if (!planner || !workspace || !value) return RGL_ERR_NULL;
    const int rc = validate_lstm(*planner, H);
    if (rc) return rc;
    const LstmPlanner& pl = *planner;
    if (D != 13 + lstm_map_floats(pl)) return RGL_ERR_BAD_SHAPE;
    if (!rows && (!self6 || !hum7 || (pl.om_channel_size && !maps))) return RGL_ERR_NULL;
    if (n_scenes < 1 || n_scenes > kLstmMaxScenes) return RGL_ERR_BAD_SHAPE;
    if (rows) scenes_per_root = 1;
    if (scenes_per_root < 1 || n_scenes % scenes_per_root) return RGL_ERR_BAD_SHAPE;
    const LstmValueScratch w = carve_lstm_value(workspace, pl);
    if (workspace_bytes < (size_t)w.bytes) return RGL_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int prc = launch_lstm_pack(pl, lstm_layout(pl), w.packed, st);
    if (prc) return prc;
    return launch_lstm_value(pl, w.packed, rows, self6, hum7, maps, lengths, n_scenes, scenes_per_root, H, value, st);
}

extern "C" size_t lstm_predict_workspace_bytes(const LstmPlanner* planner, int B, int H) {
    if (!planner || B < 1 || validate_lstm(*planner, H)) return 0;
    const long long S = (long long)B * planner->num_actions;
    if (planner->num_actions < 1 || planner->num_actions > RGL_MAX_ACTIONS || S > kLstmMaxScenes) return 0;
    return (size_t)carve_lstm_predict(nullptr, *planner, B, H).bytes;
}

extern "C" int lstm_predict_f32(const LstmPlanner* planner, const float* robot, const float* humans, const double* robot_f64,
                                const double* humans_f64, int B, int H, void* workspace, size_t workspace_bytes, float* action_values,
                                int* best_action, float* best_value, int* order, rgl_stream_t stream) {
    if (!planner || !robot || !humans || !workspace || !action_values || !best_action) return RGL_ERR_NULL;
    if (B < 1) return RGL_ERR_BAD_SHAPE;
    const LstmPlanner& pl = *planner;
    int rc = validate_lstm(pl, H);      // bounds H by RGL_MAX_NODES - 1: with the checks behind it, everything gcn_prepare_f32 asks
    if (rc) return rc;
    const int A = pl.num_actions;
    if (A < 1 || A > RGL_MAX_ACTIONS) return RGL_ERR_BAD_SHAPE;
    if (pl.kinematics != RGL_HOLONOMIC && pl.kinematics != RGL_UNICYCLE) return RGL_ERR_BAD_MODE;
    if (!pl.actions) return RGL_ERR_NULL;
    const long long S = (long long)B * A;
    if (S > kLstmMaxScenes) return RGL_ERR_BAD_SHAPE;
    const LstmPredictScratch w = carve_lstm_predict(workspace, pl, B, H);
    if (workspace_bytes < (size_t)w.bytes) return RGL_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const bool r64 = robot_f64 && humans_f64;      // as launch_gcn_prepare chooses its source
    // LstmRL.predict's sort: the order feeds the maps, the rows and the LSTM's sequence alike
    hipLaunchKernelGGL(lstm_sort_kernel, dim3((unsigned)B), dim3(128), 0, st, robot, humans, r64 ? robot_f64 : nullptr,
                       r64 ? humans_f64 : nullptr, H, w.sorted, r64 ? w.sorted64 : nullptr, order);
    RGL_LAUNCH_CHECK();
    const double* h64 = r64 ? w.sorted64 : nullptr;
    rc = launch_gcn_prepare(pl.kinematics, A, pl.time_step, pl.actions, r64 ? robot_f64 : nullptr, h64, robot, w.sorted, B, H,
                            w.one.self6, w.one.hum7, w.one.reward, st);
    if (rc) return rc;
    if (pl.om_channel_size) {       // once per root and human: without query_env the maps do not depend on the action
        rc = sarl_occupancy_maps_f32(h64, w.sorted, B, H, pl.time_step, pl.cell_num, pl.cell_size, pl.om_channel_size, w.maps, stream);
        if (rc) return rc;
    }
    rc = launch_lstm_pack(pl, lstm_layout(pl), w.net.packed, st);
    if (rc) return rc;
    rc = launch_lstm_value(pl, w.net.packed, nullptr, w.one.self6, w.one.hum7, w.maps, nullptr, S, A, H, w.one.value, st);
    if (rc) return rc;
    return launch_onestep_select(robot, w.one.reward, w.one.value, nullptr, B, A, H, pl.gamma, pl.time_step, action_values,
                                 best_action, best_value, nullptr, st);
}
