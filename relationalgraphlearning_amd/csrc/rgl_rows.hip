// rgl_rows.hip -- the tile pipeline's MLP row kernels (rgl_tile_pipeline.hip, steps 1, 3 and 5): rows of an MLP forward, and backward
// with parameter gradients, every dense product an fp32 MFMA.  mlp2_rows_kernel<T0, T2> for the shipped narrow MLPs (in -> 64 -> out,
// in / out <= 32: weight gradients in registers), head_rows_kernel for a workgroup that owns one tile (the value head at small
// batches) and mlp_rows_kernel for everything else (any MLP of the ABI); plan_rows_job decides which, rgl_plan_mlp_rows reports it.
#include "rgl_tile_mm.h"
#include "rgl_tiles.h"

using namespace rgl::tiles;

// -DRGL_PHASE_TIMING -DRGL_PHASE_HEAD: the phase counters belong to mlp_rows_kernel (the value head) instead of mlp2_rows_kernel
#ifdef RGL_PHASE_HEAD
#define HEAD_PHASE_START() PHASE_START()
#define HEAD_PHASE_MARK(i) PHASE_MARK(i)
#define HEAD_PHASE_FLUSH() PHASE_FLUSH()
#define ROWS2_PHASE_START() do { } while (0)
#define ROWS2_PHASE_MARK(i) do { } while (0)
#define ROWS2_PHASE_FLUSH() do { } while (0)
#else
#define HEAD_PHASE_START() do { } while (0)
#define HEAD_PHASE_MARK(i) do { } while (0)
#define HEAD_PHASE_FLUSH() do { } while (0)
#define ROWS2_PHASE_START() PHASE_START()
#define ROWS2_PHASE_MARK(i) PHASE_MARK(i)
#define ROWS2_PHASE_FLUSH() PHASE_FLUSH()
#endif

namespace {

// ------------------------------------------------------------------------------------------------
// rows of an MLP: forward, and backward with parameter gradients
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float* row_at(const RowMap& m, int r) {
    const int g = r / m.per;
    return m.p + g * m.group_stride + (long long)(r - g * m.per) * m.row_stride;
}

// weights and biases of layers [l0, l1) of the job's MLP -> the workgroup's LDS.  The layers are cut into chunks of U elements per
// thread (element e of a layer: weight e of torch-transposed [in][out], then the biases) and the chunks run as a two-deep pipeline:
// the next chunk's loads are in flight while this one's values are stored.  (Round 5 staged a column at a time, eight loads deep:
// nine dependent trips to L2 / the Infinity Cache -- the weights were just written by the optimizer step -- for the value head.)
template <int U>
__device__ __forceinline__ void stage_layers(const RowsJob& J, float* lds, int l0, int l1) {
    const RglMlp& m = J.m;
    const int step = blockDim.x, span = U * step;
    auto issue = [&](int l, int base, float (&v)[U]) {
        const int out = m.dims[l + 1], nw = m.dims[l] * out;
        const float* __restrict__ W = m.weight[l];
        const float* __restrict__ B = m.bias[l];
#pragma unroll
        for (int u = 0; u < U; ++u) {       // one unconditional load per element (a guarded one is a branch, and the loads serialise)
            const int e = base + threadIdx.x + u * step;
            const float* p = e < nw ? W + e : B + min(e - nw, out - 1);
            v[u] = *p;
        }
    };
    auto store = [&](int l, int base, const float (&v)[U]) {
        const int out = m.dims[l + 1], nw = m.dims[l] * out, n = nw + out, ld = J.w_ld[l];
        const float rcp = 1.0f / (float)out;
        float* Wl = lds + J.w_lds[l];
        float* Bl = lds + J.b_lds[l];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = base + threadIdx.x + u * step;
            if (e < nw) {
                const int k = (int)(((float)e + 0.5f) * rcp);      // e / out, exact: e < 2^16 and the quotient is at most 256
                Wl[k * ld + (e - k * out)] = v[u];
            } else if (e < n) {
                Bl[e - nw] = v[u];
            }
        }
    };
    if (l0 >= l1) return;
    // chunk (l, base) -> the one behind it; false behind the last one
    auto advance = [&](int& l, int& base) {
        base += span;
        if (base >= (m.dims[l] + 1) * m.dims[l + 1]) { ++l; base = 0; }
        return l < l1;
    };
    float va[U], vb[U];                 // ping and pong (a copy between them would wait for the loads it copies)
    int l = l0, base = 0;
    issue(l, base, va);
    while (true) {
        int ln = l, bn = base;
        bool more = advance(ln, bn);
        if (more) issue(ln, bn, vb);
        store(l, base, va);
        if (!more) break;
        l = ln; base = bn;
        more = advance(ln, bn);
        if (more) issue(ln, bn, va);
        store(l, base, vb);
        if (!more) break;
        l = ln; base = bn;
    }
}

// Workgroups of up to four waves: the MLP's weights are staged once per workgroup in LDS (k-major rows of odd stride: the forward's
// B-operand reads and the transposed reads of the delta products both stay within two-way bank conflicts), then every wave works
// through its own 16-row tiles without further barriers: every layer's activations of the tile in LDS ([16][act_ld]) together with
// two delta buffers ([16][d_ld]).  A wave's first tile writes its gradient slab, later tiles add to it (L2-resident).
//
// Round 6: a workgroup that owns ONE tile (few tiles: the value head at the reference's batch) now runs head_rows_kernel below;
// what stays here is the many-tiles form and, under RGL_HEAD_ROWS_DIRECT=0, the one-tile form as the A/B partner
// (profiles/r06_head_rows.txt: 35.7 us in round 5 -> 30.3 us here -> 23.0 us there).  What this kernel gained on the way: the first
// tile's rows, its upstream gradient and (where they are added to) its input gradients are requested BEFORE the weights, which
// arrive as a pipeline of chunks; the ReLU masks are applied where a delta is produced instead of in passes of their own with a
// barrier each; the barriers order LDS only (__syncthreads() waits for the gradient stores' acknowledgements); a shared tile's
// products deal single column tiles to the eight waves with eight k steps of operands requested at once.
constexpr int kCoopWaves = 8;          // waves of a workgroup that shares one tile (mlp_rows_kernel, coop)
constexpr int kRowsPre = 8;            // elements per lane of a 16-row tile that are requested ahead (rows of up to 32 columns)
__global__ __launch_bounds__(kCoopWaves * 64) void mlp_rows_kernel(const RowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l16 = lane & 15;
    const int ji = (a.n_jobs > 1 && (int)blockIdx.x >= a.job[1].wg_begin) ? 1 : 0;
    const RowsJob& J = a.job[ji];
    HEAD_PHASE_START();
    // coop (few tiles, wide layers: the value head): the eight waves of the workgroup share ONE tile -- the column tiles of every
    // product are dealt to them, with a workgroup barrier between phases -- instead of a tile each
    // (coop == 2: the MLP's weights do not fit LDS next to the tile -- path G's 150-100-100-1 head is 121 KB -- and every layer is
    // staged when it is needed, forward and again backward: a tile uses each weight once per direction anyway)
    const bool coop = J.coop != 0, per_layer = J.coop == 2;
    const int WV = coop ? kCoopWaves : 1, wv = coop ? wave : 0;
    const int w = coop ? (int)blockIdx.x - J.wg_begin : ((int)blockIdx.x - J.wg_begin) * J.waves_per_wg + wave;
    const bool mine = !((!coop && wave >= J.waves_per_wg) || w >= J.n_waves);
    const RglMlp& m = J.m;
    const int L = m.n_layers, ald = J.act_ld, dld = J.d_ld;
    // element-wise passes over the tile: lane -> (row rr = lane / 4, columns c4, c4 + 4, ..)
    const int rr = lane >> 2, c4 = lane & 3;
    const int d0 = m.dims[0], d0p = (d0 + 3) & ~3, dL = m.dims[L], dLp = (dL + 3) & ~3;
    const bool relu_top = m.last_relu != 0;
    // what the first tile reads from global memory, requested ahead of the weights (rows of up to 32 columns: the value head's 32)
    const bool pre_in = mine && d0p <= 4 * kRowsPre, pre_dout = mine && a.backward && dLp <= 4 * kRowsPre;
    const bool pre_din = mine && a.backward && J.need_din && J.din_add && d0 <= 4 * kRowsPre;
    float xin[kRowsPre], dov[kRowsPre], dinv[kRowsPre];
    {
        const int r0 = w * 16;
        const bool rok = mine && r0 + rr < J.n_rows;
        const int rrow = rok ? r0 + rr : (J.n_rows > 0 ? J.n_rows - 1 : 0);
        // unconditional loads from clamped addresses, the guards where the values are used, behind the barrier (a guarded load -- or
        // a guarded use the load can sink to -- is a branch with a wait inside: 24 round trips one after the other)
#pragma unroll
        for (int u = 0; u < kRowsPre; ++u) xin[u] = dov[u] = dinv[u] = 0.f;
        if (pre_in) {
            const float* src = row_at(J.in, rrow);
#pragma unroll
            for (int u = 0; u < kRowsPre; ++u) xin[u] = src[min(c4 + 4 * u, d0 - 1)];
        }
        if (pre_dout && J.d_out.p) {
            const float* src = row_at(J.d_out, rrow);
#pragma unroll
            for (int u = 0; u < kRowsPre; ++u) dov[u] = src[min(c4 + 4 * u, dL - 1)];
        }
        if (pre_din) {
            const float* src = row_at(J.d_in, rrow);
#pragma unroll
            for (int u = 0; u < kRowsPre; ++u) dinv[u] = src[min(c4 + 4 * u, d0 - 1)];
        }
    }
    if (!per_layer) stage_layers<16>(J, lds, 0, L);
    lds_barrier();
    HEAD_PHASE_MARK(0);
    if (!mine) {
        HEAD_PHASE_FLUSH();
        return;
    }
    auto sync = [&]() { if (coop) lds_barrier(); else wave_sync(); };
    float* acts = lds + J.weight_floats + (coop ? 0 : wave) * (16 * ald + 32 * dld);
    float* dcur = acts + 16 * ald;
    float* dnxt = dcur + 16 * dld;
    float* slab = J.slabs + (size_t)w * J.n_params;
    bool first = true;
    // C[16][NTL * 16] blocks of a product dealt to the waves that share the tile: one column tile each (coop) or pairs (a wave alone)
    auto product = [&](int cols, int ksteps, auto fa, auto fb, auto init, auto emit) {
        if (coop) {
            for (int jt = wv; jt * 16 < cols; jt += WV) {
                f32x4 acc[1][1];
                acc[0][0] = init(jt * 16 + l16);
                mm<1, 1, 8, true>(acc, ksteps, fa, [&](int k, int c) { return fb(k, jt * 16 + c); });
                each<1, 1>(acc, [&](int row, int c, float v, int, int, int) { emit(row, jt * 16 + c, v); });
            }
        } else {
            for (int jt = 0; jt * 16 < cols; jt += 2) {
                f32x4 acc[1][2];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[0][nt] = init((jt + nt) * 16 + l16);
                mm<1, 2, 4, true>(acc, ksteps, fa, [&](int k, int c) { return fb(k, jt * 16 + c); });
                each<1, 2>(acc, [&](int row, int c, float v, int, int, int) { emit(row, jt * 16 + c, v); });
            }
        }
    };
    for (int t = w; t < J.n_tiles; t += J.n_waves, first = false) {
        const int r0 = t * 16;
        const bool rok = r0 + rr < J.n_rows;
        const int rrow = rok ? r0 + rr : J.n_rows - 1;
        // input rows (zero beyond the end, zero in the padding columns)
        if (first && pre_in) {
#pragma unroll
            for (int u = 0; u < kRowsPre; ++u)
                if (c4 + 4 * u < d0p) acts[rr * ald + c4 + 4 * u] = (rok && c4 + 4 * u < d0) ? xin[u] : 0.f;
        } else {
            const float* src = row_at(J.in, rrow);
            gather<8>(d0p, c4, 4, [&](int c) { return (rok && c < d0) ? src[c] : 0.f; }, [&](int c, float v) { acts[rr * ald + c] = v; });
        }
        sync();
        HEAD_PHASE_MARK(1);
        for (int l = 0; l < L; ++l) {
            const int in = m.dims[l], out = m.dims[l + 1], inp = (in + 3) & ~3, outp = (out + 3) & ~3;
            const int ioff = J.act_off[l], ooff = J.act_off[l + 1];
            const bool relu = (l != L - 1) || relu_top;
            const float* W = lds + J.w_lds[l];
            const float* b = lds + J.b_lds[l];
            const int wld = J.w_ld[l];
            if (per_layer) {              // the previous layer's reads of the region ended at its barrier
                stage_layers<16>(J, lds, l, l + 1);
                lds_barrier();
            }
            if (coop && out <= 4) {
                // up to four outputs (the value head's last layer): a dot product per row on the VALU -- lane (row rr, quarter c4) sums
                // every fourth input, the four lanes of a row add up -- instead of one wave's chain of in / 4 dependent MFMAs
                // while seven waves wait
                if (wv == 0) {
                    float sum[4] = {0.f, 0.f, 0.f, 0.f};
                    for (int k0 = c4; k0 < inp; k0 += 32) {
                        float av[8], wv4[8][4];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int k = k0 + 4 * u;
                            // (a select between a load and a constant is turned into a branch around the load: a factor instead)
                            av[u] = acts[rr * ald + ioff + min(k, inp - 1)] * (k < inp ? 1.f : 0.f);
#pragma unroll
                            for (int o = 0; o < 4; ++o) wv4[u][o] = W[min(k, in - 1) * wld + min(o, out - 1)];
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u)
#pragma unroll
                            for (int o = 0; o < 4; ++o) sum[o] = fmaf(av[u], wv4[u][o], sum[o]);
                    }
#pragma unroll
                    for (int o = 0; o < 4; ++o) {
                        sum[o] += __shfl_xor(sum[o], 1);
                        sum[o] += __shfl_xor(sum[o], 2);
                        if (c4 == o && o < outp) {
                            const float v = sum[o] + b[min(o, out - 1)];
                            acts[rr * ald + ooff + o] = o < out ? (relu ? fmaxf(v, 0.f) : v) : 0.f;
                        }
                    }
                }
                sync();
                continue;
            }
            // clamped addresses, no guards (a guard becomes a branch and an LDS round trip per k step): the padding columns of the
            // activations are zero, and output columns past the end are never stored
            product(out, inp >> 2,
                    [&](int row, int k) { return acts[row * ald + ioff + k]; },
                    [&](int k, int col) { return W[min(k, in - 1) * wld + min(col, out - 1)]; },
                    [&](int col) { const float b0 = b[min(col, out - 1)], bv = col < out ? b0 : 0.f; return f32x4{bv, bv, bv, bv}; },
                    [&](int row, int col, float v) {
                        if (col < outp) acts[row * ald + ooff + col] = col < out ? (relu ? fmaxf(v, 0.f) : v) : 0.f;
                    });
            sync();
        }
        HEAD_PHASE_MARK(2);
        if (!a.backward) {
            const int ooff = J.act_off[L];
            float* dst = row_at(J.out, rrow);
            if (rok && wv == 0)
                for (int c = c4; c < dL; c += 4) dst[c] = acts[rr * ald + ooff + c];
            sync();
            continue;
        }
        {   // upstream gradient of the tile's rows, through the top layer's ReLU if it has one
            const int ooff = J.act_off[L];
            auto put = [&](int c, float v) {
                dcur[rr * dld + c] = (relu_top && !(acts[rr * ald + ooff + c] > 0.f)) ? 0.f : v;
            };
            if (first && pre_dout) {
#pragma unroll
                for (int u = 0; u < kRowsPre; ++u)
                    if (c4 + 4 * u < dLp) put(c4 + 4 * u, (J.d_out.p && rok && c4 + 4 * u < dL) ? dov[u] : 0.f);
            } else {
                const float* src = J.d_out.p ? row_at(J.d_out, rrow) : nullptr;
                gather<8>(dLp, c4, 4, [&](int c) { return (src && rok && c < dL) ? src[c] : 0.f; }, put);
            }
        }
        sync();
        HEAD_PHASE_MARK(3);
        for (int l = L - 1; l >= 0; --l) {
            const int in = m.dims[l], out = m.dims[l + 1], inp = (in + 3) & ~3, outp = (out + 3) & ~3;
            const int ioff = J.act_off[l];
            const float* W = lds + J.w_lds[l];
            const int wld = J.w_ld[l];
            if (per_layer && (l > 0 || J.need_din)) stage_layers<16>(J, lds, l, l + 1);      // read after the barrier below
            HEAD_PHASE_MARK(4);
            // dW^T[o][i] = sum_rows delta[row][o] act[row][i]   (M = outputs, N = inputs, K = the tile's 16 rows: the tile's columns
            // run along the contiguous dimension of torch's [out][in] layout, so a wave's stores are 64-byte runs)
            float* gW = slab + J.w_off[l];
            // blocks (ot, it) of 16 outputs x 32 inputs, dealt round-robin to the waves that share the tile
            const int nit = (in + 31) >> 5, nblocks = ((out + 15) >> 4) * nit;
            for (int blk = wv, ot = 0, itp = wv; blk < nblocks; blk += WV, itp += WV) {
                    while (itp >= nit) { itp -= nit; ++ot; }
                    const int it = 2 * itp;
                    f32x4 acc[1][2];
                    clear<1, 2>(acc);
                    if (!first) {                    // later tiles of the wave: the MFMAs accumulate on top of the slab's values
                        const int kq = lane >> 4;
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int o = ot * 16 + 4 * kq + r, i = (it + nt) * 16 + l16;
                                if (i < in && o < out) acc[0][nt][r] = gW[(size_t)o * in + i];
                            }
                    }
                    mm<1, 2, 4, true>(acc, 4,
                                [&](int mo, int k) { return dcur[k * dld + min(ot * 16 + mo, outp - 1)]; },
                                [&](int k, int c) { return acts[k * ald + ioff + min(it * 16 + c, inp - 1)]; });
                    each<1, 2>(acc, [&](int mo, int c, float v, int, int, int) {
                        const int o = ot * 16 + mo, i = it * 16 + c;
                        if (i < in && o < out) gW[(size_t)o * in + i] = v;
                    });
                }
            float* gb = slab + J.b_off[l];
            for (int c = lane + 64 * wv; c < out; c += 64 * WV) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) s += dcur[r * dld + c];
                gb[c] = first ? s : gb[c] + s;
            }
            HEAD_PHASE_MARK(5);
            if (l > 0 || J.need_din) {
                // delta_in[row][i] = sum_o delta[row][o] W[i][o], through the ReLU that produced input i (every layer below the top
                // one has it; the MLP's own input has none)
                if (per_layer) lds_barrier();
                const bool mask = l > 0;
                product(in, outp >> 2,
                        [&](int row, int k) { return dcur[row * dld + k]; },
                        [&](int k, int col) { return W[min(col, in - 1) * wld + min(k, out - 1)]; },
                        [&](int) { return zero4(); },
                        [&](int row, int i, float v) {
                            const float ai = acts[row * ald + ioff + min(i, inp - 1)];       // read unguarded, selected below
                            if (i < inp) dnxt[row * dld + i] = (i < in && !(mask && !(ai > 0.f))) ? v : 0.f;
                        });
            }
            sync();
            HEAD_PHASE_MARK(6);
            float* tmp = dcur;
            dcur = dnxt;
            dnxt = tmp;
        }
        if (J.need_din && wv == 0) {
            float* dst = row_at(J.d_in, rrow);
            if (first && (pre_din || (!J.din_add && d0 <= 4 * kRowsPre))) {
#pragma unroll
                for (int u = 0; u < kRowsPre; ++u) {
                    const int c = c4 + 4 * u;
                    if (rok && c < d0) dst[c] = (pre_din ? dinv[u] : 0.f) + dcur[rr * dld + c];
                }
            } else {
                gather<8>(d0, c4, 4, [&](int c) { return (J.din_add && rok) ? dst[c] : 0.f; },
                          [&](int c, float v) { if (rok) dst[c] = v + dcur[rr * dld + c]; });
            }
        }
        sync();
        HEAD_PHASE_MARK(7);
    }
    HEAD_PHASE_FLUSH();
}

// ------------------------------------------------------------------------------------------------
// rows of a wide MLP, a workgroup per 16-row tile, the weights straight from L2 (round 6)
// ------------------------------------------------------------------------------------------------
// The value head's rows at the reference's batch (100 scenes = 7 tiles) are latency, not work: with one tile per workgroup every
// weight is used ONCE per product, so staging the matrices in LDS (mlp_rows_kernel) only adds a round trip and an LDS read per
// MFMA operand -- 35.7 us for 0.6 us of MFMA time in round 5 (profiles/r06_head_rows.txt).  Here the B operands of every product come from
// global memory as the loads of a whole column tile in flight at once, LDS holds the tile's activations and deltas only (so any MLP
// of the ABI fits: path G's 150-100-100-1 head needs no per-layer staging), and the k slots of the MFMA are permuted -- slot
// (g, kk, u) <-> k = 16 g + 4 kk + u -- so that a lane's four k of a group are adjacent: one b128 read of its A row, and for the
// transposed products (delta_in: W[i][o] along o) one dwordx4 load per group.  Same arithmetic as mlp_rows_kernel up to the order
// of the k sum inside a product.  23.0 us against 30.3 for the batch-100 value head (7 workgroups); what remains is seven dependent
// products of ~2 us each -- one compute unit pulling a 40 KB matrix out of L2 per product -- and ~5 us of launch, row traffic and
// barriers (ablations in DESIGN §9).
constexpr int kDirectGroups = 8;       // 16-k groups of operands requested per batch (128 k: 32 + 32 registers)

// acc += A[16][16 K16] B[16 K16][16]: `arow` = this lane's A row (LDS, 16-byte aligned groups, zeros where k is past the end),
// fb(g, kk) = the four B values of k = 16 g + 4 kk .. + 3 for this lane's column
template <class FB>
__device__ __forceinline__ void direct_mm(f32x4& acc, const float* arow, int K16, FB fb) {
    const int kk = (threadIdx.x & 63) >> 4;
    for (int g0 = 0; g0 < K16; g0 += kDirectGroups) {
        f32x4 bv[kDirectGroups], av[kDirectGroups];
#pragma unroll
        for (int g = 0; g < kDirectGroups; ++g) bv[g] = fb(min(g0 + g, K16 - 1), kk);       // past the end: the last group again
#pragma unroll
        for (int g = 0; g < kDirectGroups; ++g) av[g] = *reinterpret_cast<const f32x4*>(arow + 16 * min(g0 + g, K16 - 1) + 4 * kk);
        __builtin_amdgcn_sched_barrier(0);             // every operand requested before the first MFMA
#pragma unroll
        for (int g = 0; g < kDirectGroups; ++g)
            if (g0 + g < K16) {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = mfma4(av[g][u], bv[g][u], acc);
            }
    }
}

__global__ __launch_bounds__(kCoopWaves * 64) void head_rows_kernel(const RowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l16 = lane & 15, kq = lane >> 4;
    const int ji = (a.n_jobs > 1 && (int)blockIdx.x >= a.job[1].wg_begin) ? 1 : 0;
    const RowsJob& J = a.job[ji];
    HEAD_PHASE_START();
    const int w = (int)blockIdx.x - J.wg_begin;
    if (w >= J.n_waves) return;
    const RglMlp& m = J.m;
    const int L = m.n_layers, ald = J.act_ld, dld = J.d_ld;
    float* acts = lds;                         // [16][ald]: every layer's activations, each in a region of a multiple of 16 columns
    float* dcur = acts + 16 * ald;             // [16][dld] twice: the deltas of the layer at hand and of the one below
    float* dnxt = dcur + 16 * dld;
    float* slab = J.slabs + (size_t)w * J.n_params;
    const int rr = lane >> 2, c4 = lane & 3;   // element-wise passes: lane -> (row rr, columns c4, c4 + 4, ..)
    const int d0 = m.dims[0], dL = m.dims[L];
    const bool relu_top = m.last_relu != 0;
    bool first = true;
    for (int t = w; t < J.n_tiles; t += J.n_waves, first = false) {
        const int r0 = t * 16;
        const bool rok = r0 + rr < J.n_rows;
        const int rrow = rok ? r0 + rr : J.n_rows - 1;
        {   // input rows: every column of the region written (zeros beyond the row's end and beyond the last row)
            const float* src = row_at(J.in, rrow);
            const int d16 = (d0 + 15) & ~15;
            for (int c0 = c4; c0 < d16; c0 += 32) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = src[min(c0 + 4 * u, d0 - 1)];          // unguarded loads, guarded values
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (c0 + 4 * u < d16)        // a factor, not a select: a select around a load becomes a branch with a wait inside
                        acts[rr * ald + c0 + 4 * u] = v[u] * ((rok && c0 + 4 * u < d0) ? 1.f : 0.f);
            }
        }
        lds_barrier();
        HEAD_PHASE_MARK(1);
        for (int l = 0; l < L; ++l) {
            const int in = m.dims[l], out = m.dims[l + 1], K16 = (in + 15) >> 4;
            const int ioff = J.act_off[l], ooff = J.act_off[l + 1];
            const bool relu = (l != L - 1) || relu_top;
            const float* __restrict__ W = m.weight[l];
            const float* __restrict__ B = m.bias[l];
            {
                for (int jt = wv; jt * 16 < out; jt += kCoopWaves) {
                    const int col = jt * 16 + l16, colc = min(col, out - 1);
                    const float bv = B[colc];
                    f32x4 acc = f32x4{bv, bv, bv, bv};
                    // Addresses: a wave-uniform base (row 16 g + u of the matrix: scalar arithmetic) plus ONE 32-bit offset per lane
                    // that serves every load of the tile -- per-load 64-bit multiplies and clamps cost more VALU time than the
                    // product's MFMAs.  Only the last group of a ragged K clamps its rows (their A values are zeros).
                    const unsigned lane_off = (unsigned)(4 * kq * out + colc);
                    direct_mm(acc, acts + l16 * ald + ioff, K16, [&](int g, int kk) {
                        if (16 * g + 15 < in) {
                            const float* __restrict__ Wg = W + (size_t)(16 * g) * (size_t)out;
                            return f32x4{Wg[lane_off], (Wg + out)[lane_off], (Wg + 2 * out)[lane_off], (Wg + 3 * out)[lane_off]};
                        }
                        const int k = 16 * g + 4 * kk;
                        const float* __restrict__ Wc = W + colc;
                        return f32x4{Wc[(size_t)min(k, in - 1) * out], Wc[(size_t)min(k + 1, in - 1) * out],
                                     Wc[(size_t)min(k + 2, in - 1) * out], Wc[(size_t)min(k + 3, in - 1) * out]};
                    });
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        acts[(4 * kq + r) * ald + ooff + col] = col < out ? (relu ? fmaxf(acc[r], 0.f) : acc[r]) : 0.f;
                }
            }
            lds_barrier();
        }
        HEAD_PHASE_MARK(2);
        if (!a.backward) {
            const int ooff = J.act_off[L];
            float* dst = row_at(J.out, rrow);
            if (rok && wv == 0)
                for (int c = c4; c < dL; c += 4) dst[c] = acts[rr * ald + ooff + c];
            lds_barrier();
            continue;
        }
        {   // upstream gradient of the tile's rows, through the top layer's ReLU if it has one; zeros up to a multiple of 16 columns
            const int ooff = J.act_off[L], d16 = (dL + 15) & ~15;
            const float* src = J.d_out.p ? row_at(J.d_out, rrow) : row_at(J.in, rrow);
            const bool have = J.d_out.p != nullptr;
            for (int c0 = c4; c0 < d16; c0 += 32) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = src[have ? min(c0 + 4 * u, dL - 1) : 0];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int c = c0 + 4 * u;
                    if (c < d16) {
                        const float ac = acts[rr * ald + ooff + c];
                        dcur[rr * dld + c] = v[u] * ((have && rok && c < dL && !(relu_top && !(ac > 0.f))) ? 1.f : 0.f);
                    }
                }
            }
        }
        lds_barrier();
        HEAD_PHASE_MARK(3);
        for (int l = L - 1; l >= 0; --l) {
            const int in = m.dims[l], out = m.dims[l + 1], in16 = (in + 15) & ~15, out16 = (out + 15) & ~15;
            const int ioff = J.act_off[l];
            const float* __restrict__ W = m.weight[l];
            // dW^T[o][i] = sum_rows delta[row][o] act[row][i]   (M = outputs, N = inputs, K = the tile's 16 rows: the tile's columns
            // run along the contiguous dimension of torch's [out][in] layout, so a wave's stores are 64-byte runs); blocks (ot, it) of
            // 16 outputs x 32 inputs, dealt round-robin to the waves
            float* gW = slab + J.w_off[l];
            const int nit = (in + 31) >> 5, nblocks = (out16 >> 4) * nit;
            for (int blk = wv, ot = 0, itp = wv; blk < nblocks; blk += kCoopWaves, itp += kCoopWaves) {
                while (itp >= nit) { itp -= nit; ++ot; }
                const int it = 2 * itp;
                f32x4 acc[1][2];
                clear<1, 2>(acc);
                if (!first) {                    // later tiles of the workgroup: the MFMAs accumulate on top of the slab's values
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int o = ot * 16 + 4 * kq + r, i = (it + nt) * 16 + l16;
                            if (i < in && o < out) acc[0][nt][r] = gW[(size_t)o * in + i];
                        }
                }
                mm<1, 2, 4, true>(acc, 4,
                                  [&](int mo, int k) { return dcur[k * dld + ot * 16 + mo]; },
                                  [&](int k, int c) { return acts[k * ald + ioff + min(it * 16 + c, in16 - 1)]; });
                each<1, 2>(acc, [&](int mo, int c, float v, int, int, int) {
                    const int o = ot * 16 + mo, i = it * 16 + c;
                    if (i < in && o < out) gW[(size_t)o * in + i] = v;
                });
            }
            float* gb = slab + J.b_off[l];
            for (int c = lane + 64 * wv; c < out; c += 64 * kCoopWaves) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) s += dcur[r * dld + c];
                gb[c] = first ? s : gb[c] + s;
            }
            HEAD_PHASE_MARK(5);
            if (l > 0 || J.need_din) {
                // delta_in[row][i] = sum_o delta[row][o] W[i][o], through the ReLU that produced input i (every layer below the top
                // one has it; the MLP's own input has none).  W[i][.] is contiguous along the sum: a dwordx4 per group where the
                // row length allows the alignment
                const bool mask = l > 0, vec = (out & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
                const int K16 = out16 >> 4;
                for (int jt = wv; jt * 16 < in16; jt += kCoopWaves) {
                    const int i = jt * 16 + l16, ic = min(i, in - 1);
                    const float* __restrict__ Wi = W + (size_t)ic * out;
                    f32x4 acc = zero4();
                    const unsigned lane_off = (unsigned)(ic * out + 4 * kq);
                    if (vec)
                        direct_mm(acc, dcur + l16 * dld, K16, [&](int g, int kk) {
                            if (16 * g + 15 < out)           // uniform base + the lane's offset, as in the forward products
                                return *reinterpret_cast<const f32x4*>(W + 16 * g + lane_off);
                            // a quad past the row's end: the last one again (its delta values are zeros)
                            return *reinterpret_cast<const f32x4*>(Wi + min(16 * g + 4 * kk, out - 4));
                        });
                    else
                        direct_mm(acc, dcur + l16 * dld, K16, [&](int g, int kk) {
                            const int k = 16 * g + 4 * kk;
                            return f32x4{Wi[min(k, out - 1)], Wi[min(k + 1, out - 1)], Wi[min(k + 2, out - 1)], Wi[min(k + 3, out - 1)]};
                        });
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 4 * kq + r;
                        const float ai = acts[row * ald + ioff + i];                   // i < in16: inside the region
                        dnxt[row * dld + i] = (i < in && !(mask && !(ai > 0.f))) ? acc[r] : 0.f;
                    }
                }
            }
            lds_barrier();
            HEAD_PHASE_MARK(6);
            float* tmp = dcur;
            dcur = dnxt;
            dnxt = tmp;
        }
        if (J.need_din && wv == 0) {
            float* dst = row_at(J.d_in, rrow);
            for (int c0 = c4; c0 < d0; c0 += 32) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = J.din_add ? dst[min(c0 + 4 * u, d0 - 1)] : 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (rok && c0 + 4 * u < d0) dst[c0 + 4 * u] = v[u] + dcur[rr * dld + c0 + 4 * u];
            }
        }
        lds_barrier();
        HEAD_PHASE_MARK(7);
    }
    HEAD_PHASE_FLUSH();
}

// The shipped narrow MLPs -- in -> 64 -> out with in, out <= 32: w_r, w_h (9 | 5 | 6 | 7 -> 64 -> 32), the motion head
// (32 -> 64 -> 5) -- carry nearly all rows of a batch (every node of every scene).  Same organisation as mlp_rows_kernel, but the
// shapes are template parameters (T0 / T2 = 16-wide tiles of the input / output): every k loop is unrolled with its operand loads
// batched, and the weight gradients of BOTH layers stay in MFMA accumulators over all tiles of the wave -- (4 T0 + 4 T2) tiles, 48
// registers -- so a wave touches its slab once, at the end.
constexpr int kNarrowWaves = 4;       // waves per workgroup of mlp2_rows_kernel: three workgroups fit a CU (40 KB of LDS each, <= 170 VGPRs)
template <int T0, int T2>
__global__ __launch_bounds__(kNarrowWaves * 64, 3) void mlp2_rows_kernel(const RowsArgs a) {
    constexpr int HT = 4, IN_LD = T0 * 16 + 2, HLD = 66, OLD = T2 * 16 + 2;
    constexpr int kWaveFloats = 16 * (IN_LD + HLD + OLD);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15;
    const int ji = (a.n_jobs > 1 && (int)blockIdx.x >= a.job[1].wg_begin) ? 1 : 0;
    const RowsJob& J = a.job[ji];
    ROWS2_PHASE_START();
    const int w = ((int)blockIdx.x - J.wg_begin) * J.waves_per_wg + wave;
    const bool on = wave < J.waves_per_wg && w < J.n_waves;
    const RglMlp& m = J.m;
    const int in = m.dims[0], out = m.dims[2];
    const float* W0 = lds + J.w_lds[0];
    const float* W1 = lds + J.w_lds[1];
    const float* b0 = lds + J.b_lds[0];
    const float* b1 = lds + J.b_lds[1];
    constexpr int wld0 = 65, wld1 = T2 * 16 + 1;      // compile-time row strides of the two weight matrices in LDS (plan_rows_job)
    float* xin = lds + J.weight_floats + wave * kWaveFloats;      // [16][IN_LD]   input rows, zero beyond `in`; later the input deltas
    float* hid = xin + 16 * IN_LD;                                // [16][HLD]     hidden activations
    float* d1 = hid + 16 * HLD;                                   // [16][OLD]     outputs, then their deltas (zero beyond `out`)
    float* d0 = hid;                                              // the hidden deltas replace the hidden activations in place (each
                                                                  // element is read -- its ReLU mask -- and written by the same lane)
    const bool last_relu = m.last_relu != 0;
    f32x4 gW0[HT][T0], gW1[T2][HT];
    clear<HT, T0>(gW0);
    clear<T2, HT>(gW1);
    float gb0 = 0.f, gb1 = 0.f;
    const int rr = lane >> 2, c4 = lane & 3;
    // the rows of a tile (inputs, and upstream deltas in a backward launch) are fetched one tile ahead: lane -> (row lane / 4,
    // columns lane % 4 + 4 u); the first tile's before the weights, so that the two latencies overlap
    float vin[T0 * 4], vd[T2 * 4];
    auto fetch = [&](int t) {
        const bool ok = t < J.n_tiles && t * 16 + rr < J.n_rows;
        const int row = ok ? t * 16 + rr : 0;
        const float* src = row_at(J.in, row);
#pragma unroll
        for (int u = 0; u < T0 * 4; ++u) vin[u] = (ok && c4 + 4 * u < in) ? src[c4 + 4 * u] : 0.f;
        if (a.backward) {
            const float* dsrc = J.d_out.p ? row_at(J.d_out, row) : nullptr;
#pragma unroll
            for (int u = 0; u < T2 * 4; ++u) vd[u] = (dsrc && ok && c4 + 4 * u < out) ? dsrc[c4 + 4 * u] : 0.f;
        }
    };
    fetch(on ? w : J.n_tiles);
    {   // both layers' weights and biases -> LDS, padded with zeros to whole tiles (rows of W0 beyond `in`, columns of W1 / b1 beyond
        // `out`): the k loops then need neither guards nor clamps, and every LDS address is a base register plus a constant
        constexpr int n0 = T0 * 16 * 64, n1 = 64 * T2 * 16, nb = n0 + n1, total = nb + 64 + T2 * 16;
        const float* __restrict__ g0 = m.weight[0];
        const float* __restrict__ g1 = m.weight[1];
        const float* __restrict__ gb0p = m.bias[0];
        const float* __restrict__ gb1p = m.bias[1];
        gather<7>(total, threadIdx.x, kNarrowWaves * 64,
                  [&](int idx) {
                      if (idx < n0) return (idx >> 6) < in ? g0[idx] : 0.f;
                      if (idx < nb) { const int j = idx - n0, k = j / (T2 * 16), c = j % (T2 * 16); return c < out ? g1[k * out + c] : 0.f; }
                      if (idx < nb + 64) return gb0p[idx - nb];
                      return idx - nb - 64 < out ? gb1p[idx - nb - 64] : 0.f;
                  },
                  [&](int idx, float v) {
                      if (idx < n0) lds[J.w_lds[0] + (idx >> 6) * wld0 + (idx & 63)] = v;
                      else if (idx < nb) { const int j = idx - n0; lds[J.w_lds[1] + (j / (T2 * 16)) * wld1 + j % (T2 * 16)] = v; }
                      else if (idx < nb + 64) lds[J.b_lds[0] + idx - nb] = v;
                      else lds[J.b_lds[1] + idx - nb - 64] = v;
                  });
    }
    __syncthreads();
    ROWS2_PHASE_MARK(0);
    if (!on) return;
    for (int t = w; t < J.n_tiles; t += J.n_waves) {
        const int r0 = t * 16;
        const bool rok = r0 + rr < J.n_rows;
        const int rrow = rok ? r0 + rr : J.n_rows - 1;
        float vdc[T2 * 4];
#pragma unroll
        for (int u = 0; u < T0 * 4; ++u) xin[rr * IN_LD + c4 + 4 * u] = vin[u];
#pragma unroll
        for (int u = 0; u < T2 * 4; ++u) vdc[u] = vd[u];
        fetch(t + J.n_waves);
        wave_sync();
        ROWS2_PHASE_MARK(1);
        {   // hidden = relu(x W0 + b0)
            f32x4 acc[1][HT];
#pragma unroll
            for (int nt = 0; nt < HT; ++nt) {
                const float bv = b0[nt * 16 + l16];
                acc[0][nt] = f32x4{bv, bv, bv, bv};
            }
            mm<1, HT, 4>(acc, T0 * 4, [&](int row, int k) { return xin[row * IN_LD + k]; },
                              [&](int k, int c) { return W0[k * wld0 + c]; });
            each<1, HT>(acc, [&](int row, int c, float v, int, int, int) { hid[row * HLD + c] = fmaxf(v, 0.f); });
        }
        wave_sync();
        ROWS2_PHASE_MARK(2);
        {   // y = hidden W1 + b1 (ReLU when the MLP ends with one)
            f32x4 acc[1][T2];
#pragma unroll
            for (int nt = 0; nt < T2; ++nt) {
                const int col = nt * 16 + l16;
                const float bv = b1[col];
                acc[0][nt] = f32x4{bv, bv, bv, bv};
            }
            mm<1, T2, 4>(acc, 16, [&](int row, int k) { return hid[row * HLD + k]; },
                         [&](int k, int c) { return W1[k * wld1 + c]; });
            each<1, T2>(acc, [&](int row, int c, float v, int, int, int) { d1[row * OLD + c] = last_relu ? fmaxf(v, 0.f) : v; });
        }
        wave_sync();
        ROWS2_PHASE_MARK(3);
        if (!a.backward) {
            float* dst = row_at(J.out, rrow);
            if (rok)
                for (int c = c4; c < out; c += 4) dst[c] = d1[rr * OLD + c];
            wave_sync();
            continue;
        }
        {   // upstream deltas through the last ReLU; zero in the padding columns
#pragma unroll
            for (int u = 0; u < T2 * 4; ++u) {
                const int c = c4 + 4 * u;
                d1[rr * OLD + c] = (last_relu && !(d1[rr * OLD + c] > 0.f)) ? 0.f : vdc[u];
            }
        }
        wave_sync();
        ROWS2_PHASE_MARK(4);
        // dW1^T[o][h] += sum_rows delta1[row][o] hidden[row][h]
        mm<T2, HT, 4>(gW1, 4, [&](int mo, int k) { return d1[k * OLD + mo]; }, [&](int k, int c) { return hid[k * HLD + c]; });
        if (lane < T2 * 16) {
#pragma unroll
            for (int r = 0; r < 16; ++r) gb1 += d1[r * OLD + lane];
        }
        {   // delta0 = (delta1 W1^T) where the hidden ReLU is open
            f32x4 acc[1][HT];
            clear<1, HT>(acc);
            mm<1, HT, 4>(acc, T2 * 4, [&](int row, int k) { return d1[row * OLD + k]; },
                              [&](int k, int c) { return W1[c * wld1 + k]; });
            each<1, HT>(acc, [&](int row, int c, float v, int, int, int) { d0[row * HLD + c] = hid[row * HLD + c] > 0.f ? v : 0.f; });
        }
        wave_sync();
        ROWS2_PHASE_MARK(5);
        // dW0^T[h][i] += sum_rows delta0[row][h] x[row][i]
        mm<HT, T0, 4>(gW0, 4, [&](int mh, int k) { return d0[k * HLD + mh]; }, [&](int k, int c) { return xin[k * IN_LD + c]; });
#pragma unroll
        for (int r = 0; r < 16; ++r) gb0 += d0[r * HLD + lane];
        ROWS2_PHASE_MARK(6);
        if (J.need_din) {
            f32x4 acc[1][T0];
            clear<1, T0>(acc);
            mm<1, T0, 4>(acc, 16, [&](int row, int k) { return d0[row * HLD + k]; },
                         [&](int k, int c) { return W0[c * wld0 + k]; });
            wave_sync();                          // every lane has read x for dW0
            each<1, T0>(acc, [&](int row, int c, float v, int, int, int) { xin[row * IN_LD + c] = v; });
            wave_sync();
            float* dst = row_at(J.d_in, rrow);
            float v[T0 * 4];
#pragma unroll
            for (int u = 0; u < T0 * 4; ++u) v[u] = (J.din_add && rok && c4 + 4 * u < in) ? dst[c4 + 4 * u] : 0.f;
#pragma unroll
            for (int u = 0; u < T0 * 4; ++u) {
                const int c = c4 + 4 * u;
                if (rok && c < in) dst[c] = v[u] + xin[rr * IN_LD + c];
            }
        }
        wave_sync();
        ROWS2_PHASE_MARK(7);
    }
    ROWS2_PHASE_FLUSH();
    if (a.backward) {
        float* slab = J.slabs + (size_t)w * J.n_params;
        each<HT, T0>(gW0, [&](int h, int i, float v, int, int, int) { if (i < in) slab[J.w_off[0] + h * in + i] = v; });
        each<T2, HT>(gW1, [&](int o, int h, float v, int, int, int) { if (o < out) slab[J.w_off[1] + o * 64 + h] = v; });
        slab[J.b_off[0] + lane] = gb0;
        if (lane < out) slab[J.b_off[1] + lane] = gb1;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
namespace rgl {
namespace tiles {

void plan_rows_job(RowsJob& J, const RglMlp& m, int n_rows, int max_waves) {
    J = RowsJob{};
    J.m = m;
    int off = 0, col = 0, widest = 0, wl = 0;
    for (int l = 0; l < m.n_layers; ++l) {
        J.w_off[l] = off; off += m.dims[l] * m.dims[l + 1];
        J.b_off[l] = off; off += m.dims[l + 1];
        J.w_ld[l] = m.dims[l + 1] | 1;
        J.w_lds[l] = wl; wl += (m.dims[l] * J.w_ld[l] + 3) & ~3;
        J.b_lds[l] = wl; wl += (m.dims[l + 1] + 3) & ~3;
    }
    for (int l = 0; l <= m.n_layers; ++l) {
        J.act_off[l] = col;
        col += (m.dims[l] + 3) & ~3;
        widest = m.dims[l] > widest ? m.dims[l] : widest;
    }
    J.weight_floats = wl;
    J.n_params = off;
    J.act_ld = col + 2;                         // rows two banks apart
    J.d_ld = ((widest + 3) & ~3) + 2;
    J.n_rows = n_rows;
    J.n_tiles = (n_rows + 15) / 16;
    J.n_waves = J.n_tiles < max_waves ? J.n_tiles : max_waves;
    if (m.n_layers == 2 && m.dims[1] == 64 && m.dims[0] <= 32 && m.dims[2] <= 32) {
        const int T0 = (m.dims[0] + 15) / 16, T2 = (m.dims[2] + 15) / 16;
        J.kind = 10 * T0 + T2;
        J.w_ld[0] = 65; J.w_ld[1] = T2 * 16 + 1;           // the strides mlp2_rows_kernel<T0, T2> is compiled for
        J.w_lds[0] = 0; J.b_lds[0] = (T0 * 16 * 65 + 3) & ~3;        // W0 padded to T0 * 16 rows, W1 / b1 to T2 * 16 columns
        J.w_lds[1] = J.b_lds[0] + 64; J.b_lds[1] = J.w_lds[1] + ((64 * J.w_ld[1] + 3) & ~3);
        J.weight_floats = J.b_lds[1] + 32;
        J.waves_per_wg = kNarrowWaves;
        J.n_wgs = (J.n_waves + kNarrowWaves - 1) / kNarrowWaves;
        J.wave_floats = 16 * ((T0 * 16 + 2) + 66 + (T2 * 16 + 2));
        return;
    }
    // The direct form below keeps no weights in LDS and returns without a fit check: its tile is largest with every layer at the ABI's
    // widest, and even that fits one CU (148 224 of 163 840 bytes).  validate_mlp holds every job to these limits before it is planned.
    static_assert((16 * ((RGL_MAX_MLP_LAYERS + 1) * RGL_MAX_WIDTH + 4) + 32 * (RGL_MAX_WIDTH + 4)) * sizeof(float) <=
                      (size_t)rgl::kLdsBytesPerCu - 1024,
                  "head_rows_kernel: a tile of the deepest, widest MLP the ABI admits must fit the LDS of one CU");
    if (rows_direct() && J.n_tiles <= 1024) {
        // few tiles: a workgroup per tile, the weights straight from L2 (head_rows_kernel): the tile's activations and deltas are all
        // that lives in LDS, every layer in a region of a multiple of 16 columns, rows 16 bytes aligned and four banks apart
        col = 0; widest = 0;
        for (int l = 0; l <= m.n_layers; ++l) {
            J.act_off[l] = col;
            col += (m.dims[l] + 15) & ~15;
            widest = m.dims[l] > widest ? m.dims[l] : widest;
        }
        J.act_ld = col + 4;
        J.d_ld = ((widest + 15) & ~15) + 4;
        J.wave_floats = 16 * J.act_ld + 32 * J.d_ld;
        J.weight_floats = 0;
        J.kind = 1;
        J.coop = 1;
        J.waves_per_wg = 1;
        J.n_wgs = J.n_waves;
        return;
    }
    J.wave_floats = 16 * J.act_ld + 32 * J.d_ld;
    if (J.n_tiles <= 1024 && ((size_t)wl + J.wave_floats) * sizeof(float) <= (size_t)rgl::kLdsBytesPerCu - 1024) {
        J.coop = 1;                             // few tiles: a workgroup per tile (the value head: one row per scene)
        J.waves_per_wg = 1;                     // LDS slices per workgroup
        J.n_wgs = J.n_waves;
        return;
    }
    {   // all layers do not fit next to a tile (path G's head): a workgroup per tile, one layer's weights in LDS at a time
        int wmax = 0, bmax = 0;
        for (int l = 0; l < m.n_layers; ++l) {
            const int wf = (m.dims[l] * J.w_ld[l] + 3) & ~3, bf = (m.dims[l + 1] + 3) & ~3;
            wmax = wf > wmax ? wf : wmax;
            bmax = bf > bmax ? bf : bmax;
        }
        if (((size_t)wl + J.wave_floats) * sizeof(float) > (size_t)rgl::kLdsBytesPerCu - 1024 &&
            ((size_t)wmax + bmax + J.wave_floats) * sizeof(float) <= (size_t)rgl::kLdsBytesPerCu - 1024) {
            J.coop = 2;
            for (int l = 0; l < m.n_layers; ++l) { J.w_lds[l] = 0; J.b_lds[l] = wmax; }
            J.weight_floats = wmax + bmax;
            J.waves_per_wg = 1;
            J.n_wgs = J.n_waves;
            return;
        }
    }
    // waves per workgroup: two workgroups per CU when a half of the LDS holds the weights and at least one wave's tile, else one
    // workgroup; 0 = the MLP does not fit this kernel (the caller takes another path)
    const long per_wave = (long)J.wave_floats * (long)sizeof(float), weights = (long)wl * (long)sizeof(float);
    const long lds = (long)rgl::kLdsBytesPerCu - 1024;
    long wpw = (lds / 2 - weights) / per_wave;
    if (wpw < 1) wpw = (lds - weights) / per_wave;
    J.waves_per_wg = wpw < 0 ? 0 : (wpw > 4 ? 4 : (int)wpw);
    J.n_wgs = J.waves_per_wg > 0 ? (J.n_waves + J.waves_per_wg - 1) / J.waves_per_wg : 0;
}
size_t rows_job_lds(const RowsJob& J) { return ((size_t)J.weight_floats + (size_t)J.waves_per_wg * J.wave_floats) * sizeof(float); }

template <class K>
static int launch_rows_kernel(K kernel, RowsArgs& ra, hipStream_t st) {
    size_t lds = 0;
    int wgs = 0;
    for (int j = 0; j < ra.n_jobs; ++j) {
        const size_t b = rows_job_lds(ra.job[j]);
        lds = b > lds ? b : lds;
        ra.job[j].wg_begin = wgs;
        wgs += ra.job[j].n_wgs;
    }
    bool any_coop = false;
    for (int j = 0; j < ra.n_jobs; ++j) any_coop |= ra.job[j].coop != 0;
    return rgl::launch_lds(kernel, dim3(wgs), dim3(ra.job[0].kind >= 10 ? kNarrowWaves * 64 : (any_coop ? kCoopWaves * 64 : 256)), lds, st, ra);
}

// The narrow jobs that share a launch (same kernel kind) get the same number of tiles per wave, chosen so that all their waves are
// resident at once (3 workgroups of kNarrowWaves waves per CU): a launch in one round with 3 tiles per wave beats 2 tiles per wave
// plus a second round for the overflow.
void balance_narrow(RowsJob* const* jobs, int n, int max_waves) {
    for (int j = 0; j < n; ++j) {
        if (!jobs[j] || jobs[j]->kind < 10) continue;
        bool first_of_kind = true;
        long tiles = 0;
        for (int i = 0; i < n; ++i)
            if (jobs[i] && jobs[i]->kind == jobs[j]->kind) {
                if (i < j) first_of_kind = false;
                tiles += jobs[i]->n_tiles;
            }
        if (!first_of_kind) continue;
        long capacity = 256L * 3 * kNarrowWaves;
        capacity = capacity < max_waves ? capacity : max_waves;
        const int per_wave = (int)((tiles + capacity - 1) / capacity);
        for (int i = 0; i < n; ++i)
            if (jobs[i] && jobs[i]->kind == jobs[j]->kind) {
                RowsJob& J = *jobs[i];
                J.n_waves = (J.n_tiles + per_wave - 1) / per_wave;
                J.n_wgs = (J.n_waves + kNarrowWaves - 1) / kNarrowWaves;
            }
    }
}

// the jobs of one pipeline stage: one launch per kernel kind among them
int launch_rows(RowsArgs& all, hipStream_t st) {
    bool done[kMaxRowJobs] = {};
    for (int j = 0; j < all.n_jobs; ++j) {
        if (done[j]) continue;
        RowsArgs ra{};
        ra.backward = all.backward;
        const int kind = all.job[j].kind;
        for (int i = j; i < all.n_jobs; ++i)
            if (!done[i] && all.job[i].kind == kind) { ra.job[ra.n_jobs++] = all.job[i]; done[i] = true; }
        int rc;
        switch (kind) {
            case 11: rc = launch_rows_kernel(mlp2_rows_kernel<1, 1>, ra, st); break;
            case 12: rc = launch_rows_kernel(mlp2_rows_kernel<1, 2>, ra, st); break;
            case 21: rc = launch_rows_kernel(mlp2_rows_kernel<2, 1>, ra, st); break;
            case 22: rc = launch_rows_kernel(mlp2_rows_kernel<2, 2>, ra, st); break;
            case 1: rc = launch_rows_kernel(head_rows_kernel, ra, st); break;
            default: rc = launch_rows_kernel(mlp_rows_kernel, ra, st); break;
        }
        if (rc) return rc;
    }
    return RGL_OK;
}

}  // namespace tiles
}  // namespace rgl

extern "C" int rgl_plan_mlp_rows(const RglMlp* mlp, int n_rows, int max_waves, RglRowsPlan* plan) {
    if (!mlp || !plan) return RGL_ERR_NULL;
    if (n_rows < 1 || max_waves < 1 || mlp->n_layers < 1 || mlp->n_layers > RGL_MAX_MLP_LAYERS) return RGL_ERR_BAD_SHAPE;
    for (int l = 0; l <= mlp->n_layers; ++l)
        if (mlp->dims[l] < 1 || mlp->dims[l] > RGL_MAX_WIDTH) return RGL_ERR_BAD_SHAPE;
    RowsJob J;
    plan_rows_job(J, *mlp, n_rows, max_waves);
    *plan = RglRowsPlan{};
    plan->kind = J.kind; plan->coop = J.coop; plan->waves_per_wg = J.waves_per_wg;
    plan->n_waves = J.n_waves; plan->n_tiles = J.n_tiles; plan->n_wgs = J.n_wgs;
    plan->direct = rows_direct() ? 1 : 0;
    plan->lds_bytes = rows_job_lds(J);
    return RGL_OK;
}

#ifdef RGL_PHASE_TIMING
extern "C" int rgl_debug_read_backward_phase_cycles(unsigned long long* out16, int reset) {
    return rgl::read_phase_cycles(HIP_SYMBOL(g_phase_cycles), out16, reset);
}
#endif
