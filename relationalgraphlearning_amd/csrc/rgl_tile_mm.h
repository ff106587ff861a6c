// rgl_tile_mm.h -- device helpers shared by the tile pipeline's two kernel families (rgl_rows.hip, rgl_graph_kernel.h): barriers
// that order LDS only, the fp32 MFMA block product over functor-fetched operands, and a batched gather.
#pragma once
#include "rgl_mfma.h"

namespace {

__device__ __forceinline__ void wave_sync() {         // LDS written by some lanes of the wave, read by others
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup barrier for waves that talk through LDS only: __syncthreads() also waits for every global store of the wave to be
// acknowledged (vmcnt(0): ~2.8 k cycles behind each layer's gradient stores in mlp_rows_kernel), this one orders LDS alone.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// C[MT*16][NTL*16] += A[.][k] B[k][.] over `ksteps` groups of four k: fa(row, k) / fb(k, col) fetch the operand elements
// (LDS or L1-resident weights; the callers clamp / zero what lies outside their matrices).  One A fragment per row tile and one B
// fragment per column tile feed MT*NTL MFMAs.  D row 4 (lane / 16) + r, column lane % 16 is element r of a lane's accumulator.
template <int MT, int NTL, int U, bool PIN, class FA, class FB>
__device__ __forceinline__ void mm_steps(f32x4 (&acc)[MT][NTL], int ks0, FA& fa, FB& fb) {
    const int l16 = threadIdx.x & 15, kk = (threadIdx.x & 63) >> 4;
    float av[U][MT], bv[U][NTL];
#pragma unroll
    for (int u = 0; u < U; ++u) {              // all operand fragments of U k steps in flight, then their MFMAs
        const int k = (ks0 + u) * 4 + kk;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[u][mt] = fa(mt * 16 + l16, k);
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) bv[u][nt] = fb(k, nt * 16 + l16);
    }
    // PIN: every fragment of the batch requested before its first MFMA (left alone, the scheduler sinks the loads to their uses and
    // reuses two registers: an LDS round trip per two k steps -- fine where other waves cover it, not for a workgroup that owns one
    // tile; pinned everywhere, the wide kernels of this file spill)
    if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt) acc[mt][nt] = mfma4(av[u][mt], bv[u][nt], acc[mt][nt]);
    load_fence();            // the next batch's loads stay behind this batch (hoisting them all costs hundreds of VGPRs)
}
template <int MT, int NTL, int U, bool PIN, class FA, class FB>
__device__ __forceinline__ void mm_from(f32x4 (&acc)[MT][NTL], int& ks, int ksteps, FA& fa, FB& fb) {
    for (; ks + U <= ksteps; ks += U) mm_steps<MT, NTL, U, PIN>(acc, ks, fa, fb);
    if constexpr (U > 1) mm_from<MT, NTL, U / 2, PIN>(acc, ks, ksteps, fa, fb);        // the remainder in halving batches
}
template <int MT, int NTL, int UNROLL = 2, bool PIN = false, class FA, class FB>
__device__ __forceinline__ void mm(f32x4 (&acc)[MT][NTL], int ksteps, FA fa, FB fb) {
    int ks = 0;
    mm_from<MT, NTL, UNROLL, PIN>(acc, ks, ksteps, fa, fb);
}
template <int MT, int NTL>
__device__ __forceinline__ void clear(f32x4 (&acc)[MT][NTL]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) acc[mt][nt] = zero4();
}
// f(row, col, value, mt, nt, r) for every element of the block
template <int MT, int NTL, class F>
__device__ __forceinline__ void each(const f32x4 (&acc)[MT][NTL], F f) {
    const int l16 = threadIdx.x & 15, kk = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) f(mt * 16 + 4 * kk + r, nt * 16 + l16, acc[mt][nt][r], mt, nt, r);
}

// dst(idx, src(idx)) for idx = t0, t0 + step, .. < n, the loads U at a time (a plain loop pays one global-memory latency per
// iteration: the compiler does not pipeline across iterations)
template <int U, class Src, class Dst>
__device__ __forceinline__ void gather(int n, int t0, int step, Src src, Dst dst) {
    for (int base = t0; base < n; base += U * step) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = base + u * step;
            v[u] = idx < n ? src(idx) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = base + u * step;
            if (idx < n) dst(idx, v[u]);
        }
    }
}

}  // namespace
