// numpy's legacy generator (MT19937, np.random.seed / RandomState of an integer seed) for one wave of 64 lanes that keeps the
// 624 state words in LDS: init_genrand seeding, the twist, the tempering and random_sample()'s double.  Shared by the scene
// generator (rgl_scenegen.hip) and the exploration kernels (rgl_explore.hip); tests/scenegen_cpu.py's MT19937 is the plain-integer
// restatement.  `mt` points at 624 words of LDS owned by a workgroup of exactly one wave (the barriers below are the workgroup's).
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int kMtN = 624, kMtM = 397;
constexpr int kWave = 64;

__device__ __forceinline__ unsigned temper(unsigned y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9D2C5680u;
    y ^= (y << 15) & 0xEFC60000u;
    y ^= y >> 18;
    return y;
}

// random_sample() of two successive tempered outputs: every operation exact in float64
__device__ __forceinline__ double to_double(unsigned a, unsigned b) {
#pragma clang fp contract(off)
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

// init_genrand: mt[i] = 1812433253 * (mt[i-1] ^ (mt[i-1] >> 30)) + i.  Sequential; every lane runs it, lane i % 64 stores word i.
__device__ void mt_seed(unsigned* mt, unsigned seed, int lane) {
    unsigned x = seed;
    if (lane == 0) mt[0] = x;
    for (int i = 1; i < kMtN; ++i) {
        x = 1812433253u * (x ^ (x >> 30)) + (unsigned)i;
        if ((i & (kWave - 1)) == lane) mt[i] = x;
    }
    __syncthreads();
}

// The twist, 64 words per pass in ascending order.  Word k needs the OLD words k, k + 1 and (k < 227) k + 397, and (k >= 227) the
// NEW word k - 227, written at least three passes earlier; word 623 needs the new words 0 and 396.  Within a pass every lane's
// store depends on its loads, and the one word a pass reads from the next pass's range (k + 1 of its last lane) is still old.
__device__ void mt_twist(unsigned* mt, int lane) {
    for (int base = 0; base < kMtN; base += kWave) {
        const int k = base + lane;
        unsigned v = 0;
        if (k < kMtN) {
            const unsigned y = (mt[k] & 0x80000000u) | (mt[k + 1 < kMtN ? k + 1 : 0] & 0x7FFFFFFFu);
            v = mt[k + kMtM < kMtN ? k + kMtM : k + kMtM - kMtN] ^ (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
        }
        __syncthreads();
        if (k < kMtN) mt[k] = v;
        __syncthreads();
    }
}

}  // namespace
