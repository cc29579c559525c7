// The rotation-consistency filter of U:src/ORBmatcher.cc (HISTO_LENGTH = 30, ComputeThreeMaxima),
// stated once for every matcher: the bin of a pair of keypoint angles, the three bins that
// survive, and the test of a match's bin against them. How a kernel fills its histogram (plain LDS
// atomics, one atomic per distinct bin of a wave, a bin packed into a claim word) stays with it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace orbhip {

constexpr int kHistoLength = 30;

// rot = angle1 - angle2 in [0, 360) -> bin: the reference's lines, in its order and its types
// (a double comparison of the float, the factor formed as 1.0f / HISTO_LENGTH)
__device__ __forceinline__ int rot_bin(float a, float b) {
    float rot = a - b;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / kHistoLength));
    if (bin == kHistoLength) bin = 0;
    return bin;
}

// max over the wave, every lane gets it
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true));   // row_half_mirror
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, true));   // row_mirror
    const auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = max(a[0], a[1]);
    const auto b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return max(b[0], b[1]);
}

// ComputeThreeMaxima over a 30-bin LDS histogram by one wave: keep[0..2] = ind1, ind2, ind3 (-1:
// none). The reference inserts bins in index order with strict '>' into a top-3 that starts at 0,
// so its order is value descending, ties by lower index, positive values only: three wave
// max-reductions of (value << 8 | 255 - i), each winner removed before the next. Then its
// 0.1f * max1 rule. (Counts stay below 2^24: a histogram holds at most 65535 matches.)
// NEEDS A FULL, CONVERGED WAVE: call it from all 64 lanes of one wave (tid < 64 in a work-group of
// at least 64 threads) under a work-group-uniform condition, with a barrier between the last
// histogram update and the call, and one between the call and the first read of keep.
__device__ __forceinline__ void three_maxima_wave(const int* hist, int* keep) {
    const int lane = threadIdx.x & 63;
    const int h = lane < kHistoLength ? hist[lane] : 0;
    uint32_t key = h > 0 ? ((uint32_t)h << 8) | (uint32_t)(255 - lane) : 0u;
    uint32_t k[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        k[j] = wave_max_u32(key);
        if (key == k[j]) key = 0u;
    }
    const int max1 = (int)(k[0] >> 8), max2 = (int)(k[1] >> 8), max3 = (int)(k[2] >> 8);
    int ind1 = k[0] ? 255 - (int)(k[0] & 0xFF) : -1;
    int ind2 = k[1] ? 255 - (int)(k[1] & 0xFF) : -1;
    int ind3 = k[2] ? 255 - (int)(k[2] & 0xFF) : -1;
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
    if (lane == 0) { keep[0] = ind1; keep[1] = ind2; keep[2] = ind3; }
}

// a match whose bin is none of the three kept ones is dropped
__device__ __forceinline__ bool rot_kept(int bin, const int* keep) {
    return bin == keep[0] || bin == keep[1] || bin == keep[2];
}

}  // namespace orbhip
