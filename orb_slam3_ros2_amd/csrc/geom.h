// The fp32 geometry and descriptor helpers that the projection, Fuse, Sim3, triangulation, BoW
// and brute-force kernels (and the host code that prepares their constants) share. Every
// operation is in the order written (no FMA: -ffp-contract=off), so host and device agree bit
// for bit with Eigen's float code in the reference.
#pragma once
#include <hip/hip_runtime.h>

namespace orbhip {

// Eigen QuaternionBase::_transformVector, float; q = (x, y, z, w)
__host__ __device__ __forceinline__ void quat_rotate(const float q[4], const float v[3], float o[3]) {
    float uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    const float c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    o[0] = v[0] + q[3] * uv[0] + c[0];
    o[1] = v[1] + q[3] * uv[1] + c[1];
    o[2] = v[2] + q[3] * uv[2] + c[2];
}

// Eigen QuaternionBase::toRotationMatrix, float, row-major
__host__ __device__ __forceinline__ void quat_to_matrix(const float q[4], float R[9]) {
    const float tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const float twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const float txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const float tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// The frame grid of Frame / KeyFrame (FRAME_GRID_COLS x FRAME_GRID_ROWS)
constexpr int kGridCols = 64, kGridRows = 48, kGridCells = kGridCols * kGridRows;

// PosInGrid: cell = px * 48 + py, `outside` (-1; 0xFFFF where the cell is kept in 16 bits) off the
// grid; invw = 64 / (maxx - minx), invh = 48 / (maxy - miny)
__device__ __forceinline__ int grid_cell(float minx, float miny, float invw, float invh, float x, float y,
                                         int outside = -1) {
    const int px = (int)roundf((x - minx) * invw);
    const int py = (int)roundf((y - miny) * invh);
    return (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) ? outside : px * kGridRows + py;
}

// MapPoint::PredictScale: ceil(log(ratio) / mfLogScaleFactor) clamped to [0, n_levels - 1], the one
// definition of isInFrustum's and Fuse's level. The reference takes the logarithm from the host's
// libm, and the device's logf differs from it in the last bit often enough to move the ceiling at a
// few ratios next to a step (1 of the 33 554 432 floats in [0.5, 8) at 1.2 / 8 levels, 3 next to the
// powers of two at 2.0 / 8 levels), so the device takes no logarithm: the level is monotone in the
// ratio, the host finds the smallest float ratio of every level with its own log (level_thresholds,
// stage.h) and the device counts the steps at or below the ratio. The first kStepArgs steps travel in
// the kernel arguments (LevelSteps: scalar registers, no memory round trip before the level is
// known; NaN beyond n_levels, which no ratio reaches), the steps of a deeper pyramid are read from
// thr: n_levels floats behind the scale factors of the call's block, thr[0] unused.
// orbhip_test_predict_scale_sweep compares this function with the host's level over float ranges.
constexpr int kStepArgs = 16;
struct LevelSteps { float thr[kStepArgs]; };
__device__ __forceinline__ int predict_scale(float ratio, const LevelSteps& steps, const float* __restrict__ thr,
                                             int n_levels) {
    int lvl = 0;
#pragma unroll
    for (int k = 1; k < kStepArgs; k++) lvl += ratio >= steps.thr[k] ? 1 : 0;
    for (int k = kStepArgs; k < n_levels; k++) lvl += ratio >= thr[k] ? 1 : 0;
    return lvl;
}

// Hamming distance of the 256-bit descriptors (a, b) and (c, d)
__device__ __forceinline__ int hamming256(uint4 a, uint4 b, uint4 c, uint4 d) {
    return __popc(a.x ^ c.x) + __popc(a.y ^ c.y) + __popc(a.z ^ c.z) + __popc(a.w ^ c.w) + __popc(b.x ^ d.x) +
           __popc(b.y ^ d.y) + __popc(b.z ^ d.z) + __popc(b.w ^ d.w);
}

}  // namespace orbhip
