// The 4x4 one-sided Jacobi of the triangulations (CreateNewMapPoints' k_tri_points and
// TwoViewReconstruction's CheckRT): fp64, held in registers, every index a constant.
#pragma once
#include <hip/hip_runtime.h>

namespace orbhip {

// one rotation of the one-sided Jacobi on the columns (P, Q) of U (4x4, row-major), applied to V too
template <int P, int Q>
__device__ __forceinline__ void tri_jacobi_pair(double (&U)[16], double (&V)[16]) {
    const double a = ((U[P] * U[P] + U[4 + P] * U[4 + P]) + U[8 + P] * U[8 + P]) + U[12 + P] * U[12 + P];
    const double b = ((U[Q] * U[Q] + U[4 + Q] * U[4 + Q]) + U[8 + Q] * U[8 + Q]) + U[12 + Q] * U[12 + Q];
    const double g = ((U[P] * U[Q] + U[4 + P] * U[4 + Q]) + U[8 + P] * U[8 + Q]) + U[12 + P] * U[12 + Q];
    if (g == 0.0) return;
    const double zeta = (b - a) / (2.0 * g);
    double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    if (zeta < 0.0) t = -t;
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double x = U[4 * i + P], y = U[4 * i + Q];
        U[4 * i + P] = c * x - s * y;
        U[4 * i + Q] = s * x + c * y;
        const double vx = V[4 * i + P], vy = V[4 * i + Q];
        V[4 * i + P] = c * vx - s * vy;
        V[4 * i + Q] = s * vx + c * vy;
    }
}

}  // namespace orbhip
