// g2o::Sim3 arithmetic on the device, fp64 (U:Thirdparty/g2o/g2o/types/sim3.h), shared by the Sim3
// refinement (sim3_opt.hip) and the essential-graph optimizer (essential_graph.hip). An estimate is
// double[8] = (qx qy qz qw tx ty tz s); nothing here normalises the quaternion. Every operation is
// in the order tests/sim3_opt_numpy.py and tests/essential_graph_numpy.py write it.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_se3.h"

namespace orbhip {

struct S3 {
    DQ q;
    double tx, ty, tz, s;
};

__device__ __forceinline__ S3 s3_load(const double* p) { return S3{DQ{p[0], p[1], p[2], p[3]}, p[4], p[5], p[6], p[7]}; }
__device__ __forceinline__ void s3_store(const S3& a, double* p) {
    p[0] = a.q.x; p[1] = a.q.y; p[2] = a.q.z; p[3] = a.q.w;
    p[4] = a.tx; p[5] = a.ty; p[6] = a.tz; p[7] = a.s;
}

// g2o::Sim3::operator*: (a.r b.r, a.s (a.r b.t) + a.t, a.s b.s); no normalisation
__device__ __forceinline__ S3 s3_mul(const S3& a, const S3& b) {
    S3 r;
    r.q = DQ{a.q.w * b.q.x + a.q.x * b.q.w + a.q.y * b.q.z - a.q.z * b.q.y,
             a.q.w * b.q.y + a.q.y * b.q.w + a.q.z * b.q.x - a.q.x * b.q.z,
             a.q.w * b.q.z + a.q.z * b.q.w + a.q.x * b.q.y - a.q.y * b.q.x,
             a.q.w * b.q.w - a.q.x * b.q.x - a.q.y * b.q.y - a.q.z * b.q.z};
    double x, y, z;
    qrot(a.q, b.tx, b.ty, b.tz, x, y, z);
    r.tx = a.s * x + a.tx; r.ty = a.s * y + a.ty; r.tz = a.s * z + a.tz;
    r.s = a.s * b.s;
    return r;
}

// g2o::Sim3::inverse: (r*, r* ((-1 / s) t), 1 / s)
__device__ __forceinline__ S3 s3_inv(const S3& a) {
    S3 r;
    r.q = DQ{-a.q.x, -a.q.y, -a.q.z, a.q.w};
    const double k = -1.0 / a.s;
    qrot(r.q, k * a.tx, k * a.ty, k * a.tz, r.tx, r.ty, r.tz);
    r.s = 1.0 / a.s;
    return r;
}

// g2o::Sim3(const Vector7d&), u = (omega, upsilon, sigma): the four branches of sim3.h
__device__ __forceinline__ S3 s3_exp(const double* u) {
    const double ox = u[0], oy = u[1], oz = u[2], sigma = u[6];
    const double theta = sqrt(ox * ox + oy * oy + oz * oz);
    const double O[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
    double O2[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) O2[3 * r + c] = O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c];
    const double s = exp(sigma);
    const double eps = 0.00001;
    double A, B, C, ka = 1.0, kb = 1.0;   // R = (I + ka Omega) + kb Omega^2
    const bool small = theta < eps;
    double st = 0.0, ct = 1.0;
    if (!small) {
        sincos(theta, &st, &ct);
        ka = st / theta;
        kb = (1 - ct) / (theta * theta);
    }
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (small) {
            A = 1.0 / 2.0;
            B = 1.0 / 6.0;
        } else {
            const double theta2 = theta * theta;
            A = (1 - ct) / theta2;
            B = (theta - st) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * st, b = s * ct;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2;
        }
    }
    double R[9], Wm[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double id = i % 4 == 0 ? 1.0 : 0.0;
        R[i] = small ? (id + O[i]) + O2[i] : (id + ka * O[i]) + kb * O2[i];
        Wm[i] = (A * O[i] + B * O2[i]) + C * id;
    }
    S3 r;
    r.q = mattoq(R);
    r.tx = Wm[0] * u[3] + Wm[1] * u[4] + Wm[2] * u[5];
    r.ty = Wm[3] * u[3] + Wm[4] * u[4] + Wm[5] * u[5];
    r.tz = Wm[6] * u[3] + Wm[7] * u[4] + Wm[8] * u[5];
    r.s = s;
    return r;
}

// map(X) = s (r X) + t
__device__ __forceinline__ void s3_map(const S3& a, double x, double y, double z, double& ox, double& oy, double& oz) {
    double rx, ry, rz;
    qrot(a.q, x, y, z, rx, ry, rz);
    ox = a.s * rx + a.tx; oy = a.s * ry + a.ty; oz = a.s * rz + a.tz;
}

// g2o::Sim3::log(): out = (omega, upsilon, sigma), the four branches of sim3.h; upsilon =
// W.lu().solve(t) by a 3x3 LU with partial pivoting (the first largest pivot wins)
__device__ __forceinline__ void s3_log(const S3& a, double* out) {
    const double s = a.s, sigma = log(s);
    double R[9];
    qtomat(a.q, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dx = R[7] - R[5], dy = R[2] - R[6], dz = R[3] - R[1];
    const double eps = 0.00001;
    const bool small_s = fabs(sigma) < eps, small_r = d > 1 - eps;
    double A, B, C, ox, oy, oz;
    if (small_r) {
        ox = 0.5 * dx; oy = 0.5 * dy; oz = 0.5 * dz;
        if (small_s) {
            C = 1.0; A = 1.0 / 2.0; B = 1.0 / 6.0;
        } else {
            const double sigma2 = sigma * sigma;
            C = (s - 1) / sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        }
    } else {
        const double theta = acos(d);
        double st, ct;
        sincos(theta, &st, &ct);
        const double k = theta / (2 * sqrt(1 - d * d));
        ox = k * dx; oy = k * dy; oz = k * dz;
        const double theta2 = theta * theta;
        if (small_s) {
            C = 1.0;
            A = (1 - ct) / theta2;
            B = (theta - st) / (theta2 * theta);
        } else {
            C = (s - 1) / sigma;
            const double a_ = s * st, b_ = s * ct, c_ = theta2 + sigma * sigma;
            A = (a_ * sigma + (1 - b_) * theta) / (theta * c_);
            B = (C - ((b_ - 1) * sigma + a_ * theta) / c_) / theta2;
        }
    }
    const double O[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
    double M[3][4];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double o2 = O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c];
            M[r][c] = (A * O[3 * r + c] + B * o2) + C * (r == c ? 1.0 : 0.0);
        }
    M[0][3] = a.tx; M[1][3] = a.ty; M[2][3] = a.tz;
    auto swap_rows = [&](auto I, auto J, bool c) {
        constexpr int i = decltype(I)::value, j = decltype(J)::value;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double t = M[i][k];
            M[i][k] = c ? M[j][k] : t;
            M[j][k] = c ? t : M[j][k];
        }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    {
        const double m0 = fabs(M[0][0]), m1 = fabs(M[1][0]), m2 = fabs(M[2][0]);
        const bool p1 = m1 > m0;
        const bool p2 = m2 > (p1 ? m1 : m0);
        swap_rows(I0{}, I1{}, p1 && !p2);
        swap_rows(I0{}, I2{}, p2);
#pragma unroll
        for (int i = 1; i < 3; i++) {
            const double f = M[i][0] / M[0][0];
#pragma unroll
            for (int c = 1; c < 4; c++) M[i][c] = M[i][c] - f * M[0][c];
        }
    }
    {
        swap_rows(I1{}, I2{}, fabs(M[2][1]) > fabs(M[1][1]));
        const double f = M[2][1] / M[1][1];
        M[2][2] = M[2][2] - f * M[1][2];
        M[2][3] = M[2][3] - f * M[1][3];
    }
    const double x2 = M[2][3] / M[2][2];
    const double x1 = (M[1][3] - M[1][2] * x2) / M[1][1];
    const double x0 = (M[0][3] - M[0][1] * x1 - M[0][2] * x2) / M[0][0];
    out[0] = ox; out[1] = oy; out[2] = oz;
    out[3] = x0; out[4] = x1; out[5] = x2;
    out[6] = sigma;
}

}  // namespace orbhip
