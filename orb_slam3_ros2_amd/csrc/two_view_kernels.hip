// gfx950 TwoViewReconstruction (Tracking::MonocularInitialization): both RANSACs, the model choice,
// the motion hypotheses and their CheckRT for every frame pair of a call (DESIGN.md
// "TwoViewReconstruction"):
//   tv_normalize     host, fp32, upstream's running sums: Normalize of both frames, once per problem
//   k_tvr_ransac     one wavefront per (problem, hypothesis, model), four per work-group. The 9x9 Gram
//                    matrix of the hypothesis' DLT system is formed in fp64 and held by every lane
//                    (45 doubles, every index a constant); the rows of the eigenvector matrix are
//                    dealt to the lanes (lane r holds row r: 9 doubles), so a rotation of the
//                    two-sided cyclic Jacobi updates two of a lane's values. The null vector is then
//                    gathered by nine lane reads. The wave walks the matches in 64s: a ballot per
//                    step is one word of the inlier mask, the score terms are added in fp64 (exact,
//                    so order-free) and rounded once
//   k_tvr_select     one work-group per problem: the first maximum of each model's scores, RH, the
//                    masks as bytes, and (one lane) the 4 or 8 motion hypotheses by fp64 3x3 Jacobi SVDs
//   k_tvr_check_rt   one work-group per (problem, motion hypothesis): triangulation and CheckRT's
//                    gates per inlier match, the count, and the k-th smallest cosine by counting
//   k_tvr_final      one work-group per problem: upstream's acceptance rule and the outputs
// No work-group waits for another; the four launches are ordered by the stream.
#include <hip/hip_runtime.h>

#include <cmath>

#include "jacobi4.h"
#include "orbhip_device.h"
#include "orbhip_kernels.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" two view", x)

namespace orbhip {

constexpr int kTvMaxN = 8192;      // matches per problem
constexpr int kTvMaxHyp = 4096;    // hypotheses per model and problem
// Jacobi sweeps: the measured need + 1 (tests/test_two_view.py: 8 for the 9x9 null vector, 4 for
// the 3x3 SVDs over the scene set)
constexpr int kTvSweeps9 = 9;
constexpr int kTvSweeps3 = 5;
constexpr int kTvSweeps4 = 6;      // the triangulation, as CreateNewMapPoints
constexpr int kTvWaves = 4;        // hypotheses per work-group
constexpr int kTvThreads = 256;    // select, CheckRT, final
constexpr int kTvHead = 64;        // words of a problem's head
// head: [success model best_h best_f | SH SF | H21 9 | F21 9 | R21 9 | t21 3 | n_good 8 | parallax 8 |
//        cos_sel 8 | chosen n_mot n_inl]
enum { kHdSuccess = 0, kHdModel, kHdBestH, kHdBestF, kHdSH, kHdSF, kHdH21, kHdF21 = kHdH21 + 9, kHdR21 = kHdF21 + 9,
       kHdT21 = kHdR21 + 9, kHdGood = kHdT21 + 3, kHdPar = kHdGood + 8, kHdCos = kHdPar + 8, kHdChosen = kHdCos + 8,
       kHdMot, kHdInl };
static_assert(kHdInl < kTvHead, "the head holds every scalar output");

struct TvDev {                       // one problem in the call's staging block (device pointers)
    const float *x1, *y1, *x2, *y2;      // n each: the matches' keypoints
    const float *xn1, *yn1, *xn2, *yn2;  // normalised
    const int32_t* sets;                 // H x 8
    float* score;                        // 2 x H: model 0 (H), then model 1 (F)
    float* mat;                          // 2 x H x 9: H21 / F21
    unsigned long long* mask;            // 2 x H x words
    int32_t* head;                       // kTvHead words
    float* mot;                          // 8 x 12: (R row-major, t)
    uint8_t* inl;                        // 3 x n: best H mask, best F mask, the chosen model's
    uint8_t* good;                       // 8 x n: 0 not counted, 1 counted, 3 counted and vbGood
    float* p3d;                          // 8 x n x 3
    float* out_p3d;                      // n x 3
    uint8_t* out_tri;                    // n
    float T1[9], T2inv[9], T2t[9], K[4];
    float inv_sigma2, th2;
    int n, H, words, pad;
};

// ---- fp32 3x3 helpers, every operation in the order written ----
__device__ __forceinline__ void tv_mm3(const float* A, const float* B, float* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ float tv_det3(const float* M) {
    const float c0 = M[4] * M[8] - M[5] * M[7], c1 = M[5] * M[6] - M[3] * M[8], c2 = M[3] * M[7] - M[4] * M[6];
    return (M[0] * c0 + M[1] * c1) + M[2] * c2;
}
// the adjugate over the determinant (first-row expansion); a singular M gives inf / NaN
__device__ __forceinline__ void tv_inv3(const float* M, float* I) {
    const float c0 = M[4] * M[8] - M[5] * M[7], c1 = M[5] * M[6] - M[3] * M[8], c2 = M[3] * M[7] - M[4] * M[6];
    const float det = (M[0] * c0 + M[1] * c1) + M[2] * c2;
    const float d = 1.0f / det;
    I[0] = c0 * d;
    I[1] = (M[2] * M[7] - M[1] * M[8]) * d;
    I[2] = (M[1] * M[5] - M[2] * M[4]) * d;
    I[3] = c1 * d;
    I[4] = (M[0] * M[8] - M[2] * M[6]) * d;
    I[5] = (M[2] * M[3] - M[0] * M[5]) * d;
    I[6] = c2 * d;
    I[7] = (M[1] * M[6] - M[0] * M[7]) * d;
    I[8] = (M[0] * M[4] - M[1] * M[3]) * d;
}
__device__ __forceinline__ void tv_transpose(const float* M, float* T) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) T[3 * i + j] = M[3 * j + i];
}

// ---- the 9x9 null vector ----
// one rotation of the two-sided Jacobi on the symmetric A (9x9, the upper triangle is kept:
// A[9 r + c], r <= c; the same in every lane); Vr is this lane's row of the eigenvector matrix.
// The rotation is sim3_jacobi_pair's
template <int P, int Q>
__device__ __forceinline__ void tv_jacobi9_pair(double (&A)[81], double (&Vr)[9]) {
    const double g = A[9 * P + Q];
    if (g == 0.0) return;
    const double zeta = (A[10 * Q] - A[10 * P]) / (2.0 * g);
    double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    if (zeta < 0.0) t = -t;
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    A[10 * P] = A[10 * P] - t * g;
    A[10 * Q] = A[10 * Q] + t * g;
    A[9 * P + Q] = 0.0;
#pragma unroll
    for (int r = 0; r < 9; r++) {
        if (r != P && r != Q) {
            const int ip = r < P ? 9 * r + P : 9 * P + r, iq = r < Q ? 9 * r + Q : 9 * Q + r;
            const double x = A[ip], y = A[iq];
            A[ip] = c * x - s * y;
            A[iq] = s * x + c * y;
        }
    }
    const double vx = Vr[P], vy = Vr[Q];
    Vr[P] = c * vx - s * vy;
    Vr[Q] = s * vx + c * vy;
}
// the 36 pairs of a sweep in the order (0,1), (0,2), ..., (7,8)
template <int P, int Q>
__device__ __forceinline__ void tv_sweep9(double (&A)[81], double (&Vr)[9]) {
    tv_jacobi9_pair<P, Q>(A, Vr);
    if constexpr (Q < 8) tv_sweep9<P, Q + 1>(A, Vr);
    else if constexpr (P < 7) tv_sweep9<P + 1, P + 2>(A, Vr);
}
// A = A + a a^T (upper triangle), the products exact in fp64
__device__ __forceinline__ void tv_gram_row(double (&A)[81], const float (&a)[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = i; j < 9; j++) A[9 * i + j] = A[9 * i + j] + (double)a[i] * (double)a[j];
}
// the eigenvector of the smallest eigenvalue (the lowest column among equals), in every lane, as fp32
__device__ __forceinline__ void tv_null_vector(double (&A)[81], int lane, float (&v)[9]) {
    double Vr[9];
#pragma unroll
    for (int j = 0; j < 9; j++) Vr[j] = j == lane ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kTvSweeps9; sweep++) tv_sweep9<0, 1>(A, Vr);
    double best = A[0], mine = Vr[0];
#pragma unroll
    for (int k = 1; k < 9; k++)
        if (A[10 * k] < best) { best = A[10 * k]; mine = Vr[k]; }
#pragma unroll
    for (int j = 0; j < 9; j++) v[j] = (float)__shfl(mine, j);
}

// ---- the 3x3 SVD (fp64 one-sided Jacobi, tri_jacobi_pair's rotation) ----
template <int P, int Q>
__device__ __forceinline__ void tv_jacobi3_pair(double (&U)[9], double (&W)[9]) {
    const double a = (U[P] * U[P] + U[3 + P] * U[3 + P]) + U[6 + P] * U[6 + P];
    const double b = (U[Q] * U[Q] + U[3 + Q] * U[3 + Q]) + U[6 + Q] * U[6 + Q];
    const double g = (U[P] * U[Q] + U[3 + P] * U[3 + Q]) + U[6 + P] * U[6 + Q];
    if (g == 0.0) return;
    const double zeta = (b - a) / (2.0 * g);
    double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    if (zeta < 0.0) t = -t;
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double x = U[3 * i + P], y = U[3 * i + Q];
        U[3 * i + P] = c * x - s * y;
        U[3 * i + Q] = s * x + c * y;
        const double vx = W[3 * i + P], vy = W[3 * i + Q];
        W[3 * i + P] = c * vx - s * vy;
        W[3 * i + Q] = s * vx + c * vy;
    }
}
__device__ __forceinline__ double tv_col(const double (&M)[9], int r, int k) {
    return k == 0 ? M[3 * r] : k == 1 ? M[3 * r + 1] : M[3 * r + 2];
}
// M = Q diag(sig) W^T: W's columns are the accumulated rotations in the order of descending
// column norm of C = M W (the first of equals first, the last of equals last), sig the norms, Q's
// first two columns the normalised columns of C, its third their cross product with the sign of
// its product with C's third column
struct TvSvd3 { double Q[9], sig[3], W[9], C[9]; };
__device__ __forceinline__ void tv_svd3(const double (&M)[9], TvSvd3& o) {
    double U[9], W[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { U[i] = M[i]; W[i] = (i % 4 == 0) ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < kTvSweeps3; sweep++) {
        tv_jacobi3_pair<0, 1>(U, W);
        tv_jacobi3_pair<0, 2>(U, W);
        tv_jacobi3_pair<1, 2>(U, W);
    }
    double n[3];
#pragma unroll
    for (int k = 0; k < 3; k++) n[k] = (U[k] * U[k] + U[3 + k] * U[3 + k]) + U[6 + k] * U[6 + k];
    int i0 = 0, i2 = 0;
    double best = n[0];
#pragma unroll
    for (int k = 1; k < 3; k++)
        if (n[k] > best) { best = n[k]; i0 = k; }
    best = n[0];
#pragma unroll
    for (int k = 1; k < 3; k++)
        if (n[k] <= best) { best = n[k]; i2 = k; }
    if (i0 == i2) { i0 = 0; i2 = 2; }
    const int idx[3] = {i0, 3 - i0 - i2, i2};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double nk = idx[k] == 0 ? n[0] : idx[k] == 1 ? n[1] : n[2];
        o.sig[k] = sqrt(nk);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            o.C[3 * r + k] = tv_col(U, r, idx[k]);
            o.W[3 * r + k] = tv_col(W, r, idx[k]);
        }
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        o.Q[3 * r] = o.C[3 * r] / o.sig[0];
        o.Q[3 * r + 1] = o.C[3 * r + 1] / o.sig[1];
    }
    double q2[3] = {o.Q[3] * o.Q[7] - o.Q[6] * o.Q[4], o.Q[6] * o.Q[1] - o.Q[0] * o.Q[7], o.Q[0] * o.Q[4] - o.Q[3] * o.Q[1]};
    const double dot = (q2[0] * o.C[2] + q2[1] * o.C[5]) + q2[2] * o.C[8];
#pragma unroll
    for (int r = 0; r < 3; r++) o.Q[3 * r + 2] = dot < 0.0 ? -q2[r] : q2[r];
}

// ---- k_tvr_ransac ----
__global__ __launch_bounds__(64 * kTvWaves) void k_tvr_ransac(const TvDev* __restrict__ probs) {
    const int lane = threadIdx.x & 63;
    const int wv = blockIdx.x * kTvWaves + (threadIdx.x >> 6);   // wave-uniform
    const int h = wv >> 1, model = wv & 1;
    const TvDev& P = probs[blockIdx.y];
    if (h >= P.H) return;
    const int n = P.n;
    const int32_t* __restrict__ set = P.sets + 8 * h;
    double A[81];
#pragma unroll
    for (int i = 0; i < 81; i++) A[i] = 0.0;
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        const int i = set[k];
        const float u1 = P.xn1[i], v1 = P.yn1[i], u2 = P.xn2[i], v2 = P.yn2[i];
        if (model == 0) {
            const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
            const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -(u2 * u1), -(u2 * v1), -u2};
            tv_gram_row(A, r0);
            tv_gram_row(A, r1);
        } else {
            const float r0[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
            tv_gram_row(A, r0);
        }
    }
    float v[9];
    tv_null_vector(A, lane, v);
    float M[9], Mi[9], tmp[9];   // H21 and H12, or F21
    if (model == 0) {
        tv_mm3(P.T2inv, v, tmp);
        tv_mm3(tmp, P.T1, M);
        tv_inv3(M, Mi);
    } else {
        double Fd[9];
#pragma unroll
        for (int i = 0; i < 9; i++) Fd[i] = (double)v[i];
        TvSvd3 sv;
        tv_svd3(Fd, sv);
        float Fn[9];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++)
                Fn[3 * r + c] = (float)(sv.C[3 * r] * sv.W[3 * c] + sv.C[3 * r + 1] * sv.W[3 * c + 1]);
        tv_mm3(P.T2t, Fn, tmp);
        tv_mm3(tmp, P.T1, M);
#pragma unroll
        for (int i = 0; i < 9; i++) Mi[i] = 0.f;
    }
    const size_t slot = (size_t)model * P.H + h;
    unsigned long long* __restrict__ mask = P.mask + slot * P.words;
    const float isg = P.inv_sigma2;
    const float thH = 5.991f, thF = 3.841f, thScore = 5.991f;
    double acc = 0.0;
    for (int i0 = 0, w = 0; i0 < n; i0 += 64, w++) {
        const int i = i0 + lane;
        bool in = false;
        if (i < n) {
            const float u1 = P.x1[i], v1 = P.y1[i], u2 = P.x2[i], v2 = P.y2[i];
            float chi1, chi2, t1, t2;
            if (model == 0) {
                float w2 = 1.0f / ((Mi[6] * u2 + Mi[7] * v2) + Mi[8]);
                float a = ((Mi[0] * u2 + Mi[1] * v2) + Mi[2]) * w2, b = ((Mi[3] * u2 + Mi[4] * v2) + Mi[5]) * w2;
                chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * isg;
                w2 = 1.0f / ((M[6] * u1 + M[7] * v1) + M[8]);
                a = ((M[0] * u1 + M[1] * v1) + M[2]) * w2;
                b = ((M[3] * u1 + M[4] * v1) + M[5]) * w2;
                chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * isg;
                t1 = chi1 > thH ? 0.f : thH - chi1;
                t2 = chi2 > thH ? 0.f : thH - chi2;
                in = !(chi1 > thH) && !(chi2 > thH);
            } else {
                const float a2 = (M[0] * u1 + M[1] * v1) + M[2], b2 = (M[3] * u1 + M[4] * v1) + M[5];
                const float c2 = (M[6] * u1 + M[7] * v1) + M[8];
                const float num2 = (a2 * u2 + b2 * v2) + c2;
                chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * isg;
                const float a1 = (M[0] * u2 + M[3] * v2) + M[6], b1 = (M[1] * u2 + M[4] * v2) + M[7];
                const float c1 = (M[2] * u2 + M[5] * v2) + M[8];
                const float num1 = (a1 * u1 + b1 * v1) + c1;
                chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * isg;
                t1 = chi1 > thF ? 0.f : thScore - chi1;
                t2 = chi2 > thF ? 0.f : thScore - chi2;
                in = !(chi1 > thF) && !(chi2 > thF);
            }
            acc += (double)t1;
            acc += (double)t2;
        }
        const unsigned long long m = __ballot(in);
        if (lane == 0) mask[w] = m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
        P.score[slot] = (float)acc;
#pragma unroll
        for (int i = 0; i < 9; i++) P.mat[slot * 9 + i] = M[i];
    }
}

// ---- k_tvr_select ----
// ReconstructF's four (R, t): E21 = K^T F21 K, DecomposeE
__device__ void tv_motions_f(const float* F21, const float* K, float* mot) {
    const float Km[9] = {K[0], 0.f, K[2], 0.f, K[1], K[3], 0.f, 0.f, 1.f};
    float Kt[9], tmp[9], E[9];
    tv_transpose(Km, Kt);
    tv_mm3(Kt, F21, tmp);
    tv_mm3(tmp, Km, E);
    double Et[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Et[3 * i + j] = (double)E[3 * j + i];
    TvSvd3 sv;   // E^T = Q sig W^T: U of E = W, V of E = Q
    tv_svd3(Et, sv);
    float U[9], V[9], Vt[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { U[i] = (float)sv.W[i]; V[i] = (float)sv.Q[i]; }
    tv_transpose(V, Vt);
    const float tn = sqrtf((U[2] * U[2] + U[5] * U[5]) + U[8] * U[8]);
    const float t[3] = {U[2] / tn, U[5] / tn, U[8] / tn};
    const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float Wt[9], R1[9], R2[9];
    tv_transpose(Wm, Wt);
    tv_mm3(U, Wm, tmp);
    tv_mm3(tmp, Vt, R1);
    if (tv_det3(R1) < 0.f)
#pragma unroll
        for (int i = 0; i < 9; i++) R1[i] = -R1[i];
    tv_mm3(U, Wt, tmp);
    tv_mm3(tmp, Vt, R2);
    if (tv_det3(R2) < 0.f)
#pragma unroll
        for (int i = 0; i < 9; i++) R2[i] = -R2[i];
#pragma unroll
    for (int m = 0; m < 4; m++) {
#pragma unroll
        for (int i = 0; i < 9; i++) mot[12 * m + i] = (m & 1) ? R2[i] : R1[i];
#pragma unroll
        for (int i = 0; i < 3; i++) mot[12 * m + 9 + i] = m < 2 ? t[i] : -t[i];
    }
}

// ReconstructH's eight (R, t) in upstream's order; 0 at the d1/d2, d2/d3 exit
__device__ int tv_motions_h(const float* H21, const float* K, float* mot) {
    const float Km[9] = {K[0], 0.f, K[2], 0.f, K[1], K[3], 0.f, 0.f, 1.f};
    const float Ki[9] = {1.0f / K[0], 0.f, (-K[2]) / K[0], 0.f, 1.0f / K[1], (-K[3]) / K[1], 0.f, 0.f, 1.f};
    float tmp[9], A[9];
    tv_mm3(Ki, H21, tmp);
    tv_mm3(tmp, Km, A);
    double Ad[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Ad[i] = (double)A[i];
    TvSvd3 sv;
    tv_svd3(Ad, sv);
    float U[9], V[9], Vt[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { U[i] = (float)sv.Q[i]; V[i] = (float)sv.W[i]; }
    tv_transpose(V, Vt);
    const float d1 = (float)sv.sig[0], d2 = (float)sv.sig[1], d3 = (float)sv.sig[2];
    const float s = tv_det3(U) * tv_det3(Vt);
    if (d1 / d2 < 1.00001f || d2 / d3 < 1.00001f) return 0;
    const float den = d1 * d1 - d3 * d3;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / den), aux3 = sqrtf((d2 * d2 - d3 * d3) / den);
    const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
    const float prod = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3));
    const float ast = prod / ((d1 + d3) * d2), ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float asp = prod / ((d1 - d3) * d2), cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sgn[4] = {1.f, -1.f, -1.f, 1.f};
    float sU[9];
#pragma unroll
    for (int i = 0; i < 9; i++) sU[i] = s * U[i];
#pragma unroll 1
    for (int m = 0; m < 8; m++) {
        const int i = m & 3;
        const bool neg = m >= 4;   // the case d' = -d2
        const float sn = sgn[i] < 0.f ? -(neg ? asp : ast) : (neg ? asp : ast);
        const float Rp[9] = {neg ? cp : ct, 0.f, neg ? sn : -sn, 0.f, neg ? -1.f : 1.f, 0.f, sn, 0.f, neg ? -cp : ct};
        float R[9];
        tv_mm3(sU, Rp, tmp);
        tv_mm3(tmp, Vt, R);
        const float dd = neg ? d1 + d3 : d1 - d3;
        const float tp[3] = {x1[i] * dd, 0.f, (neg ? x3[i] : -x3[i]) * dd};
        float t[3];
#pragma unroll
        for (int r = 0; r < 3; r++) t[r] = (U[3 * r] * tp[0] + U[3 * r + 1] * tp[1]) + U[3 * r + 2] * tp[2];
        const float tn = sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
#pragma unroll
        for (int r = 0; r < 9; r++) mot[12 * m + r] = R[r];
#pragma unroll
        for (int r = 0; r < 3; r++) mot[12 * m + 9 + r] = t[r] / tn;
    }
    return 8;
}

__global__ __launch_bounds__(kTvThreads) void k_tvr_select(const TvDev* __restrict__ probs) {
    __shared__ unsigned long long s_key[2][kTvThreads / 64];
    __shared__ int s_best[2], s_model, s_inl;
    const TvDev& P = probs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) s_inl = 0;
    // the first maximum above 0: the largest (score bits, -h); a NaN or a score <= 0 never enters
    unsigned long long key[2] = {0ull, 0ull};
    for (int h = tid; h < P.H; h += kTvThreads)
#pragma unroll
        for (int m = 0; m < 2; m++) {
            const float s = P.score[(size_t)m * P.H + h];
            if (s > 0.0f) {
                const unsigned long long k = ((unsigned long long)__float_as_uint(s) << 32) | (0xFFFFFFFFu - (unsigned)h);
                key[m] = k > key[m] ? k : key[m];
            }
        }
#pragma unroll
    for (int m = 0; m < 2; m++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key[m], o);
            key[m] = other > key[m] ? other : key[m];
        }
        if (lane == 0) s_key[m][wid] = key[m];
    }
    __syncthreads();
    if (tid == 0) {
        int best[2];
        float S[2];
#pragma unroll
        for (int m = 0; m < 2; m++) {
            unsigned long long k = s_key[m][0];
            for (int w = 1; w < kTvThreads / 64; w++) k = s_key[m][w] > k ? s_key[m][w] : k;
            best[m] = k ? (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)) : -1;
            S[m] = k ? __uint_as_float((unsigned)(k >> 32)) : 0.0f;
            s_best[m] = best[m];
        }
        float* hf = (float*)P.head;
        P.head[kHdSuccess] = 0;
        P.head[kHdBestH] = best[0];
        P.head[kHdBestF] = best[1];
        hf[kHdSH] = S[0];
        hf[kHdSF] = S[1];
        for (int i = 0; i < 9; i++) {
            hf[kHdH21 + i] = best[0] >= 0 ? P.mat[(size_t)best[0] * 9 + i] : 0.f;
            hf[kHdF21 + i] = best[1] >= 0 ? P.mat[((size_t)P.H + best[1]) * 9 + i] : 0.f;
            hf[kHdR21 + i] = 0.f;
        }
        for (int i = 0; i < 3; i++) hf[kHdT21 + i] = 0.f;
        for (int i = 0; i < 8; i++) { P.head[kHdGood + i] = 0; hf[kHdPar + i] = 0.f; hf[kHdCos + i] = 0.f; }
        P.head[kHdChosen] = -1;
        int model = -1, n_mot = 0;
        if (S[0] + S[1] != 0.0f) {
            const float RH = S[0] / (S[0] + S[1]);
            if (RH > 0.50f) {
                model = 0;
                n_mot = tv_motions_h(hf + kHdH21, P.K, P.mot);
            } else {
                model = 1;
                tv_motions_f(hf + kHdF21, P.K, P.mot);
                n_mot = 4;
            }
        }
        P.head[kHdModel] = model;
        P.head[kHdMot] = n_mot;
        s_model = model;
    }
    __syncthreads();
    const int model = s_model;
    const unsigned long long* mh = s_best[0] >= 0 ? P.mask + (size_t)s_best[0] * P.words : nullptr;
    const unsigned long long* mf = s_best[1] >= 0 ? P.mask + ((size_t)P.H + s_best[1]) * P.words : nullptr;
    int cnt = 0;
    for (int i = tid; i < P.n; i += kTvThreads) {
        const uint8_t a = mh ? (uint8_t)((mh[i >> 6] >> (i & 63)) & 1ull) : 0;
        const uint8_t b = mf ? (uint8_t)((mf[i >> 6] >> (i & 63)) & 1ull) : 0;
        const uint8_t c = model == 0 ? a : model == 1 ? b : 0;
        P.inl[i] = a;
        P.inl[P.n + i] = b;
        P.inl[2 * (size_t)P.n + i] = c;
        cnt += c;
    }
    cnt = wave_sum_i32(cnt);
    if (lane == 0 && cnt) atomicAdd(&s_inl, cnt);   // a count: the same whatever the order
    __syncthreads();
    if (tid == 0) P.head[kHdInl] = s_inl;
}

// ---- k_tvr_check_rt ----
// a float as an unsigned key of the same order, and back
__device__ __forceinline__ unsigned tv_order_key(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float tv_order_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__global__ __launch_bounds__(kTvThreads) void k_tvr_check_rt(const TvDev* __restrict__ probs) {
    __shared__ float s_cos[kTvMaxN];
    __shared__ int s_good, s_cnt[32];
    __shared__ float s_sel;
    const TvDev& P = probs[blockIdx.y];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, n = P.n;
    if (m >= P.head[kHdMot]) return;   // uniform over the work-group
    if (tid == 0) { s_good = 0; s_sel = 0.f; }
    if (tid < 32) s_cnt[tid] = 0;
    __syncthreads();
    const float* __restrict__ mot = P.mot + 12 * m;
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = mot[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = mot[9 + i];
    const float fx = P.K[0], fy = P.K[1], cx = P.K[2], cy = P.K[3], th2 = P.th2;
    const float P1[12] = {fx, 0.f, cx, 0.f, 0.f, fy, cy, 0.f, 0.f, 0.f, 1.f, 0.f};
    float P2[12], O2[3];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float r0 = j < 3 ? R[j] : t[0], r1 = j < 3 ? R[3 + j] : t[1], r2 = j < 3 ? R[6 + j] : t[2];
        P2[j] = fx * r0 + cx * r2;
        P2[4 + j] = fy * r1 + cy * r2;
        P2[8 + j] = r2;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) O2[i] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
    const uint8_t* __restrict__ inl = P.inl + 2 * (size_t)n;
    uint8_t* __restrict__ good = P.good + (size_t)m * n;
    float* __restrict__ p3d = P.p3d + (size_t)m * n * 3;
    const float kCos = 0.99998f;
    for (int i0 = 0; i0 < n; i0 += kTvThreads) {
        const int i = i0 + tid;
        int flag = 0;
        float cosp = 0.f, x = 0.f, y = 0.f, z = 0.f;
        if (i < n && inl[i]) {
            const float u1 = P.x1[i], v1 = P.y1[i], u2 = P.x2[i], v2 = P.y2[i];
            double U[16], V[16];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                U[j] = (double)(u1 * P1[8 + j] - P1[j]);
                U[4 + j] = (double)(v1 * P1[8 + j] - P1[4 + j]);
                U[8 + j] = (double)(u2 * P2[8 + j] - P2[j]);
                U[12 + j] = (double)(v2 * P2[8 + j] - P2[4 + j]);
            }
#pragma unroll
            for (int k = 0; k < 16; k++) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
#pragma unroll 1
            for (int sweep = 0; sweep < kTvSweeps4; sweep++) {
                tri_jacobi_pair<0, 1>(U, V);
                tri_jacobi_pair<0, 2>(U, V);
                tri_jacobi_pair<0, 3>(U, V);
                tri_jacobi_pair<1, 2>(U, V);
                tri_jacobi_pair<1, 3>(U, V);
                tri_jacobi_pair<2, 3>(U, V);
            }
            double best = ((U[0] * U[0] + U[4] * U[4]) + U[8] * U[8]) + U[12] * U[12];
            double v0 = V[0], v1d = V[4], v2d = V[8], v3 = V[12];
#pragma unroll
            for (int k = 1; k < 4; k++) {
                const double nk = ((U[k] * U[k] + U[4 + k] * U[4 + k]) + U[8 + k] * U[8 + k]) + U[12 + k] * U[12 + k];
                if (nk < best) { best = nk; v0 = V[k]; v1d = V[4 + k]; v2d = V[8 + k]; v3 = V[12 + k]; }
            }
            x = (float)(v0 / v3); y = (float)(v1d / v3); z = (float)(v2d / v3);
            bool ok = isfinite(x) && isfinite(y) && isfinite(z);
            const float d1 = sqrtf((x * x + y * y) + z * z);
            const float nx = x - O2[0], ny = y - O2[1], nz = z - O2[2];
            const float d2 = sqrtf((nx * nx + ny * ny) + nz * nz);
            const float c = ((x * nx + y * ny) + z * nz) / (d1 * d2);
            if (z <= 0.f && c < kCos) ok = false;
            const float X2 = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
            const float Y2 = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
            const float Z2 = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
            if (Z2 <= 0.f && c < kCos) ok = false;
            float iz = 1.0f / z;
            float ex = ((fx * x) * iz + cx) - u1, ey = ((fy * y) * iz + cy) - v1;
            if ((ex * ex + ey * ey) > th2) ok = false;
            iz = 1.0f / Z2;
            ex = ((fx * X2) * iz + cx) - u2;
            ey = ((fy * Y2) * iz + cy) - v2;
            if ((ex * ex + ey * ey) > th2) ok = false;
            if (ok) { flag = c < kCos ? 3 : 1; cosp = c; }
        }
        if (i < n) {
            good[i] = (uint8_t)flag;
            p3d[3 * (size_t)i] = x; p3d[3 * (size_t)i + 1] = y; p3d[3 * (size_t)i + 2] = z;
        }
        // the counted cosines, packed: a wave takes its places with one add (which wave comes first
        // does not matter: the selection below is order-free), a lane its rank in the ballot
        const unsigned long long bal = __ballot(flag != 0);
        const int c = __popcll(bal);
        int base = 0;
        if (lane == 0 && c) base = atomicAdd(&s_good, c);
        base = __shfl(base, 0);
        if (flag) s_cos[base + __popcll(bal & ((1ull << lane) - 1ull))] = cosp;
    }
    __syncthreads();
    const int n_good = s_good;
    if (n_good > 0) {   // uniform over the work-group
        // the k-th smallest cosine without a sort: the least key K with more than k keys <= K, by
        // bisection over the 32 bits of the order-preserving key; a step counts the keys <= mid
        // (n_good / 256 per thread, one LDS counter per step). K is the key of a counted cosine,
        // and counts do not depend on any order. (-0 lies below +0 here; a NaN, which a counted
        // point has only in a camera centre, above every number.)
        const int k = min(50, n_good - 1);
        unsigned lo = 0u, hi = 0xFFFFFFFFu;
        for (int step = 0; step < 32; step++) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            int c = 0;
            for (int i = tid; i < n_good; i += kTvThreads) c += tv_order_key(s_cos[i]) <= mid;
            c = wave_sum_i32(c);
            if (lane == 0 && c) atomicAdd(&s_cnt[step], c);
            __syncthreads();
            if (s_cnt[step] > k) hi = mid;
            else lo = mid + 1u;
        }
        if (tid == 0) s_sel = tv_order_value(lo);
    }
    __syncthreads();
    if (tid == 0) {
        float* hf = (float*)P.head;
        P.head[kHdGood + m] = n_good;
        if (n_good > 0) {
            hf[kHdCos + m] = s_sel;
            hf[kHdPar + m] = (float)((double)(acosf(s_sel) * 180.0f) / 3.14159265358979323846);
        }
    }
}

// ---- k_tvr_final ----
__global__ __launch_bounds__(kTvThreads) void k_tvr_final(const TvDev* __restrict__ probs) {
    __shared__ int s_chosen;
    const TvDev& P = probs[blockIdx.x];
    const int tid = threadIdx.x, n = P.n;
    if (tid == 0) {
        const float* hf = (const float*)P.head;
        const int model = P.head[kHdModel], n_mot = P.head[kHdMot], n_inl = P.head[kHdInl];
        const int* g = P.head + kHdGood;
        const float minParallax = 1.0f;
        const int minTriangulated = 50;
        int chosen = -1;
        if (model == 1) {
            int maxGood = g[0];
            for (int i = 1; i < 4; i++) maxGood = max(maxGood, g[i]);
            const int nMinGood = max((int)(0.9 * (double)n_inl), minTriangulated);
            int nsimilar = 0;
            for (int i = 0; i < 4; i++) nsimilar += (double)g[i] > 0.7 * (double)maxGood;
            if (!(maxGood < nMinGood || nsimilar > 1)) {
                int k = 0;
                for (int i = 3; i >= 0; i--)
                    if (g[i] == maxGood) k = i;
                if (hf[kHdPar + k] > minParallax) chosen = k;
            }
        } else if (model == 0 && n_mot > 0) {
            int best = 0, second = 0, k = -1;
            float par = -1.0f;
            for (int i = 0; i < 8; i++) {
                if (g[i] > best) { second = best; best = g[i]; k = i; par = hf[kHdPar + i]; }
                else if (g[i] > second) second = g[i];
            }
            if ((double)second < 0.75 * (double)best && par >= minParallax && best > minTriangulated &&
                (double)best > 0.9 * (double)n_inl)
                chosen = k;
        }
        P.head[kHdChosen] = chosen;
        P.head[kHdSuccess] = chosen >= 0;
        if (chosen >= 0) {
            float* out = (float*)P.head;
            for (int i = 0; i < 9; i++) out[kHdR21 + i] = P.mot[12 * chosen + i];
            for (int i = 0; i < 3; i++) out[kHdT21 + i] = P.mot[12 * chosen + 9 + i];
        }
        s_chosen = chosen;
    }
    __syncthreads();
    const int chosen = s_chosen;
    for (int i = tid; i < n; i += kTvThreads) {
        const int flag = chosen >= 0 ? P.good[(size_t)chosen * n + i] : 0;
        const float* src = P.p3d + ((size_t)max(chosen, 0) * n + i) * 3;
        P.out_tri[i] = (uint8_t)(flag == 3);
        P.out_p3d[3 * (size_t)i] = flag ? src[0] : 0.f;
        P.out_p3d[3 * (size_t)i + 1] = flag ? src[1] : 0.f;
        P.out_p3d[3 * (size_t)i + 2] = flag ? src[2] : 0.f;
    }
}

// ---- host ----
// Normalize over the n matches' keypoints: upstream's running fp32 sums in match order; T and, in
// closed form, its inverse
static void tv_normalize(const float* x, const float* y, int n, float* xn, float* yn, float* T, float* Tinv) {
    float mx = 0.f, my = 0.f;
    for (int i = 0; i < n; i++) { mx += x[i]; my += y[i]; }
    mx = mx / (float)n;
    my = my / (float)n;
    float dx = 0.f, dy = 0.f;
    for (int i = 0; i < n; i++) {
        xn[i] = x[i] - mx;
        yn[i] = y[i] - my;
        dx += std::fabs(xn[i]);
        dy += std::fabs(yn[i]);
    }
    dx = dx / (float)n;
    dy = dy / (float)n;
    const float sx = 1.0f / dx, sy = 1.0f / dy;
    for (int i = 0; i < n; i++) { xn[i] = xn[i] * sx; yn[i] = yn[i] * sy; }
    const float t[9] = {sx, 0.f, -mx * sx, 0.f, sy, -my * sy, 0.f, 0.f, 1.f};
    const float ti[9] = {1.0f / sx, 0.f, mx, 0.f, 1.0f / sy, my, 0.f, 0.f, 1.f};
    for (int i = 0; i < 9; i++) { T[i] = t[i]; Tinv[i] = ti[i]; }
}

// the argument check; *n_out = the number of matches
static int tv_check(const orbhip_two_view_problem& p, const orbhip_two_view_result& r, int* n_out) {
    if (p.n1 < 8 || p.n2 < 1 || p.n_hyp < 1) return ORBHIP_ERR_ARG;
    if (!p.kps1 || !p.kps2 || !p.matches12 || !p.sets || !r.p3d || !r.triangulated) return ORBHIP_ERR_ARG;
    if (!(p.K[0] > 0.0f) || !(p.K[1] > 0.0f) || !std::isfinite(p.K[0]) || !std::isfinite(p.K[1]) ||
        !(p.sigma > 0.0f) || !std::isfinite(p.sigma))
        return ORBHIP_ERR_ARG;
    int n = 0;
    for (int i = 0; i < p.n1; i++) {
        const int32_t m = p.matches12[i];
        if (m < -1 || m >= p.n2) return ORBHIP_ERR_ARG;
        n += m >= 0;
    }
    if (n < 8) return ORBHIP_ERR_ARG;   // upstream would never leave its draw loop
    if (n > kTvMaxN || p.n_hyp > kTvMaxHyp) return ORBHIP_ERR_UNSUPPORTED;
    for (int h = 0; h < p.n_hyp; h++) {   // an index past the matches would be read on the device
        const int32_t* s = p.sets + 8 * (size_t)h;
        for (int a = 0; a < 8; a++) {
            if ((unsigned)s[a] >= (unsigned)n) return ORBHIP_ERR_ARG;
            for (int b = 0; b < a; b++)
                if (s[a] == s[b]) return ORBHIP_ERR_ARG;
        }
    }
    *n_out = n;
    return ORBHIP_OK;
}

int two_view_batch(StageBlock& S, StageTimer& timer, hipStream_t st, const orbhip_two_view_problem* probs, int B,
                   orbhip_two_view_result* res) {
    if (B < 0) return ORBHIP_ERR_ARG;
    if (B == 0) return 0;
    if (!probs || !res) return ORBHIP_ERR_ARG;
    if (B > kTvMaxBatch) return ORBHIP_ERR_UNSUPPORTED;
    int N[kTvMaxBatch];
    for (int b = 0; b < B; b++)
        if (const int rc = tv_check(probs[b], res[b], &N[b])) return rc;
    // one block, the same layout on the host (pinned) and the device:
    // [problems B | per problem: x1 y1 x2 y2 xn1 yn1 xn2 yn2 sets] uploaded; device only [scores,
    // matrices, masks, motions, CheckRT's flags and points]; read back [heads B x 64 words | per
    // problem: the two masks and the chosen model's | out_tri | out_p3d]
    struct Off { size_t pts, sets, score, mat, mask, mot, good, p3d, inl, tri, out; };
    Off off[kTvMaxBatch];
    StageLayout lay(16);
    const size_t o_probs = lay.take((size_t)B * sizeof(TvDev));
    int max_h = 0;
    for (int b = 0; b < B; b++) {
        off[b].pts = lay.take((size_t)N[b] * 8 * 4);
        off[b].sets = lay.take((size_t)probs[b].n_hyp * 8 * 4);
        max_h = probs[b].n_hyp > max_h ? probs[b].n_hyp : max_h;
    }
    const size_t up_bytes = lay.total();
    for (int b = 0; b < B; b++) {
        const size_t n = (size_t)N[b], H = (size_t)probs[b].n_hyp;
        off[b].score = lay.take(2 * H * 4);
        off[b].mat = lay.take(2 * H * 9 * 4);
        off[b].mask = lay.take(2 * H * ((n + 63) / 64) * 8);
        off[b].mot = lay.take(8 * 12 * 4);
        off[b].good = lay.take(8 * n);
        off[b].p3d = lay.take(8 * n * 12);
    }
    const size_t o_head = lay.take((size_t)B * kTvHead * 4);
    for (int b = 0; b < B; b++) {
        const size_t n = (size_t)N[b];
        off[b].inl = lay.take(3 * n);
        off[b].tri = lay.take(n);
        off[b].out = lay.take(n * 12);
    }
    const size_t back_bytes = lay.total() - o_head;
    HIPOK(S.ensure(lay.total(), up_bytes + back_bytes + 16));
    uint8_t* const d = S.d;
    uint8_t* const h = S.h;
    TvDev* dev = (TvDev*)(h + o_probs);
    for (int b = 0; b < B; b++) {
        const orbhip_two_view_problem& p = probs[b];
        const int n = N[b];
        float* pts = (float*)(h + off[b].pts);
        float *x1 = pts, *y1 = pts + n, *x2 = pts + 2 * n, *y2 = pts + 3 * n;
        for (int i = 0, k = 0; i < p.n1; i++) {   // mvMatches12: the pairs (i, matches12[i]) in index order
            const int32_t m = p.matches12[i];
            if (m < 0) continue;
            x1[k] = p.kps1[i].x; y1[k] = p.kps1[i].y;
            x2[k] = p.kps2[m].x; y2[k] = p.kps2[m].y;
            k++;
        }
        TvDev& v = dev[b];
        float T1[9], T1inv[9], T2[9];
        tv_normalize(x1, y1, n, pts + 4 * n, pts + 5 * n, T1, T1inv);
        tv_normalize(x2, y2, n, pts + 6 * n, pts + 7 * n, T2, v.T2inv);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) { v.T1[3 * i + j] = T1[3 * i + j]; v.T2t[3 * i + j] = T2[3 * j + i]; }
        S.put(off[b].sets, p.sets, (size_t)p.n_hyp * 32);
        const float* dp = (const float*)(d + off[b].pts);
        v.x1 = dp; v.y1 = dp + n; v.x2 = dp + 2 * n; v.y2 = dp + 3 * n;
        v.xn1 = dp + 4 * n; v.yn1 = dp + 5 * n; v.xn2 = dp + 6 * n; v.yn2 = dp + 7 * n;
        v.sets = (const int32_t*)(d + off[b].sets);
        v.score = (float*)(d + off[b].score);
        v.mat = (float*)(d + off[b].mat);
        v.mask = (unsigned long long*)(d + off[b].mask);
        v.head = (int32_t*)(d + o_head + (size_t)b * kTvHead * 4);
        v.mot = (float*)(d + off[b].mot);
        v.inl = d + off[b].inl;
        v.good = d + off[b].good;
        v.p3d = (float*)(d + off[b].p3d);
        v.out_p3d = (float*)(d + off[b].out);
        v.out_tri = d + off[b].tri;
        for (int k = 0; k < 4; k++) v.K[k] = p.K[k];
        v.inv_sigma2 = (float)(1.0 / (double)(p.sigma * p.sigma));
        v.th2 = 4.0f * (p.sigma * p.sigma);
        v.n = n; v.H = p.n_hyp; v.words = (n + 63) / 64; v.pad = 0;
    }
    HIPOK(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    {
        const StageScope scope(timer);
        const TvDev* dp = (const TvDev*)(d + o_probs);
        timer.begin(16, st);
        ORBHIP_LAUNCH(k_tvr_ransac, dim3((unsigned)((2 * max_h + kTvWaves - 1) / kTvWaves), (unsigned)B),
                      dim3(64 * kTvWaves), 0, st, dp);
        ORBHIP_LAUNCH(k_tvr_select, dim3((unsigned)B), dim3(kTvThreads), 0, st, dp);
        ORBHIP_LAUNCH(k_tvr_check_rt, dim3(8u, (unsigned)B), dim3(kTvThreads), 0, st, dp);
        ORBHIP_LAUNCH(k_tvr_final, dim3((unsigned)B), dim3(kTvThreads), 0, st, dp);
        timer.end(16, st);
    }
    HIPOK(hipGetLastError());
    uint8_t* const hb = h + up_bytes;   // the read-back lies behind the upload in the pinned image
    HIPOK(hipMemcpyAsync(hb, d + o_head, back_bytes, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    auto back = [&](size_t o) { return hb + (o - o_head); };
    for (int b = 0; b < B; b++) {   // nothing is written before every problem's head is known to be sane
        const int32_t* head = (const int32_t*)back(o_head + (size_t)b * kTvHead * 4);
        const int H = probs[b].n_hyp;
        if (head[kHdBestH] < -1 || head[kHdBestH] >= H || head[kHdBestF] < -1 || head[kHdBestF] >= H ||
            head[kHdModel] < -1 || head[kHdModel] > 1 || head[kHdChosen] < -1 || head[kHdChosen] >= 8)
            return ORBHIP_ERR_DEVICE;
    }
    int nok = 0;
    for (int b = 0; b < B; b++) {
        const orbhip_two_view_problem& p = probs[b];
        orbhip_two_view_result& r = res[b];
        const size_t n = (size_t)N[b];
        const int32_t* head = (const int32_t*)back(o_head + (size_t)b * kTvHead * 4);
        const float* hf = (const float*)head;
        r.success = head[kHdSuccess]; r.model = head[kHdModel];
        r.best_h = head[kHdBestH]; r.best_f = head[kHdBestF]; r.chosen = head[kHdChosen];
        r.SH = hf[kHdSH]; r.SF = hf[kHdSF];
        std::memcpy(r.H21, hf + kHdH21, 36);
        std::memcpy(r.F21, hf + kHdF21, 36);
        std::memcpy(r.R21, hf + kHdR21, 36);
        std::memcpy(r.t21, hf + kHdT21, 12);
        std::memcpy(r.n_good, head + kHdGood, 32);
        std::memcpy(r.parallax, hf + kHdPar, 32);
        std::memcpy(r.cos_sel, hf + kHdCos, 32);
        if (r.inliers_h) std::memcpy(r.inliers_h, back(off[b].inl), n);
        if (r.inliers_f) std::memcpy(r.inliers_f, back(off[b].inl) + n, n);
        std::memset(r.p3d, 0, (size_t)p.n1 * 12);
        std::memset(r.triangulated, 0, (size_t)p.n1);
        const uint8_t* tri = back(off[b].tri);
        const float* out = (const float*)back(off[b].out);
        for (int i = 0, k = 0; i < p.n1; i++) {
            if (p.matches12[i] < 0) continue;
            std::memcpy(r.p3d + 3 * (size_t)i, out + 3 * (size_t)k, 12);
            r.triangulated[i] = tri[k];
            k++;
        }
        nok += r.success != 0;
    }
    return nok;
}

}  // namespace orbhip
